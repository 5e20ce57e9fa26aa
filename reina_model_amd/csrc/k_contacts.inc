// reina_hip.hip part: k_day -- the streaming scan and the contact sampling of a day in ONE kernel.
// Included by reina_hip.hip only (one translation unit); not a standalone header.
// ---------------------------------------------------------------------------------------------
// k_day: Context._iterate_people (main.pyx:1982-1992) = person_advance for every agent (k_scan.inc) and, for
// the infectious ones, get_one_contact / get_person_from_age_range / person_expose / did_infect
// (main.pyx:1290-1304,1525-1535,238-244,908-934).
//
// They share a kernel AND a wave.  A wave finds the agents of its tiles (512 agents each) that have something to do today --
// on a SPARSE day from the tiles' 64 bytes of the ACTIVE bit plane, fetching the words of the agents whose bit is set (every
// day of a population of >= 4 tiles per wave: round 4); on a DENSE day by streaming the tiles' hot words themselves, three
// tiles in flight --, queues them with their words, runs the state machine on 64 of them at a time, pushes the infectious
// ones onto its LDS strip, and whenever 64 of those are pending it draws their contact counts and samples their contacts,
// one lane per contact, before it goes on.  Nothing in that cycle waits for HBM except the fetch (requested one step
// ahead) and the few contacts that survive the thinning (their targets' bits, requested a batch ahead); the exposure
// records never leave LDS.  Contact tables (one row per DISTINCT row of the matrix, Tables) are staged in LDS once per
// workgroup, behind the wave's first loads.  On a day with weekly imports the launch's last workgroups place them beside
// all this (k_open.inc: day_imports_block).
//
// Everything a contact decides is keyed by (source, day, contact number), so results do not depend on which
// wave samples it, in which batch or in which order: bit-identical to oracle B's sequential loops.
// Diagnostic builds (reina_diag.h; tools/diag.py builds and reads them): -DREINA_DAY_PROF=<part> -- every wave sums the shader-clock
// cycles of its whole loop and of ONE named part of it (PROF_BEGIN / PROF_END / PROF_IS; the names: DIAG_PROF_PARTS) and lane 0 writes them as the
// wave's row of the map's WAVES region when the wave is through --, -DREINA_DAY_STAMPS, -DREINA_ABLATE (ABLATED).
#define NEEDY_ENTRIES 128                     // queued (agent, word) pairs: fewer than 64 carried over + at most 64 per feeding step
#define DAY_XSTAGE (REINA_PRESSURE_WORDS / 2 - 1)   // exact attribution: contact records a workgroup stages in LDS (the pressure block's 8 KB: a count + 1023 records)

struct DayShared {
    uint32_t meta_row[REINA_MAX_ENTRIES];   // shared (place, range) pattern when every row has the same
    float mask_p[REINA_MAX_AGES][8];
    float p_sus[REINA_MAX_VARIANTS][REINA_MAX_AGES];
    int32_t age_start[REINA_MAX_AGES + 1];
    int32_t rcount[REINA_MAX_AGES];         // entries per distinct row
    uint8_t row_of_age[REINA_MAX_AGES];
    uint8_t age_block[REINA_AGE_BLOCKS];
    uint32_t pre[DAY_WAVES][64];            // inclusive prefix of contact counts per wave batch
    uint4 item[DAY_WAVES][64];              // the wave's current 64 sources
    int32_t daily[REINA_NR_PLACES];
    int32_t n_contacts;
    int32_t n_active;                       // agents the workgroup's stream queued today (-> REINA_L_ACTIVE)
    int32_t n_hosp, n_icu;                  // the workgroup's admission / ICU-transfer requests of the day (-> REINA_L_EV_*)
    float iot[REINA_MAX_VARIANTS][REINA_IOT_LEN + 3];
    // per variant: p_asymptomatic_infection, psus_max, infectiousness_multiplier, iot_mask (bits) -- what the state machine and
    // the count draw index by an agent's variant (from the parameter block in HBM that was a vector load, i.e. a round trip
    // to L2, in every state-machine round and three at the head of every contact batch)
    uint32_t var_par[REINA_MAX_VARIANTS][4];
    uint8_t crow_of_age[REINA_MAX_AGES];     // count row (thresholds of the contact COUNT) of every age
    uint2 needy[DAY_WAVES][NEEDY_ENTRIES];      // (agent, hot word) awaiting the state machine
    uint32_t idxq[DAY_WAVES][NEEDY_ENTRIES];    // sparse day: agents whose bit is set, awaiting the fetch of their word
    unsigned long long ev_key[DAY_EV_STAGE];    // the workgroup's bed / ICU events of the day (keys as in the buckets)
    uint32_t ev_n;
    uint2 strip[DAY_WAVES][128];            // infectious agents awaiting their contacts (< 64 carried + 64 per round)
    uint32_t own_cnt[DAY_WAVES][64];         // sources whose contacts end at each position of the step's window (contact_batch)
    // contacts that can transmit, awaiting their target: self-contained records (source | contact number, table entry,
    // source age, variant, has-list | source infectiousness bits) that outlive the batch that found them, so a wave
    // resolves them 64 at a time whatever the batch sizes: 64 target gathers in flight per resolve instead of the dozen a
    // batch of 64 sources leaves behind
    uint32_t pend_src[DAY_WAVES][128];
    uint32_t pend_info[DAY_WAVES][128];
    uint32_t pend_inf[DAY_WAVES][128];
    // the words of the infected plane that hold the bits of the targets in flight: written by the gather itself (LDS-DMA,
    // resolve_issue), read by resolve_finish after its own wait
    uint32_t pend_bits[DAY_WAVES][64];
    uint32_t grp[REINA_LDS_ROWS][8];        // place groups of the staged contact rows (k_common.inc: Tables::grp)
    // dynamic tail: uint32_t thr[lds_rows][REINA_MAX_ENTRIES]; uint8_t guide[lds_rows][256];
    // uint32_t cthr[lds_crows][REINA_COUNT_WORDS]; uint8_t cguide[lds_crows][256]; when sharded
    // int32_t pressure[REINA_PRESSURE_WORDS] (this workgroup's outgoing cross-shard pressure)
};
#define DAY_ROW_BYTES (REINA_MAX_ENTRIES * 4 + 256)
#define DAY_CROW_BYTES (REINA_COUNT_WORDS * 4 + 256)
static_assert(sizeof(DayShared) + (size_t)REINA_LDS_ROWS * DAY_ROW_BYTES + (size_t)REINA_LDS_CROWS * DAY_CROW_BYTES + REINA_PRESSURE_WORDS * 4 <= 160 * 1024 - 3072,
              "k_day's LDS image (sharded, REINA_LDS_ROWS contact rows, REINA_LDS_CROWS count rows) must fit one CU beside up to 3 KB of static LDS (tests/test_abi.py)");
static size_t day_shared_bytes(uint32_t lds_rows, uint32_t lds_crows, uint32_t n_shards) {
    return sizeof(DayShared) + (size_t)lds_rows * DAY_ROW_BYTES + (size_t)lds_crows * DAY_CROW_BYTES + (n_shards > 1 ? REINA_PRESSURE_WORDS * 4 : 0);
}

// adds a lane's packed per-place counts to the workgroup histogram: wave sums first, one LDS atomic per
// place and wave
__device__ __forceinline__ void flush_places(int32_t *daily, uint32_t lo, uint32_t hi) {
#pragma unroll
    for (int pl = 0; pl < REINA_NR_PLACES; pl++) {
        const int c = wave_sum((int)(((pl < 3 ? lo : hi) >> (10 * (pl % 3))) & 1023u));
        if (c && lane_id() == 0) atomicAdd(&daily[pl], c);
    }
}

// inclusive prefix sum over the 64 lanes in six cross-lane VALU moves (row_shr 1, 2, 4, 8; row_bcast 15 -> rows 1, 3;
// row_bcast 31 -> rows 2, 3): no LDS round trip, no scalar instruction -- the shuffle form (ds_bpermute) was six
// dependent LDS operations with a compare each
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
    return v;
}

// what a wave carries through its batches
struct ContactState {
    uint32_t n_cand;                 // candidate records written to the wave's region so far
    uint32_t slice_base, slice_cap;
    uint32_t wave_contacts;
    uint64_t pl;          // this lane's contacts by place, 10 bits per place
    uint32_t pl_rounds;
    // pending records of the wave (LDS: DayShared::pend_*, two regions of 64): region `cur` is being filled (n_pend records),
    // the other one holds the 64 records whose targets' bits are in flight (fl = their number, 0: none; fl_t: this lane's target;
    // the word of the infected plane that holds its bit lands in DayShared::pend_bits
    // lane's target and the word of the infected plane that holds its bit)
    uint32_t n_pend, cur, fl;
    uint32_t fl_t;
    // the key of the contacts' draws (rp_contact_key of the engine's Philox key), made opaque to the compiler at the kernel's
    // head: left as an expression of P->k0 / P->k1 it was "rematerialised" where it is used -- a scalar load, a wait for it AND for
    // every vector-memory operation of the wave in flight, a multiply, an add and an xor in front of every step of 64 contacts
    uint32_t ckey;
    // ... and the parameters the batches and the resolve steps ask at every turn, pinned the same way (each was a scalar load and a
    // wait of its own where it was used: five in a row per resolve turn)
    uint32_t n_shards, shard_rank, age_shift, nr_ages;
    PROF_IN_MEMBERS;   // (REINA_DAY_PROF: the sums of a part that lies inside contact_batch)
};

// The contacts that CAN transmit -- contacts whose transmission draw lies below the source's largest possible transmission
// probability -- resolved 64 at a time.  Only these need a target: get_person_from_age_range, person_expose, did_infect
// (main.pyx:1525-1535,238-244,908-934).  Round 4: in TWO steps with the wave's other work between them.  resolve_issue
// draws the targets of the 64 records of one region of the pending list and REQUESTS the words of the infected bit plane
// (buffers.infected_bits: a table of N / 8 bytes that stays in the Infinity Cache; rounds 1-3 gathered the targets' hot
// words from HBM for one bit of each); resolve_finish, one batch of records or one pass of the stream later, tests the
// bits, applies the targets' susceptibility and claims.  A wave waited for every batch's gather before (30 times 2-4 us a
// wave on the peak day at 10^8 agents); now the gather is in flight while the next contacts are sampled.
// The contact's draws are recomputed in either step (for one contact in fifty that costs less than carrying four more words
// per contact through LDS).
// get_one_contact (main.pyx:1290-1304) by inversion: the entry of contact row `row` (cnt entries) that the draw r0 selects --
// the first one with r0 < threshold (thresholds are non-decreasing), the last one when there is none -- and its meta word.
// The guide gives the first entry above the draw's top byte; the next two thresholds and the three meta words they choose
// between come in ONE look (one wait instead of two to four), the rare longer walk goes step by step.  Needed by the contacts
// that pass the thinning (their age range: resolve_*) and, where the place groups cannot serve, by every contact for its place.
__device__ __forceinline__ uint32_t contact_entry(const CAS Tables *T, const DayShared &S, const uint32_t (*S_thr)[REINA_MAX_ENTRIES],
                                                  const uint8_t (*S_guide)[256], uint32_t lds_rows, uint32_t uniform_meta,
                                                  uint32_t row, int cnt, uint32_t r0, uint32_t *l2_out) {
    int l2;
    uint32_t m;
    if (row < lds_rows) {
        l2 = S_guide[row][r0 >> 24];
        const uint32_t t0 = S_thr[row][l2], t1 = S_thr[row][l2 + 1];   // (past a row's end: the next row or the guides, never used)
        uint32_t m0 = 0, m1 = 0, m2 = 0;
        if (uniform_meta) { m0 = S.meta_row[l2]; m1 = S.meta_row[l2 + 1]; m2 = S.meta_row[l2 + 2]; }
        m = m0;
        if (l2 < cnt - 1 && r0 >= t0) {
            l2++;
            m = m1;
            if (l2 < cnt - 1 && r0 >= t1) {
                l2++;
                m = m2;
                if (l2 < cnt - 1 && r0 >= S_thr[row][l2]) {
                    do l2++; while (l2 < cnt - 1 && r0 >= S_thr[row][l2]);
                    m = S.meta_row[l2];
                }
            }
        }
        if (!uniform_meta) m = LD_U32_NOW(T->meta[row][l2]);   // (the reads through L2: k_common.inc, ld_u32_now)
    } else {   // more distinct rows than the LDS image holds: this one is read through L2
        l2 = (int)LD_U8_NOW(T->guide[row][r0 >> 24]);
        while (l2 < cnt - 1 && r0 >= LD_U32_NOW(T->thr[row][l2])) l2++;
        m = uniform_meta ? S.meta_row[l2] : LD_U32_NOW(T->meta[row][l2]);
    }
    *l2_out = (uint32_t)l2;
    return m;
}
__device__ __forceinline__ uint32_t resolve_target(uint32_t n_shards, const DayShared &S, const reina_day_t &dp, uint32_t ckey, uint32_t src,
                                                   uint32_t c, uint32_t m, uint32_t *dest_out) {
    const rp_u2 q1 = rp_philox2(ckey, src, rp_contact_ctr(dp.day, c, 1));
    const int cmin = (int)((m >> 8) & 0xFFu), cmax = (int)((m >> 16) & 0xFFu);
    const uint32_t start = (uint32_t)S.age_start[cmin], end = (uint32_t)S.age_start[cmax + 1];
    // uniform member of the range over the WHOLE population: uniform shard, then uniform agent of that shard (every shard
    // holds 1/G of every age; an unsharded population skips the two integer divisions: x % 1 = 0, x / 1 = x)
    *dest_out = n_shards > 1 ? q1.v[0] % n_shards : 0u;
    if (end <= start) return 0xFFFFFFFFu;
    return start + (n_shards > 1 ? q1.v[0] / n_shards : q1.v[0]) % (end - start);
}
__device__ __forceinline__ void resolve_issue(const CAS DevParams *P, const CAS Tables *T, const GBuffers &B, DayShared &S,
                                              const uint32_t (*S_thr)[REINA_MAX_ENTRIES], const uint8_t (*S_guide)[256], uint32_t lds_rows,
                                              uint32_t uniform_meta, const reina_day_t &dp, uint32_t first, uint32_t n, ContactState &C) {
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    C.fl_t = 0xFFFFFFFFu;
    // (wave-uniform LDS byte address of the wave's row: an LDS pointer's low 32 bits)
    const uint32_t lds_row = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t *)&S.pend_bits[wave][0]);
    if ((uint32_t)lane < n) {
        // the contact's table entry (the sampling loop found only its place: contact_batch), kept in the record for
        // resolve_finish; then the target
        uint32_t dest, l2;
        const uint32_t src = S.pend_src[wave][first + lane], pe = S.pend_info[wave][first + lane];
        const uint32_t c = pe & 0xFFu, row = S.row_of_age[(pe >> 16) & 0x7Fu];
        const uint32_t ckey = C.ckey;
        const uint32_t r0 = rp_philox2(ckey, src, rp_contact_ctr(dp.day, c, 0)).v[0];
        const uint32_t m = contact_entry(T, S, S_thr, S_guide, lds_rows, uniform_meta, row, S.rcount[row], r0, &l2);
        S.pend_info[wave][first + lane] = pe | (l2 << 8);
        const uint32_t t = resolve_target(C.n_shards, S, dp, ckey, src, c, m, &dest);
        if (dest == C.shard_rank && t != 0xFFFFFFFFu) {
            C.fl_t = t;
            // The gather writes LDS itself (global_load_lds_dword: M0 + 4 x lane, the lanes that are off write nothing): with a
            // register as its destination the compiler, which copies loop-carried registers at the contact loop's back edge, put
            // s_waitcnt vmcnt(0) in front of that copy -- every step of 64 contacts waited for the gather it had just issued (and
            // for the stream's fetch: round 4's "pipelining gains nothing" was this wait).  The compiler does not count an asm
            // load; resolve_finish waits for it by hand.
            const GAS uint32_t *gp = &B.infected_bits[t >> 5];
            uint32_t keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %1, off\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(gp), "s"(lds_row) : "memory");
        }
    }
    C.fl = n;
}
template <class PT>
__device__ __forceinline__ void resolve_finish(PT P, const CAS Tables *T, const GBuffers &B, DayShared &S,
                                               int32_t *S_pressure, uint32_t uniform_meta, const reina_day_t &dp,
                                               uint32_t first, ContactState &C) {
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const CAS reina_disease_t &d = P->dis;
    const uint32_t shard_rank = C.shard_rank;
    const uint32_t n = C.fl;
    C.fl = 0;
    // the gather has landed (everything else the wave has in flight too: the next fetch of the stream is issued after this)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    bool hit = false;
    uint4 cand = make_uint4(0xFFFFFFFFu, 0, 0, 0);
    if (ABLATED(RESOLVE)) return;
    if ((uint32_t)lane < n) {
        const uint32_t src = S.pend_src[wave][first + lane], pe = S.pend_info[wave][first + lane];
        const uint32_t c = pe & 0xFFu, l2 = (pe >> 8) & 0xFFu;
        const float src_inf = rp_u2f(S.pend_inf[wave][first + lane]);
        const int age_s = (int)((pe >> 16) & 0x7Fu), v = (int)((pe >> 24) & 3u);
        const uint32_t has_list = pe >> 31;
        const uint32_t row = S.row_of_age[age_s];
        // the contact's draws (Philox2x32 twice): q0.v[1] transmission (the draw that passed the thinning), q1.v[0] shard +
        // target (resolve_target), q1.v[1] mask; its place / range draw came with the list (l2)
        const uint32_t ckey = C.ckey;
        const uint32_t r2 = rp_philox2(ckey, src, rp_contact_ctr(dp.day, c, 0)).v[1];
        const uint32_t m = uniform_meta ? S.meta_row[l2] : LD_U32_NOW(T->meta[row][l2]);
        const int place = (int)(m & 0xFFu);
        const int cmax = (int)((m >> 16) & 0xFFu);
        const uint32_t t = C.fl_t;
        uint32_t dest = shard_rank;
        if (C.n_shards > 1) dest = rp_philox2(ckey, src, rp_contact_ctr(dp.day, c, 1)).v[0] % C.n_shards;
        if (dest != shard_rank && IS_EXACT(P)) {
            // exact attribution: the source completes did_infect (main.pyx:908-934) itself -- age ranges are global knowledge,
            // so it draws the target on the other shard and knows its age -- and sends (target, source id, variant, list flag);
            // all the destination adds is person_expose's test (main.pyx:239) and the claim (k_remote.inc)
            const int cmin = (int)((m >> 8) & 0xFFu);
            const CAS int32_t *das = P->shard_age_start[dest];
            const uint32_t ds = (uint32_t)das[cmin], de = (uint32_t)das[cmax + 1];
            if (de > ds) {
                const rp_u2 q1 = rp_philox2(ckey, src, rp_contact_ctr(dp.day, c, 1));
                const uint32_t tt = ds + (q1.v[0] / C.n_shards) % (de - ds);
                const int age_t = age_of(das, tt, cmin, cmax);
                bool pass = rp_chance(src_inf * S.p_sus[v][age_t] * rp_u2f(S.var_par[v][2]), r2) != 0;
                const float mp = S.mask_p[age_s][place];
                if (pass && mp != 0.0f) {
                    float a = mp * LD_F32_NOW(d.p_mask_protects_others[v]);
                    float b = mp * LD_F32_NOW(d.p_mask_protects_wearer[v]);
                    float pm = a + b - a * b;
                    if (rp_chance(pm, q1.v[1])) pass = false;
                }
                if (pass) {
                    // the record waits in the workgroup's stage (the LDS block that holds the pressure counts under mirror
                    // attribution) and goes to its segment when the stream is through: a slot from a returning GLOBAL atomic
                    // here put a round trip into every resolve step (k_day 50 -> 68 us on a peak day of 8 x 1.25 x 10^7 agents).
                    // (staged with the DESTINATION in the id's shard bits: the source's own shard is put back at the flush)
                    const uint32_t pos = atomicAdd(reinterpret_cast<uint32_t *>(&S_pressure[0]), 1u);
                    if (pos < DAY_XSTAGE) {
                        const uint64_t r = rp_xrec(tt, (uint32_t)v | (has_list << 2), (dest << RP_GID_SHIFT) | src);
                        S_pressure[2u + 2u * pos] = (int32_t)(uint32_t)r;
                        S_pressure[3u + 2u * pos] = (int32_t)(uint32_t)(r >> 32);
                    } else xsend_push(P, B, dest, rp_xrec(tt, (uint32_t)v | (has_list << 2), (uint32_t)gid_of(P, src)));
                }
            }
        } else if (dest != shard_rank) {
            // source-side part of did_infect: the draw passed src_inf * psus_max * multiplier (that is what put
            // the contact on this list); the destination applies p_sus / psus_max
            bool pass = true;
            const float mp = S.mask_p[age_s][place];
            if (mp != 0.0f) {
                float a = mp * LD_F32_NOW(d.p_mask_protects_others[v]);
                float b = mp * LD_F32_NOW(d.p_mask_protects_wearer[v]);
                float pm = a + b - a * b;
                if (rp_chance(pm, rp_philox2(ckey, src, rp_contact_ctr(dp.day, c, 1)).v[1])) pass = false;
            }
            if (pass) {
                atomicAdd(&S_pressure[(dest * REINA_MAX_RANGES + (m >> 24)) * REINA_MAX_VARIANTS + (uint32_t)v], 1);
                // mirror table: smallest (tie-break, src) per slot, tagged with today
                rp_u4 hm = rp_philox(opaque_s(P->k0), opaque_s(P->k1), src, dp.day, RP_P_MIRROR, c);
                const uint32_t MS = P->mirror_slots, cell = (m >> 24) * REINA_MAX_VARIANTS + (uint32_t)v;
                const uint32_t eff = LD_U32_NOW(B.mirror_meta[cell]);   // slots of this cell in use today
                GAS uint64_t *slot = B.mirror + (size_t)cell * MS + (hm.v[0] & (eff - 1));
                atomicMin((unsigned long long *)slot, (unsigned long long)rp_order_key(dp.day, hm.v[1] >> 12, src));
                B.mirror_meta[REINA_MIRROR_CELLS + cell] = dp.day + 1;
            }
        } else if (t != 0xFFFFFFFFu) {
            // person_expose (main.pyx:239): only a never-infected target can be infected -- its bit of the infected plane
            // (no agent enters or leaves that state while k_day runs: infections are installed by the day's last launch)
            if (!((S.pend_bits[wave][lane] >> (t & 31u)) & 1u)) {
                // the target's age: coarse block table, then 0-1 steps
                int age_t = S.age_block[t >> C.age_shift];
                while (age_t < cmax && (uint32_t)S.age_start[age_t + 1] <= t) age_t++;
                float p = src_inf * S.p_sus[v][age_t] * rp_u2f(S.var_par[v][2]);
                if (rp_chance(p, r2)) {
                    hit = true;
                    const float mp = S.mask_p[age_s][place];
                    if (mp != 0.0f) {
                        float a = mp * LD_F32_NOW(d.p_mask_protects_others[v]);
                        float b = mp * LD_F32_NOW(d.p_mask_protects_wearer[v]);
                        float pm = a + b - a * b;
                        if (rp_chance(pm, rp_philox2(ckey, src, rp_contact_ctr(dp.day, c, 1)).v[1])) hit = false;
                    }
                    if (hit) {
                        // (the claim key and the record carry the source's GLOBAL id where the population keeps them)
                        // (the key's ten round keys are derived HERE, for one contact in five hundred: as loop invariants of the contact loop
                        // they occupied twenty scalar registers of a kernel that spills them)
                        const uint32_t prio = rp_priority20(opaque_s(P->k0), opaque_s(P->k1), src, dp.day);
                        atomicMin((unsigned long long *)&B.cold[t].claim, (unsigned long long)rp_order_key(dp.day, prio, (uint32_t)gid_of(P, src)));
                        cand = make_uint4(t, (uint32_t)gid_of(P, src), (uint32_t)v | (has_list << 8), prio);
                    }
                }
            }
        }
    }
    // candidate records: ballot slots in the wave's region, no atomics
    const uint64_t hm = __ballot(hit);
    if (hm) {
        if (hit) {
            const uint32_t pos = C.n_cand + (uint32_t)__popcll(hm & ((1ull << lane) - 1ull));
            if (pos < C.slice_cap) {
                gst(&reinterpret_cast<GAS uint4 *>(B.candidates)[C.slice_base + pos], cand);
            } else {
                // more successful attempts than the region holds (= than agents the wave scans: a dense
                // outbreak in a small population): a shared overflow list, one returning atomic per
                // record -- rare enough not to matter
                const uint32_t o = (uint32_t)atomicAdd(&B.control[REINA_L_CAND_OVF], 1);
                if (o < P->cand_ovf_cap)
                    gst(&reinterpret_cast<GAS uint4 *>(B.candidates)[P->cand_ovf_base + o], cand);
                else
                    set_problem(B.counters, REINA_PROBLEM_CANDIDATE_OVERFLOW);
            }
        }
        C.n_cand += (uint32_t)__popcll(hm);
    }
}
// the region being filled is full: the batch in flight is finished, this one requested, the regions change roles
template <class PT>
__device__ __forceinline__ void resolve_turn(PT P, const CAS Tables *T, const GBuffers &B, DayShared &S,
                                             const uint32_t (*S_thr)[REINA_MAX_ENTRIES], const uint8_t (*S_guide)[256], uint32_t lds_rows,
                                             int32_t *S_pressure, uint32_t uniform_meta, const reina_day_t &dp, ContactState &C) {
    __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): the wave-private records are written
    __builtin_amdgcn_wave_barrier();
    if (C.fl) resolve_finish(P, T, B, S, S_pressure, uniform_meta, dp, (C.cur ^ 1u) * 64u, C);
    resolve_issue(P, T, B, S, S_thr, S_guide, lds_rows, uniform_meta, dp, C.cur * 64u, C.n_pend, C);
    C.cur ^= 1u;
    C.n_pend = 0;
    __builtin_amdgcn_wave_barrier();
}

// Samples the contacts of the n <= 64 exposure records at rec[0..n) (LDS, this wave's).
// person_expose_others -> get_exposed_people -> get_nr_contacts (main.pyx:247-281,936-955,1308-1320): the
// scan recorded (agent, start-of-day word) of every infectious, undetected agent; its contact COUNT is drawn
// here, 64 agents at a time, then the wave's lanes are spread evenly over the contacts of the batch.
// Every contact gets its place (get_one_contact, main.pyx:1290-1304: daily_contacts counts them all) and its
// transmission draw; a contact whose draw is not below the source's LARGEST possible transmission probability
// (infectiousness x the most susceptible age x multiplier) cannot infect whoever it meets and ends there -- about
// forty-nine in fifty.  The others are collected and resolved densely, 64 at a time (resolve_issue / resolve_finish).  The outcome of
// every contact is exactly what sampling its target first would give.
template <class PT>
__device__ __forceinline__ void contact_batch(PT P, const CAS Tables *T, const GBuffers &B, DayShared &S,
                                              const uint32_t (*S_thr)[REINA_MAX_ENTRIES], const uint8_t (*S_guide)[256],
                                              const uint32_t (*S_cthr)[REINA_COUNT_WORDS], const uint8_t (*S_cguide)[256], uint32_t lds_crows,
                                              int32_t *S_pressure, uint32_t lds_rows, uint32_t uniform_meta, bool grouped, const reina_day_t &dp,
                                              const uint2 *rec, uint32_t n, ContactState &C, uint32_t day_flags) {
    const int lane = lane_id(), wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const CAS reina_disease_t &d = P->dis;
    uint4 it = make_uint4(0, 0, 0, 0);
    uint32_t nr = 0;
    PROF_IN_VAR(pb_);
    if (PROF_IS(BATCH_HEAD) || PROF_IS(BATCH_STEPS) || PROF_IS(HEAD_DRAIN) || PROF_IS(HEAD_DRAINED)) PROF_IN_MARK(pb_);
    if (PROF_IS(HEAD_DRAIN) || PROF_IS(HEAD_DRAINED)) {   // the wave's memory operations in flight drained at the head of a batch: the drain, or the head behind it
        PROF_DRAIN();
        if (PROF_IS(HEAD_DRAIN)) PROF_IN_ADD(C, pb_, 1u);
        PROF_IN_MARK(pb_);
    }
    if ((uint32_t)lane < n) {
        const uint2 ex = rec[lane];
        const uint32_t i = ex.x, w = ex.y;
        const uint32_t st = RH_STATE(w);
        const int v = RH_VARIANT(w), sev = RH_SEV(w);
        const int dayrel = st == RS_INCUBATION ? -(int)RH_DAYS_LEFT(w, dp.day) : (int)RH_DOI(w, dp.day);
        const float inf = S.iot[v][dayrel + 10];
        int age = S.age_block[i >> C.age_shift];
        while (age < (int)C.nr_ages - 1 && (uint32_t)S.age_start[age + 1] <= i) age++;
        // get_nr_contacts (main.pyx:1308-1320) by inversion: the day's draw against the thresholds of the agent's age
        // (reina_contacts.h: rc_count_thresholds) -- full class: from the guide entry of the draw's top byte, 0-2 steps;
        // an agent with symptoms (factor 0.5, limit 5): five comparisons
        const uint32_t rc = rp_count_draw_keyed(opaque_s(C.ckey), i, dp.day);
        const uint32_t crow = S.crow_of_age[age];
        const bool in_lds = crow < lds_crows;
        int nn;
        if (ABLATED(COUNT_DRAW)) {
            nn = (int)((i * 2654435761u) >> 30) + 1;
        } else if (st == RS_ILLNESS && sev != RV_ASYMPTOMATIC) {
            // (LDS rows and rows read through L2 apart: chosen per threshold, every one of the five LDS reads stood behind a wait
            // for the wave's vector memory -- the stream's fetch, issued a moment ago)
            nn = 0;
            if (in_lds) {
#pragma unroll
                for (int k = 0; k < REINA_COUNT_ILL; k++) nn += rc >= S_cthr[crow][REINA_COUNT_FULL + k] ? 1 : 0;
            } else {
#pragma unroll
                for (int k = 0; k < REINA_COUNT_ILL; k++) nn += rc >= LD_U32_NOW(T->cthr[crow][REINA_COUNT_FULL + k]) ? 1 : 0;
            }
        } else if (in_lds) {
            // (the guide entry, then the next two thresholds in one look -- they decide all but a draw in a thousand --, then
            // step by step)
            nn = S_cguide[crow][rc >> 24];
            const uint32_t c0 = S_cthr[crow][nn], c1 = S_cthr[crow][nn + 1];   // (nn + 1 <= 100: inside the row's 112 words)
            if (nn < REINA_COUNT_FULL && rc >= c0) {
                nn++;
                if (nn < REINA_COUNT_FULL && rc >= c1) {
                    nn++;
                    while (nn < REINA_COUNT_FULL && rc >= S_cthr[crow][nn]) nn++;
                }
            }
        } else {   // more distinct count rows than the LDS image holds: this one is read through L2
            nn = (int)LD_U8_NOW(T->cguide[crow][rc >> 24]);
            while (nn < REINA_COUNT_FULL && rc >= LD_U32_NOW(T->cthr[crow][nn])) nn++;
        }
        nr = (uint32_t)nn;
        float src_inf = inf;
        const uint4 vp = *reinterpret_cast<const uint4 *>(S.var_par[v]);
        if (sev == RV_ASYMPTOMATIC) src_inf *= rp_u2f(vp.x);
        // the largest transmission probability any target can give this source (did_infect with the most
        // susceptible age; the same expression, so it bounds every target's p from above bit for bit)
        const float p_max = src_inf * rp_u2f(vp.y) * rp_u2f(vp.z);
        // (bit 31: the source's infectee list exists iff it was infected while contact tracing was on: its START-
        // of-day word says so -- person_expose_others runs before the source's own transition, main.pyx:404-414)
        // (what a contact needs of its source in one 16-byte look.  it.y: the source's part of a pending record where the record
        // has it -- age [16:23) | variant [24:26) | keeps a list 31 -- and the entries of the age's contact row in [0:7), where the
        // record has the contact number; it.w: the thinning bound as the threshold of the 24-bit draw (rp_chance_threshold:
        // one comparison per contact) [0:25) | contact row of the age [25:32))
        const uint32_t row = S.row_of_age[age];
        it = make_uint4(i, (uint32_t)S.rcount[row] | ((uint32_t)age << 16) | ((uint32_t)v << 24) | ((w & RH_HASLIST) ? 0x80000000u : 0u),
                        rp_f2u(src_inf), rp_chance_threshold(p_max) | (row << 25));
    }
    // prefix sum of the counts across the wave: source `lane` owns the contacts [inc - nr, inc) of the batch
    const uint32_t inc = wave_scan_add(nr);
    S.pre[wave][lane] = inc - nr;
    S.item[wave][lane] = it;
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): wave-private LDS rows written
    __builtin_amdgcn_wave_barrier();
    C.wave_contacts += total;
    if (PROF_IS(BATCH_HEAD) || PROF_IS(HEAD_DRAINED)) PROF_IN_ADD(C, pb_, 1u);
    if (PROF_IS(BATCH_STEPS)) PROF_IN_MARK(pb_);
    // The owning source of contact j is the number of sources that lie wholly before it, E(j) = #{s : inc[s] <= j}.  Per step
    // of 64 contacts: every source whose contacts END inside the step's window marks the position (LDS counters, one add per
    // such source), a prefix sum over the window (six cross-lane moves) + the sources that ended before it = E.  (Rounds
    // 2-3 stamped every contact's owner into a byte map, one LDS store per CONTACT in a divergent loop as long as the largest
    // count of the batch, and read a byte of it per contact.  Measured together with the other changes of the batch -- DPP prefix
    // sums, thresholds and meta words in one look, per-variant parameters in LDS --: the peak day at 10^8 agents 327 -> 289 us,
    // LDS instructions 8.8 -> 7.5 x 10^6, scalar ones 7.7 -> 7.4 x 10^7: the scalar side of the kernel is its branches, spread
    // over every piece of it, not one loop.)
    uint32_t *S_cnt = S.own_cnt[wave];
    uint32_t ebase = 0;
#ifndef REINA_NO_DAY_PRIO
    __builtin_amdgcn_s_setprio(0);
#endif
    for (uint32_t j0 = 0; j0 < (ABLATED(CONTACTS) ? 0u : total); j0 += 64) {
        S_cnt[lane] = 0u;
        __builtin_amdgcn_wave_barrier();
        if (inc - j0 < 64u) atomicAdd(&S_cnt[inc - j0], 1u);
        __builtin_amdgcn_wave_barrier();
        const uint32_t owner_e = ebase + wave_scan_add(S_cnt[lane]);
        ebase = (uint32_t)__builtin_amdgcn_readlane((int)owner_e, 63);
        const uint32_t j = j0 + lane;
        bool poss = false;
        uint32_t pe = 0, pe_src = 0, pe_inf = 0;
        if (j < total) {
            const uint32_t owner = owner_e;
            const uint32_t c = j - S.pre[wave][owner];
            const uint4 own = S.item[wave][owner];
            const uint32_t row = own.w >> 25;
            const int cnt = (int)(own.y & 0x7Fu);
            // half 0 of the contact's draws: v[0] place / age range, v[2] transmission (Philox2x32: one multiply per
            // round; the other half is drawn only for the one contact in fifty that passes the thinning)
            const rp_u2 q0 = rp_philox2(C.ckey, own.x, rp_contact_ctr(dp.day, c, 0));
            rp_u4 r;
            r.v[0] = q0.v[0]; r.v[2] = q0.v[1];
            // daily_contacts[place] (main.pyx:1571): the place of the draw -- all that a contact which fails the thinning needs
            // of its table entry -- from the row's place groups: five comparisons against one 32-byte look (rounds 1-4 searched
            // the entry itself for every contact: guide byte, then two thresholds and three meta words, two dependent looks and a
            // nest of divergent branches; the entry is now found for the contacts that pass, in resolve_issue).  Counted per lane
            // in a 64-bit register, a 10-bit field per place, added to the LDS histogram every 1000 rounds at most.
            uint32_t sh;
            if (grouped) {
                const uint4 ga = *reinterpret_cast<const uint4 *>(&S.grp[row][0]);
                const uint2 gb = *reinterpret_cast<const uint2 *>(&S.grp[row][4]);
                const uint32_t g = (uint32_t)(r.v[0] >= ga.x) + (uint32_t)(r.v[0] >= ga.y) + (uint32_t)(r.v[0] >= ga.z) +
                                   (uint32_t)(r.v[0] >= ga.w) + (uint32_t)(r.v[0] >= gb.x);
                sh = ((gb.y >> (5u * g)) & 31u) * 2u;   // (10 x place, stored halved in five bits per group)
            } else {
                uint32_t l2_;
                sh = 10u * (contact_entry(T, S, S_thr, S_guide, lds_rows, uniform_meta, row, cnt, r.v[0], &l2_) & 0xFFu);
            }
            C.pl += 1ull << sh;
            poss = (r.v[2] >> 8) < (own.w & 0x1FFFFFFu);
            pe = c | (own.y & 0x837F0000u);   // (its table entry goes to bits [8:16) in resolve_issue)
            pe_src = own.x;
            pe_inf = own.z;
        }
        if (++C.pl_rounds == 1000u) {
            flush_places(S.daily, (uint32_t)C.pl & 0x3FFFFFFFu, (uint32_t)(C.pl >> 30) & 0x3FFFFFFFu);
            C.pl = 0ull;
            C.pl_rounds = 0;
        }
        const uint64_t pm = __ballot(poss);
        if (pm) {
            // the records go to the region being filled; when it is full (64) it is turned over -- requested, the one in flight
            // finished -- and the rest of this step's records start the other region
            const uint32_t cnt = (uint32_t)__popcll(pm), rank = (uint32_t)__popcll(pm & ((1ull << lane) - 1ull));
            const uint32_t room = 64u - C.n_pend;
            if (poss && rank < room) {
                const uint32_t q = C.cur * 64u + C.n_pend + rank;
                S.pend_src[wave][q] = pe_src;
                S.pend_info[wave][q] = pe;
                S.pend_inf[wave][q] = pe_inf;
            }
            if (cnt >= room) {
                C.n_pend = 64u;
                PROF_IN_VAR(pt_);
                if (PROF_IS(RESOLVE_TURNS)) PROF_IN_MARK(pt_);
#ifndef REINA_NO_DAY_PRIO
                __builtin_amdgcn_s_setprio(3);   // (the turn ends with the targets' gather going out: the sooner the better)
#endif
                resolve_turn(P, T, B, S, S_thr, S_guide, lds_rows, S_pressure, uniform_meta, dp, C);
#ifndef REINA_NO_DAY_PRIO
                __builtin_amdgcn_s_setprio(0);
#endif
                if (PROF_IS(RESOLVE_TURNS)) PROF_IN_ADD(C, pt_, 1u);
                if (poss && rank >= room) {
                    const uint32_t q = C.cur * 64u + rank - room;
                    S.pend_src[wave][q] = pe_src;
                    S.pend_info[wave][q] = pe;
                    S.pend_inf[wave][q] = pe_inf;
                }
                C.n_pend = cnt - room;
            } else {
                C.n_pend += cnt;
            }
        }
    }
    if (PROF_IS(BATCH_STEPS)) PROF_IN_ADD(C, pb_, (total + 63u) / 64u);
    __builtin_amdgcn_wave_barrier();
}

// (Measured dead end, round 2: carrying the day's OPENING in this launch -- the first workgroups to arrive taking the
// opening roles, the streaming workgroups holding their effects back until those had signalled -- was built, bit-exact,
// and slower at every size: HUS 28.5 us against 13 + 16.5, 10^8 agents 193 against 36 + 137, a 128-member group 685
// against 37 + 297.  The opening's chains of dependent round trips run two to three times longer beside the stream,
// and the streaming waves stall at the gate once their queues are full.)
// (SPARSE: the form of the stream, a property of the LAUNCH since round 5 -- one kernel that chose at run time carried the state of
// both forms through its loop, in scalar registers it did not have: the loop's own counters lived in spill lanes)
// (round 6: the body is a function of the workgroup's number `bx_` among the `nbx_` workgroups of the stream's phase and of its LDS
// block -- k_day below hands it blockIdx.x / gridDim.x and the launch's dynamic LDS, the fused day of a small population
// (k_small_day, reina_hip.hip) calls it between two launch-wide barriers.  FEED: how a wave finds its active agents -- FEED_DENSE /
// FEED_SPARSE: the two hand-scheduled forms described below, which own v104..v127; FEED_PLAIN: the bit plane and the words by
// ordinary loads, no register named by hand, for a population so small that the stream is a few lines per wave.)
enum { FEED_DENSE = 0, FEED_SPARSE = 1, FEED_PLAIN = 2 };
// `tables_staged`: the workgroup's LDS image of the tables is there already (a launch that runs several days: k_small_days) -- only the
// day's own words (place histogram, counts, the event stage) are reset.
template <bool EXACT, int FEED>
__device__ __forceinline__ void day_block(const MemberRef &mref_, const reina_day_t &dp, uint32_t lds_rows_launch, uint32_t lds_crows_launch,
                                          uint32_t day_flags, uint32_t import_wgs, uint32_t bx_, uint32_t nbx_, unsigned char *smem_raw,
                                          bool tables_staged = false) {
    const ParamsX<EXACT> P{(const CAS DevParams *)mref_.P};
    const GBuffers B = global_buffers(mref_.B);  // by value: pointers live in SGPRs, never re-read after stores
    const CAS Tables *T = (const CAS Tables *)mref_.T;
    DIAG_CLOCK(DAY, ds_t0);   // (-DREINA_DAY_STAMPS: where an (almost) empty day's k_day spends its time, thread 0 of every workgroup)
    // the LDS image is carved for lds_rows_launch rows (the same for every member of a group); this member fills
    // and uses min(its own distinct rows, that)
    const uint32_t lds_rows = T->n_rows < lds_rows_launch ? T->n_rows : lds_rows_launch;
    const uint32_t lds_crows = T->n_crows < lds_crows_launch ? T->n_crows : lds_crows_launch;
    const uint32_t uniform_meta = T->uniform_meta;
    // (the place groups serve when every row has them -- entries sorted by place, as the reference's are -- and every row is in LDS)
    const bool grouped = T->grouped != 0u && T->n_rows <= lds_rows_launch && T->n_rows <= REINA_LDS_ROWS;
    DayShared &S = *reinterpret_cast<DayShared *>(smem_raw);
    uint32_t (*S_thr)[REINA_MAX_ENTRIES] = reinterpret_cast<uint32_t (*)[REINA_MAX_ENTRIES]>(smem_raw + sizeof(DayShared));
    uint8_t (*S_guide)[256] = reinterpret_cast<uint8_t (*)[256]>(smem_raw + sizeof(DayShared) + (size_t)lds_rows_launch * REINA_MAX_ENTRIES * 4);
    unsigned char *smem_c = smem_raw + sizeof(DayShared) + (size_t)lds_rows_launch * DAY_ROW_BYTES;
    uint32_t (*S_cthr)[REINA_COUNT_WORDS] = reinterpret_cast<uint32_t (*)[REINA_COUNT_WORDS]>(smem_c);
    uint8_t (*S_cguide)[256] = reinterpret_cast<uint8_t (*)[256]>(smem_c + (size_t)lds_crows_launch * REINA_COUNT_WORDS * 4);
    int32_t *S_pressure = reinterpret_cast<int32_t *>(smem_c + (size_t)lds_crows_launch * DAY_CROW_BYTES);
    // (the wave number through readfirstlane: everything derived from it -- tile indices, queue bases, loop conditions --
    // is then provably wave-uniform and lives in scalar registers, branches on it are scalar branches)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t N = P->n_agents;
    const uint32_t n4 = N >> 2;
    const GAS uint4 *hot4 = reinterpret_cast<const GAS uint4 *>(B.hot);
    // each wave walks tiles of 128 uint4 (two 1-KiB loads in flight per wave)
    const uint32_t tiles = (n4 + 127u) / 128u;
    // the launch's last `import_wgs` workgroups place the day's weekly imports beside the stream (k_open.inc: deferred
    // placement); nothing the streaming workgroups do waits for them
    const uint32_t stream_blocks = nbx_ - import_wgs;
    if (bx_ >= stream_blocks) {
        day_imports_block(mref_, dp, smem_raw, bx_ - stream_blocks, import_wgs);
        return;
    }
    const uint32_t wave_global = bx_ * DAY_WAVES + wave, waves_total = stream_blocks * DAY_WAVES;
    // THREE register sets hold the three tiles a wave has in flight (six 1-KiB loads); they are used in turn, and each
    // is reloaded -- three tiles ahead -- as soon as its words have been looked at.  The sets are the registers
    // v104..v127, which the compiler never sees: the kernel is compiled for 104 VGPRs (amdgpu_num_vgpr) and the loads,
    // the counted wait and the extraction of the eight RH_ACTIVE bits are inline assembly naming those registers.
    // (Left to the compiler, every tile waited for the loads it had just issued -- s_waitcnt vmcnt(0) and register
    // copies at each loop-carried merge -- i.e. one tile in flight per wave and a latency-bound stream; handing it
    // asynchronously loaded values as ordinary variables is not safe either: it copies them while they are in flight.)
    // Loads are unconditional: addresses past the end are clamped to the last 16-byte group (the lanes concerned are
    // masked out when the tile is looked at).  The first loads go out before anything else: the table staging runs
    // behind them.
    const uint32_t n4m1 = n4 ? n4 - 1u : 0u;
#define DAY_STR_(x) #x
#define DAY_STR(x) DAY_STR_(x)
#define DAY_ISSUE_REGS(tile, R0, R3, R4, R7)                                                            \
    do {                                                                                                \
        const uint32_t p0_ = (tile) * 128u + lane, p1_ = p0_ + 64u;                                     \
        const GAS uint4 *g0_ = hot4 + (p0_ < n4m1 ? p0_ : n4m1), *g1_ = hot4 + (p1_ < n4m1 ? p1_ : n4m1); \
        asm volatile("global_load_dwordx4 v[" DAY_STR(R0) ":" DAY_STR(R3) "], %0, off\n\t"              \
                     "global_load_dwordx4 v[" DAY_STR(R4) ":" DAY_STR(R7) "], %1, off"                    \
                     : : "v"(g0_), "v"(g1_) : "memory");                                                \
    } while (0)
    // vector-memory operations complete in issue order: a set's two loads have landed once at most the four younger
    // ones (the other two sets') are outstanding; then bit 15 of its eight words -> bits 0..7 of the mask
#define DAY_MASK_REGS(m_, R0, R1, R2, R3, R4, R5, R6, R7)                                               \
    do {                                                                                                \
        uint32_t t_;                                                                                    \
        asm volatile("s_waitcnt vmcnt(4)\n\t"                                                           \
                     "v_bfe_u32 %0, v" DAY_STR(R0) ", 15, 1\n\t"                                        \
                     "v_bfe_u32 %1, v" DAY_STR(R1) ", 15, 1\n\tv_lshl_or_b32 %0, %1, 1, %0\n\t"         \
                     "v_bfe_u32 %1, v" DAY_STR(R2) ", 15, 1\n\tv_lshl_or_b32 %0, %1, 2, %0\n\t"         \
                     "v_bfe_u32 %1, v" DAY_STR(R3) ", 15, 1\n\tv_lshl_or_b32 %0, %1, 3, %0\n\t"         \
                     "v_bfe_u32 %1, v" DAY_STR(R4) ", 15, 1\n\tv_lshl_or_b32 %0, %1, 4, %0\n\t"         \
                     "v_bfe_u32 %1, v" DAY_STR(R5) ", 15, 1\n\tv_lshl_or_b32 %0, %1, 5, %0\n\t"         \
                     "v_bfe_u32 %1, v" DAY_STR(R6) ", 15, 1\n\tv_lshl_or_b32 %0, %1, 6, %0\n\t"         \
                     "v_bfe_u32 %1, v" DAY_STR(R7) ", 15, 1\n\tv_lshl_or_b32 %0, %1, 7, %0"              \
                     : "=&v"(m_), "=&v"(t_) : : "memory");                                              \
    } while (0)
#define DAY_ISSUE(set, tile)                                                     \
    do {                                                                         \
        if ((set) == 0u) DAY_ISSUE_REGS(tile, 104, 107, 108, 111);               \
        else if ((set) == 1u) DAY_ISSUE_REGS(tile, 112, 115, 116, 119);          \
        else DAY_ISSUE_REGS(tile, 120, 123, 124, 127);                           \
    } while (0)
#define DAY_MASK(m_, set)                                                                    \
    do {                                                                                     \
        if ((set) == 0u) DAY_MASK_REGS(m_, 104, 105, 106, 107, 108, 109, 110, 111);          \
        else if ((set) == 1u) DAY_MASK_REGS(m_, 112, 113, 114, 115, 116, 117, 118, 119);     \
        else DAY_MASK_REGS(m_, 120, 121, 122, 123, 124, 125, 126, 127);                      \
    } while (0)
    // (the clobbers that tell the compiler these registers are written: it must count them into the kernel's allocation)
    if (FEED != FEED_PLAIN)
        asm volatile("" : : : "v104", "v105", "v106", "v107", "v108", "v109", "v110", "v111", "v112", "v113", "v114", "v115",
                     "v116", "v117", "v118", "v119", "v120", "v121", "v122", "v123", "v124", "v125", "v126", "v127");
    // SPARSE DAYS (round 4).  Context._iterate_people looks at every person and leaves all but the infected at once
    // (main.pyx:1974-1975).  The same test here is the ACTIVE flag of the hot word -- and one bit per agent in
    // buffers.active_bits, kept beside it by install_infection and by the counting step (k_scan.inc).  When yesterday's
    // stream found fewer than `sparse_below` active agents, today's does not stream the hot words (4 N bytes) at all: a wave
    // reads the 64 bytes of bits of each of ITS tiles (same tiles, same per-wave slices as on a dense day, so nothing
    // downstream knows the difference), queues the agents whose bit is set and fetches only their words.  At 10^8 agents
    // that is 12.5 MB + one sector per active agent instead of 400 MB on the two days in three on which fewer than one agent
    // in a hundred is infected.  Both forms give the same queue contents, hence bit-identical results (tests/test_parity_gpu.py
    // runs every scenario family in both).
    // The wave's bit words land in the same hand-reserved registers, as FIVE sets of four (one set = 16 tiles: lane l holds the
    // four words of quarter l & 3 of the wave's tile 16 c + (l >> 2) of chunk c); all five are requested before the tables
    // are staged, a set is requested again five chunks ahead when it has been taken.  v124 receives the hot words of the
    // agents being fetched (below).
    const uint32_t my_tiles = wave_global < tiles ? (tiles - 1u - wave_global) / waves_total + 1u : 0u;
    // (a wave with few tiles has few lanes holding bits -- one tile is four lanes' worth -- and queues few agents per step:
    // the sparse form pays from a handful of tiles per wave on; a HUS-sized population on a whole chip has one)
    constexpr bool sparse = FEED == FEED_SPARSE, plain = FEED == FEED_PLAIN;
    const uint32_t sp_chunks = (my_tiles + 15u) >> 4;
    const GAS uint4 *bits4 = reinterpret_cast<const GAS uint4 *>(B.active_bits);
#define SP_SETS 5u
#define SP_ISSUE_REGS(chunk, R0, R3)                                                                         \
    do {                                                                                                     \
        const uint32_t tl_ = (chunk) * 16u + ((uint32_t)lane >> 2);                                         \
        const GAS uint4 *g_ = bits4 + (tl_ < my_tiles ? (wave_global + tl_ * waves_total) * 4u + ((uint32_t)lane & 3u) : 0u); \
        asm volatile("global_load_dwordx4 v[" DAY_STR(R0) ":" DAY_STR(R3) "], %0, off" : : "v"(g_) : "memory"); \
    } while (0)
#define SP_ISSUE(set, chunk)                                         \
    do {                                                             \
        if ((set) == 0u) SP_ISSUE_REGS(chunk, 104, 107);             \
        else if ((set) == 1u) SP_ISSUE_REGS(chunk, 108, 111);        \
        else if ((set) == 2u) SP_ISSUE_REGS(chunk, 112, 115);        \
        else if ((set) == 3u) SP_ISSUE_REGS(chunk, 116, 119);        \
        else SP_ISSUE_REGS(chunk, 120, 123);                         \
    } while (0)
#define SP_TAKE_REGS(b_, R0, R1, R2, R3)                                                                     \
    asm volatile("s_waitcnt vmcnt(0)\n\tv_mov_b32 %0, v" DAY_STR(R0) "\n\tv_mov_b32 %1, v" DAY_STR(R1)       \
                 "\n\tv_mov_b32 %2, v" DAY_STR(R2) "\n\tv_mov_b32 %3, v" DAY_STR(R3)                         \
                 : "=&v"(b_.x), "=&v"(b_.y), "=&v"(b_.z), "=&v"(b_.w) : : "memory")
#define SP_TAKE(b_, set)                                                 \
    do {                                                                 \
        if ((set) == 0u) SP_TAKE_REGS(b_, 104, 105, 106, 107);           \
        else if ((set) == 1u) SP_TAKE_REGS(b_, 108, 109, 110, 111);      \
        else if ((set) == 2u) SP_TAKE_REGS(b_, 112, 113, 114, 115);      \
        else if ((set) == 3u) SP_TAKE_REGS(b_, 116, 117, 118, 119);      \
        else SP_TAKE_REGS(b_, 120, 121, 122, 123);                       \
    } while (0)
    // a dense day's word k (0..7) of register set `set`: the tile's words stay in their registers until every slot has been
    // queued, and go to the queue WITH the agent's number (round 4; rounds 1-3 queued the number and read the word again, from
    // L2, when its turn came: a round trip at the head of every state-machine round)
#define DAY_WORD_REG(w_, R) asm volatile("v_mov_b32 %0, v" DAY_STR(R) : "=v"(w_) : : "memory")
#define DAY_WORD(w_, set, k)                                                                                     \
    do {                                                                                                         \
        switch ((set) * 8u + (k)) {                                                                              \
        case 0: DAY_WORD_REG(w_, 104); break; case 1: DAY_WORD_REG(w_, 105); break; case 2: DAY_WORD_REG(w_, 106); break;   \
        case 3: DAY_WORD_REG(w_, 107); break; case 4: DAY_WORD_REG(w_, 108); break; case 5: DAY_WORD_REG(w_, 109); break;   \
        case 6: DAY_WORD_REG(w_, 110); break; case 7: DAY_WORD_REG(w_, 111); break; case 8: DAY_WORD_REG(w_, 112); break;   \
        case 9: DAY_WORD_REG(w_, 113); break; case 10: DAY_WORD_REG(w_, 114); break; case 11: DAY_WORD_REG(w_, 115); break; \
        case 12: DAY_WORD_REG(w_, 116); break; case 13: DAY_WORD_REG(w_, 117); break; case 14: DAY_WORD_REG(w_, 118); break; \
        case 15: DAY_WORD_REG(w_, 119); break; case 16: DAY_WORD_REG(w_, 120); break; case 17: DAY_WORD_REG(w_, 121); break; \
        case 18: DAY_WORD_REG(w_, 122); break; case 19: DAY_WORD_REG(w_, 123); break; case 20: DAY_WORD_REG(w_, 124); break; \
        case 21: DAY_WORD_REG(w_, 125); break; case 22: DAY_WORD_REG(w_, 126); break; default: DAY_WORD_REG(w_, 127); break; \
        }                                                                                                        \
    } while (0)
    if (plain) {
    } else if (sparse) {
#pragma unroll
        for (uint32_t c = 0; c < SP_SETS; c++)
            if (c < sp_chunks) SP_ISSUE(c, c);
    } else {
        DAY_ISSUE_REGS(wave_global, 104, 107, 108, 111);
        DAY_ISSUE_REGS(wave_global + waves_total, 112, 115, 116, 119);
        DAY_ISSUE_REGS(wave_global + 2u * waves_total, 120, 123, 124, 127);
    }
    if (tables_staged) {
        const uint32_t t = (uint32_t)tid;
        if (t < REINA_NR_PLACES) S.daily[t] = 0;
        if (t == 0) { S.n_contacts = S.n_active = S.n_hosp = S.n_icu = 0; S.ev_n = 0u; }
    } else {
        // The tables' staging: every thread REQUESTS all its pieces first (a dozen independent loads), waits once, and then
        // stores them to LDS.  (Written as one copy loop per table, each loop's load was waited for before the next one
        // went out: eight L2 round trips in a row, 4-6 us of every k_day launch.)
        static_assert(REINA_LDS_ROWS * REINA_MAX_ENTRIES * 4 / 16 <= DAY_THREADS && REINA_LDS_CROWS * REINA_COUNT_WORDS * 4 / 16 <= DAY_THREADS &&
                      REINA_MAX_AGES * 8 <= DAY_THREADS && REINA_MAX_VARIANTS * REINA_MAX_AGES <= DAY_THREADS && REINA_AGE_BLOCKS / 4 <= DAY_THREADS && REINA_LDS_ROWS * 8 <= DAY_THREADS,
                      "one element per thread in every staging copy");
        const uint32_t n_thr = lds_rows * REINA_MAX_ENTRIES * 4 / 16, n_gd = lds_rows * 256 / 16;
        const uint32_t n_cthr = lds_crows * REINA_COUNT_WORDS * 4 / 16, n_cgd = lds_crows * 256 / 16;
        const uint32_t t = (uint32_t)tid;
        uint4 v_thr = make_uint4(0, 0, 0, 0), v_gd = v_thr, v_cthr = v_thr, v_cgd = v_thr;
        uint32_t v_meta = 0, v_ab = 0, v_as = 0, v_rc = 0, v_roa = 0, v_croa = 0;
        float v_mask = 0.0f, v_psus = 0.0f, v_iot = 0.0f;
        const GAS Tables *Tg = (const GAS Tables *)mref_.T;   // (the staging copy reads whole rows per thread: global loads)
        if (t < n_thr) v_thr = gld(&reinterpret_cast<const GAS uint4 *>(&Tg->thr[0][0])[t]);
        if (t < n_gd) v_gd = gld(&reinterpret_cast<const GAS uint4 *>(&Tg->guide[0][0])[t]);
        if (t < n_cthr) v_cthr = gld(&reinterpret_cast<const GAS uint4 *>(&Tg->cthr[0][0])[t]);
        if (t < n_cgd) v_cgd = gld(&reinterpret_cast<const GAS uint4 *>(&Tg->cguide[0][0])[t]);
        if (t < REINA_MAX_ENTRIES) v_meta = T->meta[0][t];
        uint32_t v_grp = 0;
        if (t < lds_rows * 8u) v_grp = (&T->grp[0][0])[t];
        if (t < REINA_MAX_AGES * 8) v_mask = (&P->mask_p[0][0])[t];
        if (t < REINA_MAX_VARIANTS * REINA_MAX_AGES) v_psus = (&P->dis.p_susceptibility[0][0])[t];
        if (t <= REINA_MAX_AGES) v_as = (uint32_t)P->age_start[t];
        if (t < REINA_MAX_AGES) {
            v_rc = (uint32_t)T->rcount[t];
            v_roa = T->row_of_age[t];
            v_croa = T->crow_of_age[t];
        }
        if (t < REINA_AGE_BLOCKS / 4) v_ab = reinterpret_cast<const GAS uint32_t *>(Tg->age_block)[t];
        if (t < REINA_MAX_VARIANTS * (REINA_IOT_LEN + 3)) v_iot = (&P->dis.infectiousness_over_time[0][0])[t];
        const uint32_t sharded = P->n_shards > 1 ? 1u : 0u;
        if (t < n_thr) reinterpret_cast<uint4 *>(&S_thr[0][0])[t] = v_thr;
        if (t < n_gd) reinterpret_cast<uint4 *>(&S_guide[0][0])[t] = v_gd;
        if (t < n_cthr) reinterpret_cast<uint4 *>(&S_cthr[0][0])[t] = v_cthr;
        if (t < n_cgd) reinterpret_cast<uint4 *>(&S_cguide[0][0])[t] = v_cgd;
        if (t < REINA_MAX_ENTRIES) S.meta_row[t] = v_meta;
        if (t < lds_rows * 8u) (&S.grp[0][0])[t] = v_grp;
        if (t < REINA_MAX_AGES * 8) (&S.mask_p[0][0])[t] = v_mask;
        if (t < REINA_MAX_VARIANTS * REINA_MAX_AGES) (&S.p_sus[0][0])[t] = v_psus;
        if (t <= REINA_MAX_AGES) S.age_start[t] = (int32_t)v_as;
        if (t < REINA_MAX_AGES) {
            S.rcount[t] = (int32_t)v_rc;
            S.row_of_age[t] = (uint8_t)v_roa;
            S.crow_of_age[t] = (uint8_t)v_croa;
        }
        if (t < REINA_AGE_BLOCKS / 4) reinterpret_cast<uint32_t *>(S.age_block)[t] = v_ab;
        if (t < REINA_MAX_VARIANTS * (REINA_IOT_LEN + 3)) (&S.iot[0][0])[t] = v_iot;
        if (t < REINA_MAX_VARIANTS) {
            S.var_par[t][0] = rp_f2u(P->dis.p_asymptomatic_infection[t]);
            S.var_par[t][1] = rp_f2u(P->psus_max[t]);
            S.var_par[t][2] = rp_f2u(P->dis.infectiousness_multiplier[t]);
            S.var_par[t][3] = P->iot_mask[t];
        }
        if (t < REINA_NR_PLACES) S.daily[t] = 0;
        if (t == 0) { S.n_contacts = S.n_active = S.n_hosp = S.n_icu = 0; S.ev_n = 0u; }
        if (sharded)
            for (int k = tid; k < REINA_PRESSURE_WORDS; k += DAY_THREADS) S_pressure[k] = 0;
    }
    __syncthreads();
    DIAG_SINCE(DAY, DIAG_DAY_STAGED, DIAG_THREAD0, ds_t0, B.mirror);
    ScanLists L;
    ContactState C;
    {
        const uint32_t cap = P->max_work_items, base = scan_slice_base(wave_global, waves_total, tiles);
        L.l[LIST_EXP] = nullptr;
        L.l[LIST_ILL] = reinterpret_cast<GAS uint2 *>(B.work_items) + cap + base;
        L.l[LIST_EV] = nullptr;   // (events go to the day's priority buckets)
        L.l[LIST_BOOK] = reinterpret_cast<GAS uint2 *>(B.scan_lists) + cap + base;
        L.n[0] = L.n[1] = L.n[2] = L.n[3] = 0;
        L.strip = S.strip[wave];
        L.qn = 0;
        L.n_hosp = L.n_icu = 0;
        C.n_cand = 0;
        C.slice_base = base;
        C.slice_cap = (wave_global + 1 < waves_total ? scan_slice_base(wave_global + 1, waves_total, tiles) : cap) - base;
        C.wave_contacts = 0;
        C.pl = 0ull;
        C.pl_rounds = 0;
        C.n_pend = C.cur = C.fl = 0;
        C.fl_t = 0;
        C.ckey = opaque_s(rp_contact_key(P->k0, P->k1));
        C.n_shards = opaque_s(P->n_shards);
        C.shard_rank = opaque_s(P->shard_rank);
        C.age_shift = opaque_s(T->age_shift);
        C.nr_ages = opaque_s((uint32_t)P->nr_ages);
        PROF_IN_RESET(C);
    }
    // The wave's LDS queues: nq = (agent, hot word) pairs awaiting the state machine, filled from the tiles (dense day:
    // the words are in the tile's registers) or from the fetches (sparse day); xq (L.strip) = infectious agents found by
    // the state machine, awaiting their contacts.  Both are worked off 64 entries at a time, from the back, so every lane
    // is busy whatever the prevalence.  Nothing in a state-machine round waits for memory any more: the word comes with
    // the queue entry, bed / ICU events go to the workgroup's stage in LDS (below), the lists are plain stores.
    uint2 *nq = S.needy[wave];
    uint32_t *iq = S.idxq[wave];
    uint32_t nqn = 0, iqn = 0;
    uint32_t n_act = 0;              // agents this wave queued (wave-uniform)
    uint32_t tcur = wave_global;     // dense: tile whose words sit in register set `cur`
    uint32_t cur = 0;
    uint32_t tmask = 0, kslot = 0;   // dense: the open tile's need bits not yet queued, the next word slot
    bool open = false;               // dense: a tile is open (its register set not yet requested again)
    uint64_t b_lo = 0, b_hi = 0;         // sparse: this lane's bits of chunk sp_k - 1 that have not been queued yet (agents 0-63, 64-127 of its 128)
    uint32_t b_base = 0;                 // ... and the agent its bit 0 stands for
    uint32_t sp_k = 0;                   // ... and the next chunk to take
    uint32_t fl_i = 0, fl_n = 0;         // sparse: the agents whose words are in flight (v124), and how many
#define DAY_PUSH(need_, i_, w_)                                                                        \
    do {                                                                                               \
        const uint64_t m_ = __ballot(need_);                                                           \
        if (m_) {                                                                                      \
            if (need_) nq[nqn + (uint32_t)__popcll(m_ & ((1ull << lane) - 1ull))] = make_uint2((i_), (w_)); \
            nqn += (uint32_t)__popcll(m_);                                                             \
            n_act += (uint32_t)__popcll(m_);                                                           \
        }                                                                                              \
    } while (0)
    if (wave_global == 0) {   // ragged tail: N not a multiple of 4 (first: the queue is empty now, and holds only 128 pairs)
        const uint32_t i = (n4 << 2) + lane;
        const bool in = lane < (int)(N & 3u);
        const uint32_t w = in ? (uint32_t)B.hot[i] : 0u;
        DAY_PUSH(in && (w & RH_ACTIVE), i, w);
    }
    PROF_DECL;
    PROF_BEGIN(LOOP);
    // Wave priorities by PHASE (round 5): the feed and the state-machine rounds are chains of dependent steps with few vector
    // instructions between them, a contact batch is vector instructions back to back.  The SIMD issues its oldest wave first;
    // with the chains above the batches, a wave in its feed gets its few instructions out between the multiplies of the others'
    // contact steps instead of behind them.
    for (;;) {
        bool more;
#ifndef REINA_NO_DAY_PRIO
        __builtin_amdgcn_s_setprio(3);
#endif
        PROF_BEGIN(FEED);
        if (plain) {
            // The fused day of a small population (k_small_day): a wave's tiles are a handful, the launch has a few dozen
            // workgroups -- the bits of sixteen tiles by one ordinary 16-byte load per lane, the set bits to agent numbers exactly as
            // on a sparse day, the words of (up to) 64 agents by one ordinary gather, waited for at once.
            bool have = (b_lo | b_hi) != 0ull;
            while (nqn < 64u) {
                while (iqn < 64u) {
                    while (!__any(have) && sp_k < sp_chunks) {
                        const uint32_t tl = sp_k * 16u + ((uint32_t)lane >> 2);
                        uint4 bw = make_uint4(0, 0, 0, 0);
                        if (tl < my_tiles) bw = gld(&bits4[(wave_global + tl * waves_total) * 4u + ((uint32_t)lane & 3u)]);
                        b_lo = (uint64_t)bw.x | ((uint64_t)bw.y << 32);
                        b_hi = (uint64_t)bw.z | ((uint64_t)bw.w << 32);
                        b_base = (wave_global + tl * waves_total) * 512u + ((uint32_t)lane & 3u) * 128u;
                        sp_k++;
                        have = (b_lo | b_hi) != 0ull;
                    }
                    if (!__any(have)) break;
                    const bool up = b_lo == 0ull;
                    const uint64_t word = up ? b_hi : b_lo;
                    const uint32_t w_lo = (uint32_t)word, w_hi = (uint32_t)(word >> 32);
                    const uint32_t pos = w_lo ? (uint32_t)__builtin_ctz(w_lo) : 32u + (uint32_t)__builtin_ctz(w_hi | 0x80000000u);
                    const uint64_t rest = word & (word - 1ull);
                    b_lo = up ? b_lo : rest;
                    b_hi = up ? rest : b_hi;
                    const uint32_t idx = b_base + (up ? 64u : 0u) + pos;
                    const bool q = have && idx < (n4 << 2);   // (agents past the last whole group of four: the ragged tail above)
                    const uint64_t m = __ballot(q);
                    if (q) iq[iqn + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = idx;
                    iqn += (uint32_t)__popcll(m);
                    have = (b_lo | b_hi) != 0ull;
                }
                if (iqn == 0u) break;
                const uint32_t n = iqn < 64u ? iqn : 64u;
                iqn -= n;
                __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave-private queue is written
                __builtin_amdgcn_wave_barrier();
                const bool in = (uint32_t)lane < n;
                const uint32_t idx = in ? iq[iqn + lane] : 0u;
                const uint32_t w = in ? (uint32_t)B.hot[idx] : 0u;
                // (the word's own ACTIVE flag is asked again, as on a sparse day: the bit plane is a caller-visible buffer)
                DAY_PUSH(in && (w & RH_ACTIVE) != 0u, idx, w);
            }
            more = __any(have) || sp_k < sp_chunks || iqn > 0u;
        } else if (sparse) {
            // A sparse day in three small stages, so that a wave has one fetch in flight while it works:
            //   (1) the words requested one pass ago have arrived: (agent, word) -> nq;
            //   (2) bits -> agent numbers (iq): every lane that has a bit left queues the agent of its lowest one, at most 64
            //       a step; a chunk that is used up is replaced from its register set, which is requested again five ahead;
            //   (3) the next (up to) 64 agents of iq: their hot words requested into v124.
            PROF_BEGIN(SPARSE_WORDS);
            if (fl_n && nqn < 64u) {
                uint32_t w;
                PROF_BEGIN(FETCH_WAIT);
                asm volatile("s_waitcnt vmcnt(0)\n\tv_mov_b32 %0, v124" : "=v"(w) : : "memory");
                PROF_END(FETCH_WAIT);
                // (the word's own ACTIVE flag is asked again: the bit plane is a caller-visible buffer, and a word that does not agree
                // with its bit must not reach the state machine -- round-4 advisor)
                DAY_PUSH((uint32_t)lane < fl_n && (w & RH_ACTIVE) != 0u, fl_i, w);
                fl_n = 0;
                // (everything this wave has requested is there: the bits of the contacts in flight too)
                if (C.fl) resolve_finish(P, T, B, S, S_pressure, uniform_meta, dp, (C.cur ^ 1u) * 64u, C);
            }
            PROF_END(SPARSE_WORDS);
            PROF_BEGIN(SPARSE_BITS);
            // (the lane's 128 bits as two 64-bit halves, the lowest set bit of the lower non-empty half taken each step: straight-line
            // code -- as four words with a four-way choice of the word to take from and to write back, the compiler's version of
            // this loop was 75 instructions under three nested exec masks, a fifth of the wave's peak-day cycles)
            bool have = (b_lo | b_hi) != 0ull;
            while (iqn < 64u) {
                while (!__any(have) && sp_k < sp_chunks) {
                    const uint32_t set = sp_k % SP_SETS;
                    uint4 bw;
                    PROF_BEGIN(BITS_WAIT);
                    SP_TAKE(bw, set);
                    PROF_END(BITS_WAIT);
                    if (sp_k * 16u + ((uint32_t)lane >> 2) >= my_tiles) bw = make_uint4(0, 0, 0, 0);   // (a lane past the wave's last tile loaded word 0)
                    if (sp_k + SP_SETS < sp_chunks) SP_ISSUE(set, sp_k + SP_SETS);
                    b_lo = (uint64_t)bw.x | ((uint64_t)bw.y << 32);
                    b_hi = (uint64_t)bw.z | ((uint64_t)bw.w << 32);
                    // first agent of the lane's 128 bits: tile wave_global + (16 sp_k + lane / 4) x waves_total, quarter lane % 4
                    b_base = (wave_global + (sp_k * 16u + ((uint32_t)lane >> 2)) * waves_total) * 512u + ((uint32_t)lane & 3u) * 128u;
                    sp_k++;
                    have = (b_lo | b_hi) != 0ull;
                }
                if (!__any(have)) break;
                PROF_TALLY(BIT_LANES, 1u, (uint32_t)__popcll(__ballot(have)));
                const bool up = b_lo == 0ull;
                const uint64_t word = up ? b_hi : b_lo;
                const uint32_t w_lo = (uint32_t)word, w_hi = (uint32_t)(word >> 32);
                const uint32_t pos = w_lo ? (uint32_t)__builtin_ctz(w_lo) : 32u + (uint32_t)__builtin_ctz(w_hi | 0x80000000u);
                const uint64_t rest = word & (word - 1ull);
                b_lo = up ? b_lo : rest;
                b_hi = up ? rest : b_hi;
                const uint32_t idx = b_base + (up ? 64u : 0u) + pos;
                // (agents past the last whole group of four belong to the ragged tail below, as on a dense day)
                const bool q = have && idx < (n4 << 2);
                const uint64_t m = __ballot(q);
                if (q) iq[iqn + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = idx;
                iqn += (uint32_t)__popcll(m);
                have = (b_lo | b_hi) != 0ull;
            }
            PROF_END(SPARSE_BITS);
            PROF_BEGIN(SPARSE_FETCH);
            const bool bits_left = __any(have) || sp_k < sp_chunks;
            if (!fl_n && iqn >= (bits_left ? 64u : 1u)) {
                fl_n = iqn < 64u ? iqn : 64u;
                iqn -= fl_n;
                __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave-private queue is written
                __builtin_amdgcn_wave_barrier();
                if ((uint32_t)lane < fl_n) {
                    fl_i = iq[iqn + lane];
                    asm volatile("global_load_dword v124, %0, off" : : "v"(B.hot + fl_i) : "memory");
                }
            }
            more = bits_left || iqn > 0u || fl_n > 0u;
            PROF_END(SPARSE_FETCH);
        } else {
            // A dense day: the tile's words are in register set `cur`; its need bits are queued word slot by word slot (at
            // most 64 agents a step) until a state-machine round is due, then the set is requested again, three tiles ahead.
            while (nqn < 64u) {
                if (!open) {
                    if (tcur >= tiles) break;
                    DAY_MASK(tmask, cur);
                    const uint32_t q0_ = tcur * 128u + lane;
                    if (tcur + 1u >= tiles) {   // the last tile: lanes past the end hold clamped loads
                        if (q0_ >= n4) tmask &= ~0x0Fu;
                        if (q0_ + 64u >= n4) tmask &= ~0xF0u;
                    }
                    open = true;
                    kslot = 8u;
                    if (__any(tmask != 0u)) {
                        // the usual case: the whole tile fits the queue (always, below one agent in four active): its eight
                        // word slots are queued in one go, straight-line code naming the set's registers; otherwise slot by
                        // slot below, a state-machine round in between whenever 64 are queued
                        uint64_t mk[8];
                        uint32_t total = 0;
#pragma unroll
                        for (uint32_t k = 0; k < 8u; k++) {
                            mk[k] = __ballot(((tmask >> k) & 1u) != 0u);
                            total += (uint32_t)__popcll(mk[k]);
                        }
                        if (nqn + total <= NEEDY_ENTRIES) {
                            const uint32_t base0 = 4u * (tcur * 128u + lane);
#define DAY_PUSH_K(k, R)                                                                                          \
    if (mk[k]) {                                                                                                  \
        uint32_t w_;                                                                                              \
        DAY_WORD_REG(w_, R);                                                                                      \
        if ((tmask >> (k)) & 1u) nq[nqn + (uint32_t)__popcll(mk[k] & ((1ull << lane) - 1ull))] = make_uint2(base0 + ((k) < 4 ? (k) : 252u + (k)), w_); \
        nqn += (uint32_t)__popcll(mk[k]);                                                                         \
    }
#define DAY_PUSH_SET(R0, R1, R2, R3, R4, R5, R6, R7) \
    DAY_PUSH_K(0, R0) DAY_PUSH_K(1, R1) DAY_PUSH_K(2, R2) DAY_PUSH_K(3, R3) DAY_PUSH_K(4, R4) DAY_PUSH_K(5, R5) DAY_PUSH_K(6, R6) DAY_PUSH_K(7, R7)
                            if (cur == 0u) { DAY_PUSH_SET(104, 105, 106, 107, 108, 109, 110, 111) }
                            else if (cur == 1u) { DAY_PUSH_SET(112, 113, 114, 115, 116, 117, 118, 119) }
                            else { DAY_PUSH_SET(120, 121, 122, 123, 124, 125, 126, 127) }
#undef DAY_PUSH_SET
#undef DAY_PUSH_K
                            n_act += total;
                        } else {
                            kslot = 0u;
                        }
                    }
                }
                while (kslot < 8u) {
                    const uint32_t k = kslot++;
                    const bool need = ((tmask >> k) & 1u) != 0u;
                    if (__any(need)) {
                        uint32_t w;
                        DAY_WORD(w, cur, k);
                        DAY_PUSH(need, 4u * (tcur * 128u + lane) + (k < 4u ? k : 252u + k), w);
                        break;
                    }
                }
                if (kslot >= 8u) {
                    // the set's words are dead: it is reloaded three tiles ahead at once
                    DAY_ISSUE(cur, tcur + 3u * waves_total);
                    cur = cur == 2u ? 0u : cur + 1u;
                    tcur += waves_total;
                    open = false;
                }
            }
            more = open || tcur < tiles;
            // (Measured dead end, round 3: every wave has the same number of tiles, yet the first wave of a workgroup is through
            // with them 14 us before the last one on a quiet day at 10^8 agents -- the SIMD issues its oldest wave first.  Wave
            // priorities by progress (s_setprio: behind the workgroup's front -> 3, leading -> 0) brought that to 6 us and the
            // workgroup's finish from 72.9 to 70.9 us; the launch did not get shorter, the peak day got 5 % longer.  The tail of
            // the stream is not where the bandwidth is lost.)
        }
        PROF_END(FEED);
#ifndef REINA_NO_DAY_PRIO
        __builtin_amdgcn_s_setprio(2);
#endif
        // the heavy part (every piece of it exists once): state-machine rounds while 64 needy agents are queued,
        // contact batches while 64 infectious ones are; when the tiles are finished, until both queues are empty
        for (;;) {
            // (the contact queue first: a state-machine round adds up to 64 infectious agents to the fewer than 64 left)
            if (L.qn >= ((more || nqn > 0u) ? 64u : 1u)) {
                const uint32_t n = L.qn < 64u ? L.qn : 64u;
                L.qn -= n;
                __builtin_amdgcn_s_waitcnt(0xc07f);
                __builtin_amdgcn_wave_barrier();
                PROF_BEGIN(BATCHES);
#ifndef REINA_NO_DAY_PRIO
                __builtin_amdgcn_s_setprio(1);   // (the batch's head; its steps go on at 0: contact_batch)
#endif
                contact_batch(P, T, B, S, S_thr, S_guide, S_cthr, S_cguide, lds_crows, S_pressure, lds_rows, uniform_meta, grouped, dp, L.strip + L.qn, n, C, day_flags);
#ifndef REINA_NO_DAY_PRIO
                __builtin_amdgcn_s_setprio(2);
#endif
                PROF_END(BATCHES);
                continue;
            }
            if (nqn >= (more ? 64u : 1u)) {
                const uint32_t n = nqn < 64u ? nqn : 64u;
                nqn -= n;
                __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): the wave-private queue is written
                __builtin_amdgcn_wave_barrier();
                PROF_DRAINED(FEED_DRAIN);
                PROF_BEGIN(ROUNDS);
                const bool valid = (uint32_t)lane < n;
                const uint2 q = valid ? nq[nqn + lane] : make_uint2(0u, 0u);
                // (bed / ICU events: staged in LDS while the stream runs, straight to their buckets from the rounds that drain the
                // queue when it has ended -- a small population's only rounds: a flush behind the closing barrier would be
                // a round trip on every workgroup's way out)
                const uint32_t nw = scan_word(P, B, L, valid, q.x, q.y, dp.day, &S.ev_n, S.ev_key, more ? DAY_EV_STAGE : 0u, S.var_par);
                // a deferred (onset) word keeps its old value here and is written by become_ill
                if (valid && nw != q.y && !ABLATED(HOT_STORE)) B.hot[q.x] = nw;
                PROF_END(ROUNDS);
                PROF_DRAINED(ROUND_DRAIN);
                continue;
            }
            break;
        }
        if (!more) break;
    }
    DIAG_SINCE(DAY, DIAG_DAY_STREAM, DIAG_THREAD0, ds_t0, B.mirror);
    PROF_END(LOOP);
    PROF_BEGIN(TAIL);
    // the wave's last pending contacts: the batch in flight, then the fewer than 64 of the region being filled
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_wave_barrier();
    if (C.fl) resolve_finish(P, T, B, S, S_pressure, uniform_meta, dp, (C.cur ^ 1u) * 64u, C);
    if (C.n_pend) {
        resolve_issue(P, T, B, S, S_thr, S_guide, lds_rows, uniform_meta, dp, C.cur * 64u, C.n_pend, C);
        resolve_finish(P, T, B, S, S_pressure, uniform_meta, dp, C.cur * 64u, C);
    }
    asm volatile("s_waitcnt vmcnt(0)" : : : "memory");   // (the loads past the end that were never looked at)
    PROF_END(TAIL);
    PROF_WRITE_ROW(B.mirror, wave_global, C);
#undef DAY_PUSH
#undef DAY_WORD
#undef DAY_WORD_REG
#undef SP_ISSUE
#undef SP_ISSUE_REGS
#undef SP_TAKE
#undef SP_TAKE_REGS
#undef DAY_ISSUE
#undef DAY_MASK
#undef DAY_ISSUE_REGS
#undef DAY_MASK_REGS
    if (lane < 4) {
        const uint32_t c = lane == 0 ? (C.n_cand < C.slice_cap ? C.n_cand : C.slice_cap) : lane == 1 ? L.n[1] : lane == 2 ? 0u : L.n[3];
        B.work_counts[(lane == 0 ? LIST_CAND : lane) * REINA_MAX_SCAN_WAVES + wave_global] = c;
    }
    DIAG_SINCE(DAY, DIAG_DAY_RESOLVED, DIAG_THREAD0, ds_t0, B.mirror);
    flush_places(S.daily, (uint32_t)C.pl & 0x3FFFFFFFu, (uint32_t)(C.pl >> 30) & 0x3FFFFFFFu);
    if (lane == 0 && C.wave_contacts) atomicAdd(&S.n_contacts, (int)C.wave_contacts);
    if (lane == 0 && n_act) atomicAdd(&S.n_active, (int)n_act);
    if (lane == 0 && L.n_hosp) atomicAdd(&S.n_hosp, (int)L.n_hosp);   // (the day's admission / transfer requests: hosp_day_is_ordered)
    if (lane == 0 && L.n_icu) atomicAdd(&S.n_icu, (int)L.n_icu);
    __syncthreads();
    DIAG_SINCE(DAY, DIAG_DAY_BARRIER, DIAG_THREAD0, ds_t0, B.mirror);
    // the workgroup's staged bed / ICU events go to their priority buckets: one returning atomic per event, all of them in
    // flight together (rounds 1-3: one in the middle of every state-machine round that found an event)
    {
        const uint32_t n_ev = S.ev_n < DAY_EV_STAGE ? S.ev_n : DAY_EV_STAGE;
        for (uint32_t k = (uint32_t)tid; k < (ABLATED(EVENT_PUSH) ? 0u : n_ev); k += DAY_THREADS) hosp_push_key(P, B, S.ev_key[k]);
    }
    // The workgroup's sums, in TWO vector instructions: an atomic instruction occupies the L2 line it addresses for some 12 ns
    // whatever the number of its lanes and words (tools/ubench_atomics.hip), and the control words of a day share one line, its
    // scalar counters another.  (Until round 4 every WAVE added its admission / transfer requests to the control line by itself --
    // 8192 instructions on the peak day at 10^8 agents, 100 us of that line's time -- and a workgroup issued four more.)
    {
        static_assert(REINA_L_CONTACTS < 32 && REINA_L_EV_HOSPITALIZE < 32 && REINA_L_EV_TO_ICU < 32 && REINA_L_ACTIVE + 1 < 32, "one line");
        static_assert(REINA_S_DAILY_CONTACTS + REINA_NR_PLACES <= REINA_S_NR && REINA_S_EXPOSED_PER_DAY < REINA_S_DAILY_CONTACTS, "one instruction");
        const int cw = tid == 0 ? REINA_L_CONTACTS : tid == 1 ? (int)(REINA_L_ACTIVE + (dp.day & 1u)) : tid == 2 ? REINA_L_EV_HOSPITALIZE : REINA_L_EV_TO_ICU;
        const int cv = tid == 0 ? S.n_contacts : tid == 1 ? S.n_active : tid == 2 ? S.n_hosp : S.n_icu;
        if (tid < 4 && cv) atomicAdd(&B.control[cw], cv);
        // (counters: daily_contacts by place, and exposed_per_day = the sum of the counts drawn)
        const int sv = tid < REINA_NR_PLACES ? S.daily[tid] : S.n_contacts;
        if (tid <= REINA_NR_PLACES && sv)
            atomicAdd(&B.counters[SC_IDX(tid < REINA_NR_PLACES ? REINA_S_DAILY_CONTACTS + tid : REINA_S_EXPOSED_PER_DAY)], sv);
        if (P->n_shards > 1 && tid >= 2 && tid < 4 && cv)   // ... and to the words the all-reduce carries (capacity follows demand)
            atomicAdd(&B.pressure[tid == 2 ? REINA_PRESSURE_DEMAND_BEDS(P->shard_rank) : REINA_PRESSURE_DEMAND_ICU(P->shard_rank)], cv);
    }
    if (IS_EXACT(P)) {
        // exact attribution: the workgroup's staged contact records to the segments of their shards (one returning atomic per
        // wave and destination: k_common.inc xsend_push)
        const uint32_t n_rec = (uint32_t)S_pressure[0] < DAY_XSTAGE ? (uint32_t)S_pressure[0] : DAY_XSTAGE;
        for (uint32_t k = (uint32_t)tid; k < n_rec; k += DAY_THREADS) {
            const uint64_t r = (uint64_t)(uint32_t)S_pressure[2u + 2u * k] | ((uint64_t)(uint32_t)S_pressure[3u + 2u * k] << 32);
            xsend_push(P, B, rp_gid_shard(rp_xrec_gid(r)), rp_xrec(rp_xrec_index(r), rp_xrec_flags(r), P->gid_base | (rp_xrec_gid(r) & RP_GID_INDEX_MASK)));
        }
    } else if (P->n_shards > 1) {
        for (int k = tid; k < REINA_PRESSURE_WORDS; k += DAY_THREADS)
            if (S_pressure[k]) atomicAdd(&B.pressure[k], S_pressure[k]);
    }
}

// k_day: the stream as a launch of its own -- every population but the small unsharded ones whose day is one launch (k_small_day).
// Compiled for 104 VGPRs: v104..v127 are the hand-scheduled feeds' (day_block).
template <bool GROUP, bool EXACT, bool SPARSE>
__global__ __launch_bounds__(DAY_THREADS) __attribute__((amdgpu_num_vgpr(104))) void k_day(const MemberRef *M_, MemberRef one_, reina_day_t dp,
                                                                                           uint32_t lds_rows_launch, uint32_t lds_crows_launch,
                                                                                           uint32_t day_flags, uint32_t import_wgs) {
    MEMBER_OF_LAUNCH;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    day_block<EXACT, SPARSE ? FEED_SPARSE : FEED_DENSE>(mref_, dp, lds_rows_launch, lds_crows_launch, day_flags, import_wgs, blockIdx.x, gridDim.x, smem_raw);
}
