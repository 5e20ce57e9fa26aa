// reina_hip.hip part: k_init and the day-opening workgroup: snapshot, beds, import placement, vaccination.
// Included by reina_hip.hip only (one translation unit); not a standalone header.
// ---------------------------------------------------------------------------------------------
// k_init: _create_agents / _init_stats (main.pyx:1389-1450)
__global__ void k_init(const MemberRef *M_, int32_t beds, int32_t icu) {
    const MemberRef &mref_ = M_[blockIdx.y];
    const CAS DevParams *P = (const CAS DevParams *)mref_.P;
    const GBuffers B = global_buffers(mref_.B);  // by value: pointers live in SGPRs, never re-read after stores
    uint32_t N = P->n_agents;
    uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += stride) {
        B.hot[i] = 0;
        // (the record as two 16-byte stores: claim = all ones, infector -1, nobody infected | onset 0.0, never vaccinated,
        // no overflow infectees, no sibling)
        GAS v4u_ *rec = reinterpret_cast<GAS v4u_ *>(&B.cold[i]);
        v4u_ lo, hi;
        lo.x = 0xFFFFFFFFu; lo.y = 0xFFFFFFFFu; lo.z = 0xFFFFFFFFu; lo.w = 0u;
        hi.x = 0u; hi.y = 0xFFFFFFFFu; hi.z = 0xFFFFFFFFu; hi.w = 0xFFFFFFFFu;
        rec[0] = lo;
        rec[1] = hi;
    }
    for (size_t k = blockIdx.x * blockDim.x + threadIdx.x; k < (size_t)N * REINA_INLINE_INFECTEES; k += stride) B.infectees[k] = -1;
    for (size_t k = blockIdx.x * blockDim.x + threadIdx.x; k < REINA_BITS_WORDS(N); k += stride) B.active_bits[k] = B.infected_bits[k] = 0u;
    if (P->n_shards > 1) {
        const size_t nm = (size_t)REINA_MAX_RANGES * REINA_MAX_VARIANTS * P->mirror_slots;
        for (size_t k = blockIdx.x * blockDim.x + threadIdx.x; k < nm; k += stride) B.mirror[k] = ~0ull;
        if (blockIdx.x == 0 && threadIdx.x < REINA_MIRROR_CELLS) {   // smallest tables, no entries yet
            B.mirror_meta[threadIdx.x] = P->mirror_slots < RP_MIRROR_MIN_SLOTS ? P->mirror_slots : RP_MIRROR_MIN_SLOTS;
            B.mirror_meta[REINA_MIRROR_CELLS + threadIdx.x] = 0;
        }
    }
    if (P->exact) xsend_reset(P, B);   // (no records bound for anybody)
    if (blockIdx.x == 0) {
        // (the words of k_vaccinate's chain of workgroups, in the unused head of the scan lists: zero between launches)
        for (uint32_t k = threadIdx.x; k < 2u * (REINA_MAX_VACCINATIONS * 512u + REINA_MAX_VACCINATIONS) && k < 2u * P->max_work_items; k += blockDim.x) B.scan_lists[k] = 0u;
        for (uint32_t k = threadIdx.x; k < REINA_COUNTER_WORDS; k += blockDim.x) {
            int32_t v = 0;
            if (k >= CNT_IDX(REINA_C_SUSCEPTIBLE, 0) && k < CNT_IDX(REINA_C_SUSCEPTIBLE, 0) + P->nr_ages) {
                uint32_t a = k - CNT_IDX(REINA_C_SUSCEPTIBLE, 0);
                v = P->age_start[a + 1] - P->age_start[a];
            }
            if (k == SC_IDX(REINA_S_AVAILABLE_BEDS) || k == SC_IDX(REINA_S_BEDS)) v = beds;
            if (k == SC_IDX(REINA_S_AVAILABLE_ICU) || k == SC_IDX(REINA_S_ICU_UNITS)) v = icu;
            B.counters[k] = v;
        }
        for (uint32_t k = threadIdx.x; k < REINA_L_NR; k += blockDim.x)
            B.control[k] = (k >= REINA_L_VACC_CURSOR && k < REINA_L_VACC_CURSOR + REINA_MAX_VACCINATIONS) ? INT_MIN : 0;
    }
}

// ---------------------------------------------------------------------------------------------
// k_prologue: single workgroup of 1024 threads.
#define PRO_MAX_IMPORTS 16384

// Population.infect_people / get_import_infection_person (main.pyx:1632-1665), parallel form.
// Each import owns up to 10 tries (draws keyed by import number and try); pro_imports below finds, as a stable
// matching, the placement the reference reaches by working the imports off one after the other.
// the imported-infection age classes, staged once per workgroup (get_import_infection_person walks their cumulative
// weights for every try of every import: from HBM that was a chain of dependent loads per call)
struct ImportClasses {
    uint32_t n;
    float cum[REINA_MAX_IMPORT_CLASSES];
    uint32_t start[REINA_MAX_IMPORT_CLASSES], end[REINA_MAX_IMPORT_CLASSES];   // first agent of the class's youngest age, one past its oldest
};
__device__ __forceinline__ void import_classes_load(const CAS DevParams *P, const int32_t *s_age_start, ImportClasses *ic) {
    // (call with the age table staged and a barrier behind it; ends with a barrier)
    const CAS reina_disease_t &d = P->dis;
    if (threadIdx.x == 0) ic->n = d.n_import_classes;
    if (threadIdx.x < REINA_MAX_IMPORT_CLASSES) {
        const uint32_t q = threadIdx.x;
        const bool in = q < d.n_import_classes;
        ic->cum[q] = in ? (float)d.import_class_cum[q] : 2.0f;
        ic->start[q] = in ? (uint32_t)s_age_start[d.import_class_min_age[q]] : 0u;
        ic->end[q] = in ? (uint32_t)s_age_start[d.import_class_max_age[q] + 1] : 0u;
    }
    __syncthreads();
}
__device__ __forceinline__ bool import_target(const CAS DevParams *P, const ImportClasses *ic, const reina_day_t &dp,
                                              uint32_t j, uint32_t k, uint32_t *t_out) {
    rp_u4 r = rp_philox(P->k0, P->k1, j, dp.day, RP_P_IMPORT, k);
    float p = rp_uniform24(r.v[0]);
    uint32_t c = ic->n - 1;
    for (uint32_t q = 0; q < ic->n; q++)
        if (p <= ic->cum[q]) {
            c = q;
            break;
        }
    const uint32_t start = ic->start[c], end = ic->end[c];
    if (end <= start) return false;
    *t_out = start + r.v[1] % (end - start);
    return true;
}

// A batch of imports may be shared by W workgroups of the opening launch (weekly imports of a large population: 7000 a week
// at 10^8 agents -- seven per lane of ONE workgroup, whose scattered reads a single CU then has in flight alone: 52 + 14 +
// 56 us for propose / verify / infect, measured).  Imports are dealt out a wave at a time (chunk-relative import
// ((s / 64) * W + r) * 64 + s % 64 sits in slot s of workgroup r), the claims are global atomics as before, and the two
// questions "did anybody propose?" / "was anybody evicted?" are asked of all W workgroups: imports_any() is a barrier over
// them that ORs a flag (arrival counters in four rotating control words; the workgroups are those that took tickets
// 1..W of this launch, so all of them are running or about to while the others of the launch wait for nothing; bounded
// wait -> REINA_PROBLEM_SYNC_TIMEOUT).  The fixed point is the same one -- it does not depend on who proposes when.
__device__ __forceinline__ bool imports_any(const GBuffers &B, uint32_t r, uint32_t W, uint32_t &phase, int mine) {
    const int any = __syncthreads_or(mine);
    if (W == 1) return any != 0;
    __shared__ int s_any;
    if (threadIdx.x == 0) {
        GAS int32_t *w = &B.control[REINA_L_IMPORT_SYNC + (phase & 3u)];
        __threadfence();
        atomicAdd(w, 1 + (any ? 0x10000 : 0));
        int v;
        uint32_t polls = 0;
        while (((v = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) & 0xFFFF) != (int)W) {
            __builtin_amdgcn_s_sleep(2);
            if (++polls > (1u << 22)) {
                set_problem(B.counters, REINA_PROBLEM_SYNC_TIMEOUT);
                v = 0;
                break;
            }
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        // the word of two phases ago: everybody has read it (they all arrived here), nobody arrives at it again before
        // this workgroup's next arrival, which is ordered behind this store
        if (r == 0) __hip_atomic_store(&B.control[REINA_L_IMPORT_SYNC + ((phase + 2u) & 3u)], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_any = v >> 16;
    }
    __syncthreads();
    phase++;
    return s_any != 0;
}
#define IMPORT_OF_SLOT(s) ((((s) >> 6) * W + r) * 64u + ((s) & 63u))

// `deferred` (round 4): the placement runs in k_day's launch, BESIDE the day's contact sampling, and the infections are
// installed with the day's winners by the last launch.  The reference places the weekly imports before the scan
// (Population.init_day, main.pyx:1687-1699 -> infect_people_daily :1671-1685); a person infected today does nothing
// today (:402) and cannot be infected again (:239) -- which is all that order means.  The same holds here when the
// imports CLAIM their targets with keys that beat every contact's (the day tag of tomorrow: smaller than any key of today)
// and the claims are decided at night: an import's tries depend only on who was susceptible this morning (the infected
// bit plane, which nobody writes while k_day runs) and on the lower imports; a contact that meets an import's target
// loses the claim, exactly as if it had met an infected person.  Same placement, same result as oracle B's sequential
// walk -- and the 20 us chain of dependent round trips (10^8 agents: 423 imports a day from July on) leaves the day's
// critical path: it ran alone in front of the stream on 230 days of the year.
#define IMPORT_RECORD_FLAG 0x10000u   // candidate record z: an import's claim (y = import number; installed with no infector)
__device__ __forceinline__ uint64_t import_key(const reina_day_t &dp, bool deferred, uint32_t id) {
    return rp_order_key(deferred ? dp.day + 1u : dp.day, 0xFFFFFu, id);
}
__device__ void pro_imports(const CAS DevParams *P, const GBuffers &B, const reina_day_t &dp, int pre_init,
                            uint32_t *import_base, uint8_t *placed, uint32_t *s_unplaced,
                            int32_t *new_by_age, int32_t *new_by_variant, const int32_t *s_age_start, const ImportClasses *ic,
                            uint32_t &phase, bool wait_for_open = false, uint32_t r = 0, uint32_t W = 1, bool deferred = false) {
    DIAG_CLOCK(IMPORTS, ip_t);   // (-DREINA_OPEN_STAMPS: the placement's phases in the weekly-import workgroup, helper 0)
    uint32_t total = 0;
    for (uint32_t b = 0; b < dp.n_import_batches; b++)
        if ((int)dp.import_batches[b].pre_init == pre_init) total += dp.import_batches[b].count;
    if (total == 0) return;
    const uint32_t base = *import_base;
    uint32_t mine = 0;   // this thread's imports left unplaced
    // imports are worked off in chunks of PRO_MAX_IMPORTS (the LDS bookkeeping), rounds per chunk
    for (uint32_t c0 = 0; c0 < total; c0 += W * PRO_MAX_IMPORTS) {
        const uint32_t n = total - c0 < W * PRO_MAX_IMPORTS ? total - c0 : W * PRO_MAX_IMPORTS;
        // The reference places the imports one after the other: import j walks its <= 10 tries and takes the first target
        // that is still susceptible -- i.e. not taken by an import before it.  The parallel form of exactly that outcome is a
        // stable matching: targets prefer lower import numbers, imports prefer earlier tries.  placed[j]: the next try
        // (0..10, 10 = gave up) of an import that holds nothing, or 0x80 | try of one that holds its target's claim.
        //   propose  an import that holds nothing goes on to its first remaining try whose target is susceptible and not
        //            claimed by a LOWER import (a claim only ever passes to lower numbers: what is closed to j stays closed),
        //            and claims it (atomicMin of the import number) -- taking it from a higher import if one holds it;
        //   verify   an import whose claim has been taken goes back to proposing from its next try.
        // When nothing changes any more every claimed target belongs to the lowest import that wants it: the sequential
        // result, bit for bit (oracle B places the imports sequentially).  Usually one pass.
        __syncthreads();
        for (uint32_t sl = threadIdx.x; sl < PRO_MAX_IMPORTS && IMPORT_OF_SLOT(sl) < n; sl += PRO_THREADS) placed[sl] = 0;
        __syncthreads();
        DIAG_LAP(IMPORTS, DIAG_IMPORTS_SETUP, DIAG_THREAD0, ip_t, B.mirror, wait_for_open && r == 0);
        for (;;) {
            int proposals = 0;
            for (uint32_t sl = threadIdx.x; sl < PRO_MAX_IMPORTS; sl += PRO_THREADS) {
                const uint32_t j = IMPORT_OF_SLOT(sl);
                if (j >= n) break;
                uint32_t k = placed[sl];
                if (k & 0x80u) continue;   // holds a target
                const unsigned long long key = (unsigned long long)import_key(dp, deferred, base + c0 + j);
                // (Measured dead ends, round 3: the remaining tries requested four at a time -- with half the population infected
                // the slowest of a few hundred imports needs seven tries -- made this phase 14.6 us instead of 9.8 at 10^8 agents:
                // one CU keeps about 330 scattered reads per microsecond going, and four tries per lane are four times the reads;
                // with one workgroup per wave of imports the phase fell to 7.4 us, and the two barriers over the workgroups took
                // the gain back.  Keeping the word and vaccination day read here for the infection below: no gain either.)
                for (; k < 10; k++) {
                    uint32_t t = 0;
                    if (!import_target(P, ic, dp, base + c0 + j, k, &t)) continue;
                    // (both words requested side by side: one round trip; beside the stream the morning's state is the bit plane)
                    const bool taken = deferred ? agent_bit(B.infected_bits, t) : RH_STATE(ld_hot(&B.hot[t])) != RS_SUSCEPTIBLE;
                    const unsigned long long held = ld_claim(&B.cold[t].claim);
                    if (taken || held < key) continue;   // infected, or a lower import of today holds it
                    atomicMin((unsigned long long *)&B.cold[t].claim, key);
                    proposals++;
                    break;
                }
                placed[sl] = (uint8_t)(k < 10 ? (0x80u | k) : 10u);
            }
            DIAG_LAP(IMPORTS, DIAG_IMPORTS_PROPOSE, DIAG_THREAD0, ip_t, B.mirror, wait_for_open && r == 0);
            if (!imports_any(B, r, W, phase, proposals)) break;
            DIAG_LAP(IMPORTS, DIAG_IMPORTS_ANY_PROPOSED, DIAG_THREAD0, ip_t, B.mirror, wait_for_open && r == 0);
            int evicted = 0;
            for (uint32_t sl = threadIdx.x; sl < PRO_MAX_IMPORTS; sl += PRO_THREADS) {
                const uint32_t j = IMPORT_OF_SLOT(sl);
                if (j >= n) break;
                const uint32_t st = placed[sl];
                if (!(st & 0x80u)) continue;
                uint32_t t = 0;
                import_target(P, ic, dp, base + c0 + j, st & 0x7Fu, &t);
                if (ld_claim(&B.cold[t].claim) != import_key(dp, deferred, base + c0 + j)) {
                    placed[sl] = (uint8_t)((st & 0x7Fu) + 1u);   // a lower import took the target: on with the next try
                    evicted++;
                }
            }
            DIAG_LAP(IMPORTS, DIAG_IMPORTS_VERIFY, DIAG_THREAD0, ip_t, B.mirror, wait_for_open && r == 0);
            if (!imports_any(B, r, W, phase, evicted)) break;
        }
        DIAG_LAP(IMPORTS, DIAG_IMPORTS_LEFT_ROUNDS, DIAG_THREAD0, ip_t, B.mirror, wait_for_open && r == 0);
        // every holder's target is its own: infect
        for (uint32_t sl = threadIdx.x; sl < PRO_MAX_IMPORTS; sl += PRO_THREADS) {
            const uint32_t j = IMPORT_OF_SLOT(sl);
            if (j >= n) break;
            const uint32_t st = placed[sl];
            if (!(st & 0x80u)) continue;
            uint32_t t = 0;
            import_target(P, ic, dp, base + c0 + j, st & 0x7Fu, &t);
            uint32_t variant = 0, acc = 0, mode = dp.testing_mode;   // (the mode in force when the batch was imported)
            for (uint32_t b = 0; b < dp.n_import_batches; b++) {
                if ((int)dp.import_batches[b].pre_init != pre_init) continue;
                acc += dp.import_batches[b].count;
                if (c0 + j < acc) {
                    variant = dp.import_batches[b].variant;
                    mode = dp.import_batches[b].testing_mode;
                    break;
                }
            }
            if (deferred) {
                // a record among the day's candidates (the shared overflow list: an import is one record in a million contacts)
                const uint32_t o = (uint32_t)atomicAdd(&B.control[REINA_L_CAND_OVF], 1);
                if (o < P->cand_ovf_cap)
                    gst(&reinterpret_cast<GAS uint4 *>(B.candidates)[P->cand_ovf_base + o],
                        make_uint4(t, base + c0 + j, variant | IMPORT_RECORD_FLAG | (mode << 24), 0xFFFFFu));
                else
                    set_problem(B.counters, REINA_PROBLEM_CANDIDATE_OVERFLOW);
            } else {
                // (the import holds its target's claim: nobody else installs there today -- word and vaccination day requested
                // together, the new word stored without a compare-and-swap)
                const uint32_t w = ld_hot(&B.hot[t]);
                const int32_t vd = B.cold[t].vacc_day;
                install_infection(P, B, s_age_start, t, w, dp.day, variant, -1, 1, mode, new_by_age, new_by_variant, 0u, vd, true);
            }
            placed[sl] = 255;
        }
        DIAG_LAP(IMPORTS, DIAG_IMPORTS_INFECT, DIAG_THREAD0, ip_t, B.mirror, wait_for_open && r == 0);
        __syncthreads();
        for (uint32_t sl = threadIdx.x; sl < PRO_MAX_IMPORTS; sl += PRO_THREADS) {
            if (IMPORT_OF_SLOT(sl) >= n) break;
            if (placed[sl] != 255) mine++;
        }
    }
    if (threadIdx.x == 0) *s_unplaced = 0;
    // agents are placed; the counters follow the daily zeroing (a wait that gave up has flagged the day
    // failed: the counters, possibly not zeroed yet, are then left alone)
    DIAG_LAP(IMPORTS, DIAG_IMPORTS_TAIL, DIAG_THREAD0, ip_t, B.mirror, wait_for_open && r == 0);
    const bool counters_open = !wait_for_open || wait_day_open(B, dp.day);
    __syncthreads();
    DIAG_LAP(IMPORTS, DIAG_IMPORTS_WAIT_OPEN, DIAG_THREAD0, ip_t, B.mirror, wait_for_open && r == 0);
    if (mine) atomicAdd(s_unplaced, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (*s_unplaced && counters_open) atomicAdd(&B.counters[SC_IDX(REINA_S_UNABLE_TO_IMPORT)], (int)*s_unplaced);
        *import_base += total;
    }
    if (counters_open && !deferred) flush_new_infections(B, new_by_age, new_by_variant, PRO_THREADS);
    // shared intervention imports: the opening workgroup goes on to zero the day's counters only when every helper's
    // counts are in
    if (W > 1 && pre_init) imports_any(B, r, W, phase, 0);
    DIAG_LAP(IMPORTS, DIAG_IMPORTS_FLUSH, DIAG_THREAD0, ip_t, B.mirror, wait_for_open && r == 0);
}

// HealthcareSystem.vaccinate_people (main.pyx:560-583): oldest first from a persistent cursor.
// One workgroup; a step looks at VACC_CHUNKS x 1024 agents below the cursor -- chunk j of it is the agents c - 1024 j - tid, one
// coalesced load per chunk, all of them in flight together --, ranks the eligible ones in descending index (ballots per chunk and
// wave, a prefix over the 16 x VACC_CHUNKS counts) and vaccinates those whose rank is below the day's number.  Counted by age in
// LDS and added to the counters once.  (Until the end of round 4 a step was ONE chunk with three barriers, and every vaccinated
// agent added 1 to its age's counter by a global atomic -- neighbours in the index share their age, so a wave's 64 adds hit one
// WORD and L2 takes them one by one, 12 ns each: 476 000 vaccinations a day at 10^8 agents were 6.8 ms, sixty times the rest of
// the day; tools/vacc_probe.py.)
struct VaccLds {
    uint32_t cnt[16 * VACC_CHUNKS], pre[16 * VACC_CHUNKS], tot[16 * VACC_CHUNKS / 64];
    int32_t hist[REINA_MAX_AGES], age_start[REINA_MAX_AGES + 1];
    int32_t scalar;          // the cursor behind the day's last vaccinated agent (INT_MIN: not reached in this step)
    uint32_t chain_pre;      // chained launch: eligible agents in the workgroups in front of this one
    int32_t chain_cur;       // ... and the final cursor, if one of them reached the day's number
};
// One step: the VACC_CHUNKS x 1024 agents at and below c; `done` eligible agents lie in front of them.  Vaccinates those whose
// rank is below nr, returns the step's number of eligible agents (all threads); S.scalar is set by the thread that vaccinates
// number nr - 1.
// `front(total)`: the eligible agents in front of this step, asked for once the step's own number is known (the chained launch
// publishes that number and collects the others' there; all threads call it, it may hold barriers)
template <class F>
__device__ __forceinline__ uint32_t vacc_step(const CAS DevParams *P, const GBuffers &B, const reina_day_t &dp, const reina_vaccination_t &v,
                                              VaccLds &S, int32_t c, F front, uint32_t nr) {
    static_assert(PRO_THREADS == 1024 && (16 * VACC_CHUNKS) % 64 == 0 && 16 * VACC_CHUNKS <= PRO_THREADS, "one count per (chunk, wave), prefixed by the first waves");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t elig = 0;   // bit j: this thread's agent of chunk j can be vaccinated
    uint32_t hw[VACC_CHUNKS];   // (the chunks' words requested together: nothing else writes hot words while this launch runs)
#pragma unroll
    for (int j = 0; j < VACC_CHUNKS; j++) {
        const int32_t i = c - (int32_t)(j * PRO_THREADS + tid);
        hw[j] = i >= (int32_t)v.idx_start ? (uint32_t)B.hot[i] : (uint32_t)RH_VACCINATED;
    }
#pragma unroll
    for (int j = 0; j < VACC_CHUNKS; j++) {
        const uint32_t w = hw[j];
        const bool e = !(RH_STATE(w) == RS_DEAD || (w & (RH_VACCINATED | RH_DETECTED)));
        const uint64_t m = __ballot(e);
        if (e) elig |= 1u << j;
        if (lane == 0) S.cnt[j * (PRO_THREADS / 64) + wave] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    // exclusive prefix of the counts in order (chunk, wave): inside groups of 64 by shuffles, the groups' totals beside them
    if (tid < 16 * VACC_CHUNKS) {
        const uint32_t x = S.cnt[tid];
        uint32_t inc = x;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)inc, off);
            if (lane >= off) inc += y;
        }
        S.pre[tid] = inc - x;
        if (lane == 63) S.tot[wave] = inc;
    }
    __syncthreads();
    uint32_t total = 0;
#pragma unroll
    for (int q = 0; q < 16 * VACC_CHUNKS / 64; q++) total += S.tot[q];
    const uint32_t done = front(total);
    if (done >= nr) return total;   // (chained launch: the day's number was reached in front of this workgroup)
    int age = -1;   // of this thread's last vaccinated agent: the next one is 1024 x k places below it, its age found by a walk down
#pragma unroll
    for (int j = 0; j < VACC_CHUNKS; j++) {
        const bool e = ((elig >> j) & 1u) != 0u;
        const uint64_t m = __ballot(e);
        if (!m) continue;   // (wave-uniform)
        const uint32_t slot = (uint32_t)(j * (PRO_THREADS / 64) + wave);
        uint32_t before = S.pre[slot];
        for (uint32_t q = 0; q < (slot >> 6); q++) before += S.tot[q];
        const uint32_t pos = done + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));   // 0-based order among the eligible, oldest first
        const bool take = e && pos < nr;
        const uint64_t mt = __ballot(take);
        if (!mt) continue;
        const int32_t i = c - (int32_t)(j * PRO_THREADS + tid);
        if (take) {
            atomicOr(&B.hot[i], RH_VACCINATED);   // (nothing comes back: the sixteen words need not be kept across the step's barriers)
            B.cold[i].vacc_day = (int32_t)dp.day;
            if (age < 0) age = age_of(S.age_start, (uint32_t)i, 0, (int)P->nr_ages - 1);
            else while (age > 0 && S.age_start[age] > i) age--;
            if (pos == nr - 1) S.scalar = i - 1;  // the sequential loop stops right after this one
        }
        // neighbours in the index share their age: one LDS add for the wave when they all do
        const int first = __ffsll((unsigned long long)mt) - 1;
        const int a0 = __builtin_amdgcn_readlane(age, first);
        if (__ballot(take && age == a0) == mt) {
            if (lane == first) atomicAdd(&S.hist[a0], (int)__popcll(mt));
        } else if (take) {
            atomicAdd(&S.hist[age], 1);
        }
    }
    return total;
}
// steps from (c, done) until the day's number is reached or the programme's range is used up; returns the cursor
__device__ __forceinline__ int32_t vacc_steps(const CAS DevParams *P, const GBuffers &B, const reina_day_t &dp, const reina_vaccination_t &v,
                                              VaccLds &S, int32_t c, uint32_t done, uint32_t nr) {
    while (done < nr && c >= (int32_t)v.idx_start) {
        const uint32_t total = vacc_step(P, B, dp, v, S, c, [done](uint32_t) { return done; }, nr);
        __syncthreads();
        if (done + total >= nr) {
            c = S.scalar;
            done = nr;
        } else {
            done += total;
            c -= VACC_CHUNKS * PRO_THREADS;
        }
        __syncthreads();
    }
    return c;
}
__device__ __forceinline__ void vacc_begin(const CAS DevParams *P, VaccLds &S) {
    for (int t = threadIdx.x; t <= REINA_MAX_AGES; t += PRO_THREADS) S.age_start[t] = P->age_start[t];
    for (int t = threadIdx.x; t < REINA_MAX_AGES; t += PRO_THREADS) S.hist[t] = 0;
    if (threadIdx.x == 0) S.scalar = INT_MIN;
    __syncthreads();
}
__device__ __forceinline__ void vacc_end(const GBuffers &B, VaccLds &S) {
    __syncthreads();
    for (int t = threadIdx.x; t < REINA_MAX_AGES; t += PRO_THREADS)
        if (S.hist[t]) atomicAdd(&B.counters[CNT_IDX(REINA_C_VACCINATED, t)], S.hist[t]);
}
// the day's programmes one after the other, by ONE workgroup
__device__ __forceinline__ void pro_vaccinate(const CAS DevParams *P, const GBuffers &B, const reina_day_t &dp, VaccLds &S) {
    vacc_begin(P, S);
    for (uint32_t k = 0; k < dp.n_vaccinations; k++) {
        const reina_vaccination_t v = dp.vaccinations[k];
        int32_t c = B.control[REINA_L_VACC_CURSOR + v.slot];
        if (c == INT_MIN) c = (int32_t)v.idx_end - 1;
        uint32_t nr = v.nr;
        if (nr > v.idx_end - v.idx_start) nr = v.idx_end - v.idx_start;
        c = vacc_steps(P, B, dp, v, S, c, 0u, nr);
        if (c < (int32_t)v.idx_start - 1) c = (int32_t)v.idx_start - 1;
        if (threadIdx.x == 0) B.control[REINA_L_VACC_CURSOR + v.slot] = c;
        __syncthreads();
    }
    vacc_end(B, S);
}
// k_vaccinate's chained launch: the counts of steps [0, n) summed into S.chain_pre by the first wave (lane l: steps l, l + 64, ...);
// S.chain_cur = the step in which the running sum reaches nr, or -1.  All threads call it (it ends with a barrier).
__device__ __forceinline__ void vacc_collect(GAS int32_t *counters, VaccLds &S, const GAS unsigned long long *word, unsigned long long tag, uint32_t nr, uint32_t n) {
    const int tid = threadIdx.x;
    if (tid < 64) {
        uint32_t mine[4] = {0, 0, 0, 0};
        bool ok = true;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint32_t q = (uint32_t)tid + 64u * (uint32_t)r;
            if (q < n) {
                uint32_t polls = 0;
                unsigned long long w;
                while (((w = __hip_atomic_load(&word[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 32) != (tag >> 32)) {
                    __builtin_amdgcn_s_sleep(4);
                    if (++polls > (1u << 22)) { ok = false; w = 0; break; }
                }
                mine[r] = (uint32_t)w;
            }
        }
        if (!ok) set_problem(counters, REINA_PROBLEM_SYNC_TIMEOUT);
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        // running sums in step order: r-th group of 64 steps after the groups before it
        uint32_t base = 0, sum = 0;
        int hit = -1;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            uint32_t inc = mine[r];
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const uint32_t y = (uint32_t)__shfl_up((int)inc, off);
                if (tid >= off) inc += y;
            }
            const uint32_t before = base + inc - mine[r];
            if (hit < 0 && before < nr && before + mine[r] >= nr && (uint32_t)tid + 64u * (uint32_t)r < n) hit = tid + 64 * r;
            base += (uint32_t)__shfl((int)inc, 63);
        }
        sum = base;
        // (at most one lane found the step)
        int h = hit;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int o = __shfl_xor(h, off);
            h = o > h ? o : h;
        }
        if (tid == 0) {
            S.chain_pre = sum;
            S.chain_cur = h;
        }
    }
    __syncthreads();
}
// what vacc_step asks once it knows its own count: publish it, collect the counts in front
struct VaccFront {
    GAS int32_t *counters;
    VaccLds *S;
    GAS unsigned long long *word;
    unsigned long long tag;
    uint32_t nr, b;
    __device__ __forceinline__ uint32_t operator()(uint32_t total) const {
        if (threadIdx.x == 0) __hip_atomic_store(&word[b], tag | (unsigned long long)total, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        vacc_collect(counters, *S, word, tag, nr, b);
        return S->chain_pre;
    }
};
// The day's programmes by the launch's G workgroups, one programme after the other (a day on which some programme's number exceeds
// one step: reina_hip.hip).  For a programme, workgroup b takes the step at c - 16 384 b: counts its eligible agents, PUBLISHES the
// count (launch tag | count, in the head of buffers.scan_lists -- the exposure list's slice region, unused since the exposure records
// stay in LDS; 512 words per programme), collects the counts of the workgroups in front of it -- all of them are published at about
// the same time, so this is one round of polling, not a chain of dependent waits -- and vaccinates its share.  The workgroup whose
// step holds number nr - 1 publishes the cursor behind it; the LAST workgroup, which has seen everybody's count, picks it up, or
// goes on alone step by step when the G steps did not hold enough eligible agents, writes the programme's cursor (every workgroup
// has read the old one before it published).  The reference works the programmes off one after the other (vaccinate_people,
// main.pyx:560-583: a person vaccinated by an earlier programme of the day is no longer eligible for a later one whose window
// overlaps), so the launch AGREES on every programme's end before the next one starts: an arrival word per programme.
// The words carry the LAUNCH's sequence number as a tag (round 5; until then the day: a caller that stepped the same day twice
// read the first pass's counts) and are never cleared during a run (k_init zeroes them).  All G workgroups are resident
// (G <= number of CUs); the waits are bounded by a poll count all the same (REINA_PROBLEM_SYNC_TIMEOUT).
#define VACC_PROGRAMME_WORDS 512u   // 64-bit words of one programme: [256] counts, [256] cursors
// programme k of the day by workgroups 0 .. G - 1 of a chain (this one: b)
__device__ __forceinline__ void vacc_chain_programme(const CAS DevParams *P, const GBuffers &B, const reina_day_t &dp, VaccLds &S, uint32_t k, uint32_t b, uint32_t G,
                                                     unsigned long long tag) {
    const int tid = threadIdx.x;
    const reina_vaccination_t v = dp.vaccinations[k];
    uint32_t nr = v.nr;
    const uint32_t window = v.idx_end > v.idx_start ? v.idx_end - v.idx_start : 0u;
    if (nr > window) nr = window;
    if (nr == 0u) return;   // (nothing to do, for every workgroup alike: the cursor stays)
    GAS unsigned long long *word = reinterpret_cast<GAS unsigned long long *>(B.scan_lists) + (size_t)k * VACC_PROGRAMME_WORDS;   // [256] tag | eligible agents of step q
    GAS unsigned long long *curw = word + 256;                                                                              // [256] tag | cursor, from the step that reached nr
    int32_t c0 = B.control[REINA_L_VACC_CURSOR + v.slot];
    if (c0 == INT_MIN) c0 = (int32_t)v.idx_end - 1;
    const int32_t c = c0 - (int32_t)(b * VACC_CHUNKS * PRO_THREADS);
    const VaccFront front = {B.counters, &S, word, tag, nr, b};
    uint32_t total = 0;
    if (c >= (int32_t)v.idx_start) {
        total = vacc_step(P, B, dp, v, S, c, front, nr);
    } else {
        front(0u);   // (a step below the programme's range: nothing of its own, but the others wait for its word)
    }
    __syncthreads();
    const uint32_t pre = S.chain_pre;
    const bool mine_reaches = pre < nr && pre + total >= nr;   // number nr - 1 is one of this step's: S.scalar is the cursor behind it
    if (b + 1u < G) {
        if (mine_reaches && tid == 0)
            __hip_atomic_store(&curw[b], tag | (unsigned long long)(uint32_t)S.scalar, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    int32_t fin;
    if (mine_reaches) {
        fin = S.scalar;
    } else if (pre >= nr) {
        // somebody in front reached the number: which step, from the counts; its cursor word
        vacc_collect(B.counters, S, word, tag, nr, b);
        const int hit = S.chain_cur;
        if (tid == 0) {
            uint32_t polls = 0;
            unsigned long long w = tag;
            if (hit >= 0) {
                while (((w = __hip_atomic_load(&curw[hit], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) >> 32) != (tag >> 32)) {
                    __builtin_amdgcn_s_sleep(4);
                    if (++polls > (1u << 22)) { set_problem(B.counters, REINA_PROBLEM_SYNC_TIMEOUT); break; }
                }
            } else {
                set_problem(B.counters, REINA_PROBLEM_SYNC_TIMEOUT);
            }
            S.chain_cur = (int32_t)(uint32_t)w;
        }
        __syncthreads();
        fin = S.chain_cur;
    } else {
        fin = vacc_steps(P, B, dp, v, S, c - (int32_t)(VACC_CHUNKS * PRO_THREADS), pre + total, nr);
    }
    if (fin < (int32_t)v.idx_start - 1) fin = (int32_t)v.idx_start - 1;
    if (tid == 0) B.control[REINA_L_VACC_CURSOR + v.slot] = fin;
    // (the words stay as they are: a workgroup in front may still be reading them; the next launch's tag is another, and a
    // new run starts from k_init's zeros)
}
__device__ __forceinline__ void pro_vaccinate_chain(const CAS DevParams *P, const GBuffers &B, const reina_day_t &dp, VaccLds &S, uint32_t b, uint32_t G,
                                                    uint32_t seq, const VaccGeom &geo) {
    vacc_begin(P, S);
    const unsigned long long tag = (unsigned long long)seq << 32;
    const int tid = threadIdx.x;
    if (geo.parallel) {
        uint32_t first = 0;
        for (uint32_t k = 0; k < dp.n_vaccinations; k++) {
            if (b < first + geo.g[k]) {
                vacc_chain_programme(P, B, dp, S, k, b - first, geo.g[k], tag);
                break;
            }
            first += geo.g[k];
        }
        vacc_end(B, S);
        return;
    }
    GAS unsigned long long *const arrive = reinterpret_cast<GAS unsigned long long *>(B.scan_lists) + (size_t)REINA_MAX_VACCINATIONS * VACC_PROGRAMME_WORDS;   // [programme] tag | workgroups through
    for (uint32_t k = 0; k < dp.n_vaccinations; k++) {
        vacc_chain_programme(P, B, dp, S, k, b, G, tag);
        if (k + 1u < dp.n_vaccinations) {
            // every workgroup's vaccinations of this programme (and the last one's cursor) before anybody looks at the next
            __syncthreads();
            if (tid == 0) {
                __threadfence();
                GAS unsigned long long *aw = &arrive[k];
                unsigned long long old = __hip_atomic_load(aw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), nw;
                do nw = ((old >> 32) == (tag >> 32) ? old : tag) + 1ull;
                while (!__hip_atomic_compare_exchange_strong(aw, &old, nw, __ATOMIC_RELEASE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
                uint32_t polls = 0;
                while (__hip_atomic_load(aw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != (tag | (unsigned long long)G)) {
                    __builtin_amdgcn_s_sleep(4);
                    if (++polls > (1u << 22)) { set_problem(B.counters, REINA_PROBLEM_SYNC_TIMEOUT); break; }
                }
                __atomic_thread_fence(__ATOMIC_ACQUIRE);
            }
            __syncthreads();
        }
    }
    vacc_end(B, S);
}

// LDS of the day-opening roles (one role per workgroup): carved from a block the kernel provides -- static in k_open,
// the front of its dynamic LDS in k_day, whose day-opening workgroups have no other use for it
struct OpenImportsLds {
    uint8_t placed[PRO_MAX_IMPORTS];
    uint32_t s_wave_cnt[PRO_THREADS / 64];
    uint32_t s_unplaced;
    int32_t s_scalar;
    uint32_t s_import_base;
    int32_t new_by_age[REINA_MAX_AGES];
    int32_t new_by_variant[REINA_MAX_VARIANTS];
    int32_t s_age_start[REINA_MAX_AGES + 1];
    ImportClasses classes;
};

__device__ __forceinline__ void prologue_block(const MemberRef &mref_, const reina_day_t &dp, uint32_t hist_slot, int weekly_elsewhere,
                                               uint32_t W, unsigned char *lds) {
    const CAS DevParams *P = (const CAS DevParams *)mref_.P;
    const GBuffers B = global_buffers(mref_.B);  // by value: pointers live in SGPRs, never re-read after stores
    // (dp itself stays untouched: writing a field of the by-value kernel argument would spill the whole struct)
    int32_t *const history_row =
        mref_.history_base ? mref_.history_base + (size_t)hist_slot * REINA_COUNTER_WORDS : dp.history_row;
    OpenImportsLds &OL = *reinterpret_cast<OpenImportsLds *>(lds);
    uint8_t *placed = OL.placed;
    uint32_t &s_unplaced = OL.s_unplaced, &s_import_base = OL.s_import_base;
    int32_t *new_by_age = OL.new_by_age, *new_by_variant = OL.new_by_variant, *s_age_start = OL.s_age_start;
    const int tid = threadIdx.x;
    DIAG_CLOCK(OPEN, ps_t);
    if (tid <= REINA_MAX_AGES) s_age_start[tid] = P->age_start[tid];
    if (tid < REINA_MAX_AGES) new_by_age[tid] = 0;
    if (tid < REINA_MAX_VARIANTS) new_by_variant[tid] = 0;
    // (the scalars thread 0 rewrites below are requested now, beside the snapshot loads)
    int32_t pre_beds = 0, pre_abeds = 0, pre_icu = 0, pre_aicu = 0, pre_qlen = 0;
    if (tid == 0) {
        pre_beds = B.counters[SC_IDX(REINA_S_BEDS)];
        pre_abeds = B.counters[SC_IDX(REINA_S_AVAILABLE_BEDS)];
        pre_icu = B.counters[SC_IDX(REINA_S_ICU_UNITS)];
        pre_aicu = B.counters[SC_IDX(REINA_S_AVAILABLE_ICU)];
        pre_qlen = B.control[(dp.day & 1) ? REINA_L_QUEUE1 : REINA_L_QUEUE0];
    }
    // generate_state() is taken BEFORE iterate() (calc/simulation.py:195 vs :270)
    if (history_row)
        for (int k = tid; k < REINA_COUNTER_WORDS; k += PRO_THREADS) history_row[k] = B.counters[k];
    __syncthreads();
    if (tid == 0) {
        s_import_base = 0;
        B.counters[SC_IDX(REINA_S_DAY)] = (int32_t)dp.day + 1;
        B.counters[SC_IDX(REINA_S_BEDS)] = pre_beds + dp.add_beds;
        B.counters[SC_IDX(REINA_S_AVAILABLE_BEDS)] = pre_abeds + dp.add_beds;
        B.counters[SC_IDX(REINA_S_ICU_UNITS)] = pre_icu + dp.add_icu_units;
        B.counters[SC_IDX(REINA_S_AVAILABLE_ICU)] = pre_aicu + dp.add_icu_units;
    }
    __syncthreads();
    if (dp.n_import_batches) import_classes_load(P, s_age_start, &OL.classes);   // (a day without imports does not pay for it)
    // (W > 1: the day's imports are shared with W - 1 helper workgroups, import_helper_block below)
    uint32_t phase = 0;
    pro_imports(P, B, dp, 1, &s_import_base, placed, &s_unplaced, new_by_age, new_by_variant, s_age_start, &OL.classes, phase, false, 0, W);
    // Population.init_day (main.pyx:1687-1699) + Context._iterate zeroing (:1998-2000)
    __syncthreads();
    for (int k = tid; k < (int)P->nr_ages; k += PRO_THREADS) {
        B.counters[CNT_IDX(REINA_C_NEW_INFECTIONS, k)] = 0;
        B.counters[CNT_IDX(REINA_C_DETECTED, k)] = 0;
    }
    for (int k = tid; k < REINA_PRESSURE_WORDS; k += PRO_THREADS) B.pressure[k] = 0;
    if (P->n_shards > 1)   // ... and the table of the shards' bed / ICU event maps behind it (every shard fills its own segment)
        for (uint32_t k = tid; k < P->n_shards * 2u * P->hosp_ranges; k += PRO_THREADS) B.pressure[REINA_PRESSURE_WORDS + k] = 0;
    for (uint32_t k = tid; k < P->hosp_ranges; k += PRO_THREADS) {   // the day's event buckets are empty, no walker has published
        hosp_counts(B)[k] = 0;
        B.hosp_events[HOSP_AGG_OFF(P->hosp_ranges) + k] = 0ull;
    }
    if (tid < REINA_NR_PLACES) B.counters[SC_IDX(REINA_S_DAILY_CONTACTS + tid)] = 0;
    if (tid < REINA_MAX_VARIANTS) B.counters[SC_IDX(REINA_S_INFECTED_BY_VARIANT + tid)] = 0;
    if (tid == 0) {
        B.counters[SC_IDX(REINA_S_TOTAL_INFECTORS)] = 0;
        B.counters[SC_IDX(REINA_S_TOTAL_INFECTIONS)] = 0;
        B.counters[SC_IDX(REINA_S_EXPOSED_PER_DAY)] = 0;
        B.control[REINA_L_WORK] = 0;
        B.control[REINA_L_CAND] = 0;
        B.control[REINA_L_CAND_OVF] = 0;
        B.control[REINA_L_HOSP] = 0;
        B.control[REINA_L_CONTACTS] = 0;
        B.control[REINA_L_ACTIVE + (dp.day & 1u)] = 0;   // (k_day counts today's into it and reads yesterday's)
        B.control[REINA_L_HOSP_ADMIT] = 0;
        B.control[REINA_L_ICU_ADMIT] = 0;
        // what decides tonight whether the ORDER of the bed / ICU events matters (hosp_day_is_ordered)
        B.control[REINA_L_BEDS_OPEN] = pre_abeds + dp.add_beds;
        B.control[REINA_L_ICU_OPEN] = pre_aicu + dp.add_icu_units;
        B.control[REINA_L_EV_HOSPITALIZE] = 0;
        B.control[REINA_L_EV_TO_ICU] = 0;
        B.control[REINA_L_WALK_TICKET] = 0;
        B.control[REINA_L_SORT_TICKET] = 0;
        // HealthcareSystem.iterate: ct_cases_per_day = len(queue) (main.pyx:518-519)
        B.counters[SC_IDX(REINA_S_CT_CASES_PER_DAY)] = pre_qlen;
    }
    // the day is open: the test-queue workgroups of the same launch (k_open) may start; what follows
    // (weekly imports) only touches never-infected agents and the infection counters
    __syncthreads();   // workgroup-scope release: every thread's stores have reached L2; then ONE agent-scope release
    if (tid == 0 && P->n_shards > 1) {
        // a sharded population's free capacity at day open travels with the day's pressure all-reduce (the demand
        // words beside it are added by k_day); every shard then takes its share of the pool (k_remote)
        B.pressure[REINA_PRESSURE_FREE_BEDS(P->shard_rank)] = pre_abeds + dp.add_beds;
        B.pressure[REINA_PRESSURE_FREE_ICU(P->shard_rank)] = pre_aicu + dp.add_icu_units;
    }
    if (tid == 0) __hip_atomic_store(&B.control[REINA_L_DAY_OPEN], (int32_t)dp.day + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    DIAG_SINCE(OPEN, DIAG_OPEN_UNTIL_FLAG, DIAG_THREAD0, ps_t, B.mirror);
    // weekly imports (Population.infect_people_daily, main.pyx:1671-1685) run after init_day's
    // zeroing; vaccination follows the test-queue pass in the reference (main.pyx:547-558) and is
    // launched from k_vaccinate after both.
    __syncthreads();
    if (!weekly_elsewhere)
        pro_imports(P, B, dp, 0, &s_import_base, placed, &s_unplaced, new_by_age, new_by_variant, s_age_start, &OL.classes, phase, false, 0, W);
    DIAG_SINCE(OPEN, DIAG_OPEN_TOTAL, DIAG_THREAD0, ps_t, B.mirror);
}

// The weekly imports in a workgroup of their own (days without intervention imports, whose claim
// keys they would share): agents are drawn, claimed and infected from the first instruction of the
// launch; only the counter updates wait for the opening workgroup's daily zeroing.
// `with_opening`: this workgroup is helper r (1..W-1) of the opening workgroup on a day with intervention imports: it takes
// its share of them, and of the weekly imports behind them, in step with the opening workgroup -- whose snapshot precedes
// its first arrival at imports_any, and whose daily zeroing lies between the two batches, so no counter is touched early.
__device__ __forceinline__ void weekly_imports_block(const MemberRef &mref_, const reina_day_t &dp, unsigned char *lds, uint32_t r, uint32_t W,
                                                     bool with_opening = false) {
    const CAS DevParams *P = (const CAS DevParams *)mref_.P;
    const GBuffers B = global_buffers(mref_.B);
    OpenImportsLds &OL = *reinterpret_cast<OpenImportsLds *>(lds);
    uint8_t *placed = OL.placed;
    uint32_t &s_unplaced = OL.s_unplaced, &s_import_base = OL.s_import_base;
    int32_t *new_by_age = OL.new_by_age, *new_by_variant = OL.new_by_variant, *s_age_start = OL.s_age_start;
    const int tid = threadIdx.x;
    if (tid <= REINA_MAX_AGES) s_age_start[tid] = P->age_start[tid];
    if (tid < REINA_MAX_AGES) new_by_age[tid] = 0;
    if (tid < REINA_MAX_VARIANTS) new_by_variant[tid] = 0;
    if (tid == 0) s_import_base = 0;
    __syncthreads();
    DIAG_CLOCK(OPEN, ws_t);
    import_classes_load(P, s_age_start, &OL.classes);
    uint32_t phase = 0;
    if (with_opening) pro_imports(P, B, dp, 1, &s_import_base, placed, &s_unplaced, new_by_age, new_by_variant, s_age_start, &OL.classes, phase, false, r, W);
    pro_imports(P, B, dp, 0, &s_import_base, placed, &s_unplaced, new_by_age, new_by_variant, s_age_start, &OL.classes, phase, !with_opening, r, W);
    DIAG_SINCE(OPEN, DIAG_OPEN_WEEKLY, DIAG_THREAD0, ws_t, B.mirror, r == 0);
}

// ... and in k_day's launch (`deferred`, above): workgroup r of the W that follow the streaming workgroups
__device__ __forceinline__ void day_imports_block(const MemberRef &mref_, const reina_day_t &dp, unsigned char *lds, uint32_t r, uint32_t W) {
    const CAS DevParams *P = (const CAS DevParams *)mref_.P;
    const GBuffers B = global_buffers(mref_.B);
    OpenImportsLds &OL = *reinterpret_cast<OpenImportsLds *>(lds);
    const int tid = threadIdx.x;
    if (tid <= REINA_MAX_AGES) OL.s_age_start[tid] = P->age_start[tid];
    if (tid == 0) OL.s_import_base = 0;
    __syncthreads();
    import_classes_load(P, OL.s_age_start, &OL.classes);
    uint32_t phase = 0;
    pro_imports(P, B, dp, 0, &OL.s_import_base, OL.placed, &OL.s_unplaced, OL.new_by_age, OL.new_by_variant, OL.s_age_start, &OL.classes,
                phase, false, r, W, true);
}

// `seq`: the launch's sequence number (per engine, never 0): the tag of the words the chained workgroups publish
DAY_KERNEL __launch_bounds__(PRO_THREADS) void k_vaccinate(const MemberRef *M_, MemberRef one_, reina_day_t dp, uint32_t seq, VaccGeom geo) {
    MEMBER_OF_LAUNCH;
    const CAS DevParams *P = (const CAS DevParams *)mref_.P;
    const GBuffers B = global_buffers(mref_.B);  // by value: pointers live in SGPRs, never re-read after stores
    __shared__ VaccLds S;
    if (gridDim.x > 1) pro_vaccinate_chain(P, B, dp, S, blockIdx.x, gridDim.x, seq, geo);
    else pro_vaccinate(P, B, dp, S);
}
