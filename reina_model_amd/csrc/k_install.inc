// reina_hip.hip part: k_install: winners, symptom onsets, bookkeeping; k_upload.
// Included by reina_hip.hip only (one translation unit); not a standalone header.
// ---------------------------------------------------------------------------------------------
// install_block: the day's four kinds of deferred work, dealt to the launch's waves in UNITS:
//   IL_CAND  the winning exposure attempts: the attempt whose source holds the smallest (priority, id) key per target wins
//            (the reference: first source in rotated scan order, main.pyx:1982-1992) and infects it (person_infect :209-235)
//   IL_ILL   symptom onsets (person_become_ill :284-291)
//   IL_BOOK  R statistics (:1969-1972), recoveries / deaths at home (Population.recover / die :1584-1623)
//   IL_EV    the bed / ICU events of a day on which nothing can run out (every request granted, any order)
// Lists 0-2 live in per-scanning-wave slices (counts in buffers.work_counts), the events in the day's priority buckets: a
// unit is G consecutive slices (buckets) of one list, G = 8 on a quiet day (a slice holds a handful of records: eight are
// concatenated so that the 64 lanes are filled) down to 1 at an epidemic peak (hundreds of records a slice).  Every wave
// gets units of every list in turn: whatever the mix of the day, the waves finish together.
// (Round 2 split the workgroups statically in two roles, this round first in four: at the 10^8-agent peak the candidate
// workgroups then ran 170 us beside event workgroups with nothing to do -- the sum of all work was 64 us per workgroup.)
// `events`: the IL_EV list is part of the work (a day on which order does not matter); `only_events`: nothing else is
// (workgroup 0 of a small population's launch, beside the installs).
enum { IL_CAND = 0, IL_ILL, IL_BOOK, IL_EV };
// (diagnostic builds: -DREINA_NO_BYBIT installs winners by compare-and-swap on the hot word as rounds 1-4 did)
#ifdef REINA_NO_BYBIT
#define INSTALL_BY_BIT false
#else
#define INSTALL_BY_BIT true
#endif

// the unit's G counts and bases; returns the records it holds
__device__ __forceinline__ uint32_t install_unit_counts(const CAS DevParams *P, const GBuffers &B, int list, uint32_t first, uint32_t G, uint32_t limit,
                                                        uint32_t scan_waves, uint32_t scan_tiles, uint32_t (&c_n)[8], uint32_t (&base)[8]) {
    uint32_t tot = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const uint32_t idx = first + (uint32_t)k;
        const bool in = (uint32_t)k < G && idx < limit;
        uint32_t n = 0;
        if (in) {
            if (list == IL_EV) {
                n = hosp_counts(B)[idx];
                if (n > P->hosp_bucket_cap) n = P->hosp_bucket_cap;
            } else {
                n = B.work_counts[(list == IL_CAND ? LIST_CAND : list == IL_ILL ? LIST_ILL : LIST_BOOK) * REINA_MAX_SCAN_WAVES + idx];
            }
        }
        c_n[k] = n;
        base[k] = list == IL_EV ? (in ? idx * P->hosp_bucket_cap : 0u) : scan_slice_base(in ? idx : 0u, scan_waves, scan_tiles);
        tot += n;
    }
    return tot;
}
// record j of the unit's concatenation -> its position in the list's array
__device__ __forceinline__ uint32_t install_unit_pos(uint32_t j, const uint32_t (&c_n)[8], const uint32_t (&base)[8]) {
    uint32_t bsel = base[0];
    bool done = false;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        if (!done) {
            if (j < c_n[k]) {
                bsel = base[k];
                done = true;
            } else {
                j -= c_n[k];
            }
        }
    }
    return bsel + j;
}

template <bool X>
__device__ __forceinline__ void install_block(const MemberRef &mref_, const reina_day_t &dp, uint32_t scan_waves, uint32_t scan_tiles,
                                              uint32_t bx, uint32_t nbx, bool events, bool only_events, int32_t (*s_hl)[REINA_MAX_AGES],
                                              OnsetStage *stage) {
    const ParamsX<X> P{(const CAS DevParams *)mref_.P};
    const GBuffers B = global_buffers(mref_.B);  // by value: pointers live in SGPRs, never re-read after stores
    __shared__ int32_t new_by_age[REINA_MAX_AGES];
    __shared__ int32_t new_by_variant[REINA_MAX_VARIANTS];
    __shared__ int32_t s_age_start[REINA_MAX_AGES + 1];
    __shared__ int32_t s_cnt[SL_NR][REINA_MAX_AGES];
    __shared__ int32_t s_infectors, s_infections;
    __shared__ int32_t s_dbeds, s_dicu;               // (s_hl: the events' per-age counter changes)
    for (int k = threadIdx.x; k < HL_NR * REINA_MAX_AGES; k += blockDim.x) (&s_hl[0][0])[k] = 0;
    if (threadIdx.x == 0) s_dbeds = s_dicu = 0;
    for (int k = threadIdx.x; k <= REINA_MAX_AGES; k += blockDim.x) s_age_start[k] = P->age_start[k];
    for (int k = threadIdx.x; k < SL_NR * REINA_MAX_AGES; k += blockDim.x) (&s_cnt[0][0])[k] = 0;
    if (threadIdx.x == 0) {
        s_infectors = 0;
        s_infections = 0;
    }
    if (threadIdx.x < REINA_MAX_AGES) new_by_age[threadIdx.x] = 0;
    if (threadIdx.x < REINA_MAX_VARIANTS) new_by_variant[threadIdx.x] = 0;
    if (threadIdx.x == 0 && stage) stage->n = 0;
    DIAG_CLOCK(INSTALL, is_t);   // (-DREINA_INSTALL_STAMPS: the phases of the two roles, each under its own names)
#define INSTALL_LAP(ph) do { if (only_events) DIAG_LAP(INSTALL, DIAG_INSTALL_EVENTS_##ph, DIAG_BARRIER_THREAD0, is_t, B.mirror); \
                             else DIAG_LAP(INSTALL, DIAG_INSTALL_MAIN_##ph, DIAG_BARRIER_THREAD0, is_t, B.mirror); } while (0)
    __syncthreads();
    INSTALL_LAP(SETUP);
    const GAS uint4 *cand = reinterpret_cast<const GAS uint4 *>(B.candidates);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t cap = P->max_work_items;
    const GAS uint2 *l_ill = reinterpret_cast<const GAS uint2 *>(B.work_items) + cap;
    const GAS uint2 *l_book = reinterpret_cast<const GAS uint2 *>(B.scan_lists) + cap;
    // (candidates realised from cross-shard pressure (k_remote), indexed above the slice regions, and the shared overflow
    // list -- records that did not fit their wave's region, and the day's weekly imports -- are flat arrays: dealt out below
    // as units of 64 records behind the lists' units, so that they lengthen nobody's chain of dependent round trips)
    const int C_remote = (!only_events && P->n_shards > 1) ? B.control[REINA_L_CAND] : 0;
    int C_ovf = only_events ? 0 : B.control[REINA_L_CAND_OVF];
    if (C_ovf > (int)P->cand_ovf_cap) C_ovf = (int)P->cand_ovf_cap;
    // (Measured dead end, round 3: a wave's first unit GUESSED under the quiet-day geometry, G = 8, and its counts requested
    // beside the control words that decide G -- one round trip instead of two on the chain of a quiet day: the launch became
    // 1.3-1.7 us SLOWER at every size, with or without the wave number forced into scalar registers, with the control loads
    // issued first or last.  Not understood; the straight-line code in front of a launch's first useful load has a price.)
    // the units: slices (buckets) in groups of G, G from the day's contact count (one contact in eight or so leaves a record
    // in some list): 8 on a quiet day, 1 when a slice holds more than a wave's worth of records
    const uint32_t R = P->hosp_ranges;
    uint32_t G = 8u;
    {
        const uint32_t per_slice = (uint32_t)B.control[REINA_L_CONTACTS] / (8u * (scan_waves ? scan_waves : 1u));
        if (per_slice >= 48u) G = 1u; else if (per_slice >= 24u) G = 2u; else if (per_slice >= 12u) G = 4u;
    }
    const uint32_t n_l = only_events ? 0u : (scan_waves + G - 1u) / G;   // units per list
    const uint32_t n_ev = events ? (R + G - 1u) / G : 0u;                // units of the event buckets
    const uint32_t n_ovf = ((uint32_t)C_ovf + 63u) / 64u, n_rem = ((uint32_t)C_remote + 63u) / 64u;   // units of the flat lists
    const uint32_t total = 3u * n_l + n_ev + n_ovf + n_rem;
    // Wave w of the W waves takes the units w, w + W, w + 2 W, ... of the sequence (group 0: candidates, onsets, bookkeeping),
    // (group 1: ...), ..., then the event units -- with the three lists of a group ROTATED from one pass to the next, so
    // that every wave meets every kind of work whatever W is: no role has idle waves while another is still busy, and
    // no ticket counter (a returning atomic on ONE address per unit: 4700 of them serialised to 50 us of a quiet day at
    // 10^8 agents when that was tried).
    const uint32_t W = (nbx * blockDim.x) >> 6, wave_g = (bx * blockDim.x + threadIdx.x) >> 6;
    // (unit u = 3 g + r of group g: list r -- a wave's units w, w + W, ... then change lists by themselves unless 3 | W; in
    // that case no group straddles two passes and the lists of pass k are rotated by k: either way every (group, list)
    // pair is exactly one unit)
    const bool rotate = (W % 3u) == 0u;
    uint32_t pass = 0;
    for (uint32_t u = wave_g; u < total; u += W, pass++) {
        int list;
        uint32_t first;
        if (u < 3u * n_l) {
            list = (int)((u % 3u + (rotate ? pass : 0u)) % 3u);
            first = (u / 3u) * G;
        } else if (u < 3u * n_l + n_ev) {
            list = IL_EV;
            first = (u - 3u * n_l) * G;
        } else {
            // 64 records of a flat candidate list: the overflow list (weekly imports among them), then the cross-shard one
            const uint32_t f = u - 3u * n_l - n_ev;
            const bool ovf = f < n_ovf;
            const uint32_t k = (ovf ? f : f - n_ovf) * 64u + lane;
            if (k < (uint32_t)(ovf ? C_ovf : C_remote)) {
                const uint4 cd = gld(&cand[(ovf ? P->cand_ovf_base : P->max_work_items) + k]);
                if (cd.x != 0xFFFFFFFFu) {   // (a cross-shard attempt that did not get through leaves a hole)
                    const uint64_t cl = ld_claim(&B.cold[cd.x].claim);
                    const int32_t vd = B.cold[cd.x].vacc_day;
                    const uint32_t w = ld_hot(&B.hot[cd.x]);
                    if (cd.z & IMPORT_RECORD_FLAG) {
                        // a weekly import placed beside the stream (k_open.inc: pro_imports, deferred): it holds its target's
                        // claim under tomorrow's day tag, which no contact of today can beat; installed like any import -- no
                        // infector, the testing mode of its batch
                        if (cl == rp_order_key(dp.day + 1u, 0xFFFFFu, cd.y) && RH_STATE(w) == RS_SUSCEPTIBLE)
                            install_infection(P, B, s_age_start, cd.x, w, dp.day, cd.z & 0xFFu, -1, 1, (cd.z >> 24) & 3u, new_by_age, new_by_variant, 0u, vd);
                    } else if (cl == rp_order_key(dp.day, cd.w, cd.y) && RH_STATE(w) == RS_SUSCEPTIBLE) {
                        const int32_t src = (cd.y & RP_REMOTE_SRC) ? -1 : (int32_t)cd.y;
                        install_infection(P, B, s_age_start, cd.x, w, dp.day, cd.z & 0xFFu, src, 0, dp.testing_mode, new_by_age, new_by_variant, (cd.z >> 8) & 1u, vd, false, INSTALL_BY_BIT);
                    }
                }
            }
            continue;
        }
        uint32_t c_n[8], base[8];
        const uint32_t tot = install_unit_counts(P, B, list, first, G, list == IL_EV ? R : scan_waves, scan_waves, scan_tiles, c_n, base);
        if (list == IL_CAND) {
            // per-slice candidate regions written by k_day, 64 records per step
            for (uint32_t j0 = 0; j0 < tot; j0 += 64u) {
                const uint32_t j = j0 + lane;
                if (j >= tot) continue;
                const uint4 cd = gld(&cand[install_unit_pos(j, c_n, base)]);
                // the target's record (claim, vaccination day) and word are requested together (the candidate says whether the
                // source keeps an infectee list: nothing of the source is read, so the bed / ICU walk may rewrite its word meanwhile)
                const uint64_t cl = ld_claim(&B.cold[cd.x].claim);
                const int32_t vd = B.cold[cd.x].vacc_day;
                if (cl != rp_order_key(dp.day, cd.w, cd.y)) continue;
                // The target's hot word is not read (round 4: one scattered access less per record): a contact claims only
                // never-infected agents (k_contacts.inc), and all a never-infected agent's word can hold is the VACCINATED
                // flag, which its record's vaccination day tells -- it was never detected, queued or counted (testing and
                // tracing reach infected people only: seek_testing main.pyx:595-615, perform_contact_tracing :495-512).  The
                // winner is installed once: its bit of the infected plane is the claim (install_infection: by_bit), a duplicate
                // record of the same winner (two contacts of one source with one target) finds it set.
                const uint32_t w = vd >= 0 ? RH_VACCINATED : 0u;
                install_infection(P, B, s_age_start, cd.x, w, dp.day, cd.z & 0xFFu, (int32_t)cd.y, 0, dp.testing_mode, new_by_age, new_by_variant,
                                  (cd.z >> 8) & 1u, vd, false, INSTALL_BY_BIT);
            }
        } else if (list == IL_ILL) {
            // symptom onsets (person_become_ill)
            for (uint32_t j0 = 0; j0 < tot; j0 += 64u) {
                const uint32_t j = j0 + lane;
                uint2 r = make_uint2(0, 0);
                if (j < tot) r = gld(&l_ill[install_unit_pos(j, c_n, base)]);
                become_ill(P, B, dp, j < tot, r.x, r.y, stage);
            }
        } else if (list == IL_BOOK) {
            // bookkeeping: R statistics (main.pyx:1969-1972) and the per-age counters of agents who
            // recovered or died at home today (Population.recover / die, main.pyx:1584-1623)
            for (uint32_t j0 = 0; j0 < tot; j0 += 64u) {
                const uint32_t j = j0 + lane;
                int ni = 0, cr = 0;
                if (j < tot) {
                    const uint2 r = gld(&l_book[install_unit_pos(j, c_n, base)]);
                    if (r.y == EVX_COUNT_R) {
                        cr = 1;
                        ni = B.cold[r.x].n_infected;
                    } else {
                        const int age = age_of(s_age_start, r.x, 0, (int)P->nr_ages - 1);
                        atomicAdd(&s_cnt[SL_INFECTED][age], -1);
                        if (r.y == EVX_RECOVERED_HOME) {
                            atomicAdd(&s_cnt[SL_RECOVERED][age], 1);
                        } else {
                            atomicAdd(&s_cnt[SL_DEAD][age], 1);
                            atomicAdd(&s_cnt[SL_NHD][age], 1);
                        }
                    }
                }
                const int tc = wave_sum(cr), tn = wave_sum(ni);
                if (lane == 0 && tc) {
                    atomicAdd(&s_infectors, tc);
                    if (tn) atomicAdd(&s_infections, tn);
                }
            }
        } else {
            // bed / ICU events of a day on which nothing can run out: all granted, any order
            const GAS uint64_t *keys = B.hosp_events + HOSP_KEYS_OFF(R);
            for (uint32_t j0 = 0; j0 < tot; j0 += 64u) {
                const uint32_t j = j0 + lane;
                int db = 0, dc = 0;
                if (j < tot) {
                    const uint64_t key = keys[install_unit_pos(j, c_n, base)];
                    const uint32_t i = (uint32_t)((key >> 2) & 0xFFFFFFFFu);
                    const uint32_t w = B.hot[i];
                    const float od = B.cold[i].onset_days;
                    const int type = (int)(key & 3u);
                    if (type == EV_HOSPITALIZE) db = -1;
                    else if (type == EV_TO_ICU) { db = 1; dc = -1; }
                    else if (type == EV_RELEASE_WARD) db = 1;
                    else dc = 1;
                    B.hot[i] = hosp_apply(P, B, dp, s_age_start, s_hl, type, i, w, od, true);
                }
                const int tb = wave_sum(db), tc = wave_sum(dc);
                if (lane == 0) {
                    if (tb) atomicAdd(&s_dbeds, tb);
                    if (tc) atomicAdd(&s_dicu, tc);
                }
            }
        }
    }
    if (stage && !only_events) onset_stage_flush(P, B, stage, (dp.day & 1) ^ 1);   // the workgroup's appends to tomorrow's test queue
    INSTALL_LAP(WORK);
    // tomorrow's mirror-table sizes: about twice this shard's share of today's cross-shard attempts of
    // the cell (buffers.pressure holds the sums over all shards by now), a power of two in [8, mirror_slots]
    if (P->n_shards > 1 && !IS_EXACT(P) && !only_events && bx == 0 && threadIdx.x < REINA_MIRROR_CELLS) {
        uint32_t tot = 0;
        for (uint32_t dest = 0; dest < P->n_shards; dest++) {
            const int n = B.pressure[dest * REINA_MIRROR_CELLS + threadIdx.x];
            tot += n > 0 ? (uint32_t)n : 0u;
        }
        const uint32_t want = 2u * ((tot + P->n_shards - 1) / P->n_shards);
        uint32_t eff = P->mirror_slots < RP_MIRROR_MIN_SLOTS ? P->mirror_slots : RP_MIRROR_MIN_SLOTS;
        while (eff < want && eff < P->mirror_slots) eff <<= 1;
        B.mirror_meta[threadIdx.x] = eff;
    }
    // The workgroup's histograms go to the global counters ONE row at a time: an atomic instruction occupies every L2 line it touches
    // for some 12 ns, whoever else wants the line (tools/ubench_atomics.hip), and the infected / recovered / dead rows are changed
    // by the installs, by the bookkeeping AND by the events -- folded into the events' histogram first, a row of 32 ages sees one
    // instruction per workgroup instead of up to three (256 workgroups: 3 us of that line instead of 9, at the end of every launch).
    __syncthreads();
    if (threadIdx.x < REINA_MAX_AGES) {
        const int k = (int)threadIdx.x;
        s_hl[HL_INFECTED][k] += new_by_age[k] + s_cnt[SL_INFECTED][k];
        s_hl[HL_RECOVERED][k] += s_cnt[SL_RECOVERED][k];
        s_hl[HL_DEAD][k] += s_cnt[SL_DEAD][k];
        s_hl[HL_NHD][k] += s_cnt[SL_NHD][k];
    }
    flush_new_infections(B, new_by_age, new_by_variant, (int)blockDim.x, false);   // (begins and ends with a barrier)
    hosp_flush_counts(B, s_hl, (int)blockDim.x);
    if (events && threadIdx.x == 0) {
        if (s_dbeds) atomicAdd(&B.counters[SC_IDX(REINA_S_AVAILABLE_BEDS)], s_dbeds);
        if (s_dicu) atomicAdd(&B.counters[SC_IDX(REINA_S_AVAILABLE_ICU)], s_dicu);
    }
    if (only_events) return;
    if (bx == 0 && threadIdx.x < REINA_MAX_AGES) {
        // the day's detections from the test queue (side block filled by the day's opening launch): into the counters
        const int32_t v = B.control[REINA_L_DET_SIDE + threadIdx.x];
        if (v) {
            atomicAdd(&B.counters[CNT_IDX(REINA_C_DETECTED, threadIdx.x)], v);
            atomicAdd(&B.counters[CNT_IDX(REINA_C_ALL_DETECTED, threadIdx.x)], v);
            B.control[REINA_L_DET_SIDE + threadIdx.x] = 0;
        }
    }
    if (threadIdx.x == 0) {
        if (s_infectors) atomicAdd(&B.counters[SC_IDX(REINA_S_TOTAL_INFECTORS)], s_infectors);
        if (s_infections) atomicAdd(&B.counters[SC_IDX(REINA_S_TOTAL_INFECTIONS)], s_infections);
        // today's test queue has been processed (k_test_*): empty it for the day after tomorrow
        if (bx == 0) {
            B.control[(dp.day & 1) ? REINA_L_QUEUE1 : REINA_L_QUEUE0] = 0;
            B.control[REINA_L_LEVEL1] = 0;   // consumed by the level-1 pass; tomorrow's level-0 pass appends from its first instruction
            B.control[REINA_L_TRACE_DONE] = 0;   // (the tracing workgroups' arrival counter of the day's opening)
            for (int q = 0; q < 4; q++) B.control[REINA_L_IMPORT_SYNC + q] = 0;   // (and the arrival words of its import workgroups)
        }
    }
    INSTALL_LAP(FLUSH);
#undef INSTALL_LAP
}

// ---------------------------------------------------------------------------------------------
// k_hosp_install: the day's last launch (of a small unsharded population; a large one adds k_hosp_sort / k_hosp_walk).
// The bed / ICU events and the installation of the day's infections are independent -- the events rewrite hot words
// of agents leaving ILLNESS / HOSPITALIZED / IN_ICU and the bed counters; the installs turn never-infected agents
// into INCUBATION, the deferred onsets INCUBATION into ILLNESS, and nothing of an infection's SOURCE is read (its
// record carries what is needed) -- so they share one launch.  On a day on which no bed or ICU unit can run out
// (hosp_day_is_ordered) the events are applied in any order by the deferred-list workgroups; otherwise one
// workgroup walks them in priority order (HI_HOSP_WG: workgroup 0, small populations) or the two launches
// that follow do.  (A sharded population runs the same launches behind k_remote, which also takes the shard's
// demand-proportional share of the pooled free beds / ICU units: the walk starts from that.)
static_assert(HOSP_THREADS == 1024, "fused launch");
// `n_walk`: the launch's first n_walk workgroups are the walkers of a large population's ordered day (k_hospital.inc:
// hosp_walker_block); on any other day they install with the others.  Dynamic LDS: REINA_MAX_HOSP_EVENTS keys (HI_HOSP_WG) or
// HOSP_P_THREADS * HOSP_P_E keys (n_walk > 0) for the event walks; the installing workgroups stage their test-queue
// appends in its first sizeof(OnsetStage) bytes.
static_assert(sizeof(OnsetStage) <= (size_t)HOSP_THREADS * 4 * 8, "the stage fits the dynamic LDS of either launch shape");
DAY_KERNEL __launch_bounds__(HOSP_THREADS) void k_hosp_install(const MemberRef *M_, MemberRef one_, reina_day_t dp, uint32_t scan_waves,
                                                               uint32_t scan_tiles, int flags, uint32_t n_walk) {
    MEMBER_OF_LAUNCH;
    __shared__ int32_t s_hl[HL_NR][REINA_MAX_AGES];   // per-age counter changes of the bed / ICU events (either path)
    __shared__ SatFn s_f[2][HOSP_THREADS];            // the ordered walks' scan of saturating maps
    extern __shared__ __align__(16) unsigned char smem_hi[];
    const bool ordered = hosp_day_is_ordered(global_buffers(mref_.B));
    uint32_t bx = blockIdx.x, nbx = gridDim.x;
    if (n_walk && ordered) {
        if (bx < n_walk) {
            hosp_walker_block(mref_, dp, s_hl, reinterpret_cast<uint64_t *>(smem_hi), s_f,
                              ((const CAS DevParams *)mref_.P)->n_shards > 1 ? WALK_SHARDED : WALK_LOCAL);
            return;
        }
        bx -= n_walk;
        nbx -= n_walk;
    }
    // (on any other day the walkers' workgroups install with the others -- every workgroup of the launch reads the same
    // control words, so all agree on the number of installing waves: until round 4 they left at once and a quarter of the
    // chip, R / 16 = 64 of 256 CUs at 10^8 agents, stood idle through the installs of every day on which nothing ran out)
    if (flags & HI_HOSP_WG) {
        if (bx == 0 && ordered) {
            DIAG_CLOCK(HOSP, hb_t);
            hospital_block(mref_, dp, s_hl, s_f);
            DIAG_SINCE(HOSP, DIAG_HOSP_BLOCK, DIAG_BARRIER_THREAD0, hb_t, mref_.B.mirror);
            return;
        }
        if (flags & HI_INSTALL) {
            // workgroup 0 is set aside for the events: on a day on which order does not matter it applies them on its
            // own, beside the installs (a small population: a few dozen events)
            if (bx == 0) {
                if (flags & HI_EVENTS) install_block<EXACT>(mref_, dp, scan_waves, scan_tiles, 0, 1, true, true, s_hl, nullptr);
                return;
            }
            bx--;
            nbx--;
            flags &= ~HI_EVENTS;
        }
    }
    const bool events = (flags & HI_EVENTS) && !ordered;
    if (flags & HI_INSTALL)
        install_block<EXACT>(mref_, dp, scan_waves, scan_tiles, bx, nbx, events, false, s_hl, reinterpret_cast<OnsetStage *>(smem_hi));
    else if (events)
        install_block<EXACT>(mref_, dp, scan_waves, scan_tiles, bx, nbx, true, true, s_hl, nullptr);
}

// table upload: two word copies out of a pinned host buffer (see reina_upload_contact_tables)
// (the tables travel as the segments in use -- the rows of the distinct contact and count rows, not the arrays sized for 128
// of each: 55 KB instead of 288 KB over PCIe in front of the day that needs them)
struct UploadSegs {
    uint32_t n;
    uint32_t off[8], words[8];   // word offsets into the Tables image, source and destination alike
};
__global__ __launch_bounds__(256) void k_upload(uint32_t *d0, const uint32_t *s0, uint32_t n0, uint32_t *d1, const uint32_t *s1, UploadSegs segs) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n0; k += stride) d0[k] = s0[k];
    for (uint32_t q = 0; q < segs.n; q++)
        for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < segs.words[q]; k += stride) d1[segs.off[q] + k] = s1[segs.off[q] + k];
}

// the end of a run: the history rows and the counter block written straight into the caller's page-locked block (reina_read_history).
// (Two hipMemcpyAsync took the copy engine's set-up twice: 46 us for 150 KB behind a run of twenty HUS days that takes 790.)
__global__ __launch_bounds__(256) void k_export(const uint4 *hist, uint32_t n_hist4, const uint4 *counters, uint32_t n_cnt4, uint4 *out) {
    const uint32_t stride = gridDim.x * blockDim.x, n = n_hist4 + n_cnt4;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) out[k] = k < n_hist4 ? hist[k] : counters[k - n_hist4];
}
