// reina_hip.hip part: the streaming recorder over all hot words (the scan half of k_day).
// Included by reina_hip.hip only (one translation unit); not a standalone header.
// ---------------------------------------------------------------------------------------------
// Context._process_person + person_advance for every agent (main.pyx:1968-1992,395-438)
//
// Streaming: each lane loads 16 B (4 hot words) per 1-KiB wave load, two loads in flight per wave; a
// per-lane need-mask picks the words that are infected or removed-but-uncounted (everything else costs
// three integer ops).  The integer part of the state machine (countdown, recover / die at home, R
// marking) runs in place and changed words are stored back where they were loaded.  Everything that
// needs random numbers, gathers or counters is only RECORDED, as (agent, word|kind) pairs appended with
// wave ballots -- no atomics:
//   exposure candidates  -> the wave's own LDS strip; worked off 64 at a time by the same wave (k_day:
//                           contact COUNT draw, then the contacts themselves), never written to memory
//   symptom onsets       -> per-wave slice in HBM -> k_hosp_install (gamma draw of the illness course, testing decision)
//   hospital events      -> the day's priority buckets in HBM (k_hospital.inc) -> k_hosp_install / k_hosp_sort + k_hosp_walk
//   bookkeeping          -> per-wave slice in HBM -> k_hosp_install (R statistics, recovered / died-at-home counters)
#define DAY_EV_STAGE 1024   // bed / ICU events a workgroup of k_day stages in LDS before they go to their buckets
enum { SL_INFECTED = 0, SL_RECOVERED, SL_DEAD, SL_NHD, SL_NR };
enum { LIST_EXP = 0, LIST_ILL = 1, LIST_EV = 2, LIST_BOOK = 3, LIST_CAND = 4 };
enum { EVX_COUNT_R = 4, EVX_RECOVERED_HOME = 5, EVX_DIED_HOME = 6 };

// entries of scan wave `sw` start here in every list (a wave's slice is as large as the number
// of agents it scans: tiles sw, sw + W, ... of 512 agents)
__host__ __device__ __forceinline__ uint32_t scan_slice_base(uint32_t sw, uint32_t scan_waves, uint32_t scan_tiles) {
    const uint32_t tq = scan_tiles / scan_waves, tr = scan_tiles % scan_waves;
    return 512u * (sw * tq + (sw < tr ? sw : tr));
}

// person_become_ill (main.pyx:284-291, 989-1014) + seek_testing (:595-615); `w` already carries
// days_left == 0 from the countdown
// person_become_ill's durations (main.pyx:284-288,989-1014): onset->removed gamma, illness days
__device__ __forceinline__ uint32_t onset_word(const CAS DevParams *P, const GBuffers &B, uint32_t i, uint32_t w, uint32_t day) {
    const CAS reina_disease_t &d = P->dis;
    int v = RH_VARIANT(w), sev = RH_SEV(w);
    float mu = sev == RV_FATAL ? d.mean_duration_from_onset_to_death[v] : d.mean_duration_from_onset_to_recovery[v];
    float od = rp_gamma_mu_cv(mu, 0.45f, P->k0, P->k1, i, day, RP_P_ONSET, 1);
    if (!ABLATED(ONSET_STORE)) B.cold[i].onset_days = od;
    float f = od;
    if (sev >= RV_SEVERE) f *= d.ratio_of_duration_before_hospitalisation[v];
    w = RH_SET_STATE(w, RS_ILLNESS);
    w = RH_SET_DAYS_LEFT(w, clamp_days(B.counters, rp_round_to_int(f)), day);
    w = RH_SET_DOI0(w, day);
    return w;
}

// A workgroup's appends to tomorrow's test queue are staged in LDS and copied out behind ONE allocation (onset_stage_flush):
// at an epidemic peak every wave-step of onsets would otherwise take a returning atomic on the queue's single length word
// -- 16 000 of them a day at 10^8 agents, serialised in L2 at some 10 ns each, i.e. the whole 150 us of that day's last launch.
#define ONSET_STAGE 4000
struct OnsetStage {
    uint32_t n;
    uint32_t base;
    uint32_t item[ONSET_STAGE];
};
__device__ __forceinline__ void onset_stage_push(const CAS DevParams *P, const GBuffers &B, OnsetStage *st, int which, bool pred, uint32_t idx) {
    const uint64_t m = __ballot(pred);
    if (!m) return;
    uint32_t base = 0;
    const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull));
    if (pred && rank == 0) base = atomicAdd(&st->n, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, __ffsll((unsigned long long)m) - 1);
    if (pred) {
        if (base + rank < ONSET_STAGE) st->item[base + rank] = idx;
        else queue_append(P, B, which, idx);   // the stage is full: straight to the queue
    }
}
__device__ __forceinline__ void onset_stage_flush(const CAS DevParams *P, const GBuffers &B, OnsetStage *st, int which) {
    __syncthreads();
    const uint32_t cnt = st->n < ONSET_STAGE ? st->n : ONSET_STAGE;
    if (threadIdx.x == 0 && cnt) st->base = (uint32_t)atomicAdd(&B.control[which ? REINA_L_QUEUE1 : REINA_L_QUEUE0], (int)cnt);
    __syncthreads();
    if (cnt) {
        if (st->base + cnt > P->max_queue) {
            if (threadIdx.x == 0) set_problem(B.counters, REINA_PROBLEM_QUEUE_OVERFLOW);
        } else {
            GAS uint32_t *q = which ? B.queue1 : B.queue0;
            for (uint32_t k = threadIdx.x; k < cnt; k += blockDim.x) q[st->base + k] = st->item[k];
        }
    }
}

// `st`: the workgroup's stage for queue appends (LDS) or nullptr (append at once); all lanes of the wave call together,
// `valid` = this lane has an onset
__device__ __forceinline__ void become_ill(const CAS DevParams *P, const GBuffers &B, const reina_day_t &dp, bool valid, uint32_t i, uint32_t w,
                                           OnsetStage *st) {
    bool queued = false;
    if (valid) {
    const int sev = RH_SEV(w);
    w = onset_word(P, B, i, w, dp.day);
    if (sev != RV_ASYMPTOMATIC && !(w & RH_DETECTED)) {
        int q = 0;
        if (dp.testing_mode == RT_ALL_WITH_SYMPTOMS || dp.testing_mode == RT_ALL_WITH_SYMPTOMS_CT) {
            q = 1;
        } else if (dp.testing_mode == RT_ONLY_SEVERE_SYMPTOMS) {
            if (sev >= RV_SEVERE)
                q = 1;
            else
                q = rp_chance(dp.p_detected_anyway, rp_philox(P->k0, P->k1, i, dp.day, RP_P_ONSET, 0).v[3]);
        }
        if (q && !(w & RH_QUEUED)) {
            w |= RH_QUEUED;
            queued = true;
        }
    }
    B.hot[i] = w;
    }
    if (st) onset_stage_push(P, B, st, (dp.day & 1) ^ 1, queued, i);
    else if (queued) queue_append(P, B, (dp.day & 1) ^ 1, i);
}

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

struct ScanLists {
    GAS uint2 *l[4];     // [LIST_EXP] unused: exposure records go to the wave's LDS strip
    uint32_t n[4];       // wave-uniform counts
    uint2 *strip;        // LDS: pending exposure records at [0, qn)
    uint32_t qn;
    uint32_t n_hosp, n_icu;   // admission / ICU-transfer requests among the events pushed
};

__device__ __forceinline__ void list_push(ScanLists &L, int which, bool pred, uint32_t x, uint32_t y) {
    const uint64_t m = __ballot(pred);
    if (pred && !ABLATED(LIST_STORES)) gst(&L.l[which][L.n[which] + (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull))], make_uint2(x, y));
    L.n[which] += (uint32_t)__popcll(m);
}
__device__ __forceinline__ void strip_push(ScanLists &L, bool pred, uint32_t x, uint32_t y) {
    const uint64_t m = __ballot(pred);
    if (pred) L.strip[L.qn + (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull))] = make_uint2(x, y);
    L.qn += (uint32_t)__popcll(m);
}

// the in-place part for one hot word; returns the word to store (`w` itself when nothing changes
// or when the final word is written later by become_ill)
__device__ __forceinline__ uint32_t scan_word(const CAS DevParams *P, const GBuffers &B, ScanLists &L, bool valid, uint32_t i, uint32_t w, uint32_t day,
                                              uint32_t *ev_stage_n, unsigned long long *ev_stage_key, uint32_t ev_stage_cap,
                                              const uint32_t (*var_par)[4]) {
    const uint32_t st = RH_STATE(w);
    bool p_exp = false, p_ill = false, p_ev = false, p_bk = false;
    uint32_t kind = 0, nw = w;
    if (valid) {
        if (st >= RS_RECOVERED) {
            // removed, not yet counted into R (main.pyx:1969-1972): mark; n_infected is gathered later
            nw = (w | RH_INCLUDED) & ~RH_ACTIVE;
            if (!ABLATED(ACTIVE_CLEAR)) agent_bit_clear(B.active_bits, i);   // (the plane that says the same thing: k_day's sparse days stream it)
            p_bk = true;
            kind = EVX_COUNT_R;
        } else if (RH_INFECTED_TODAY(w, day)) {
            // infected earlier today (an import): waits (main.pyx:402) -- nothing to record, nothing to store
        } else {
            const int v = RH_VARIANT(w), sev = RH_SEV(w);
            uint32_t dl = RH_DAYS_LEFT(w, day);   // absolute days in the word: waiting changes nothing, nw stays w
            if (st <= RS_ILLNESS) {
                if (!(w & RH_DETECTED)) {
                    const int dayrel = st == RS_INCUBATION ? -(int)dl : (int)RH_DOI(w, day);
                    p_exp = dayrel >= -10 && dayrel <= 10 && ((var_par[v][3] >> (dayrel + 10)) & 1u);   // (iot_mask of the variant, staged in LDS)
                }
                if (st == RS_INCUBATION) {
                    if (dl > 0) dl--;
                    p_ill = dl == 0;  // become_ill stores the final word
                } else {
                    if (dl > 0) dl--;
                    if (dl == 0) {
                        if (sev == RV_FATAL && (w & RH_POD_OUTSIDE)) {
                            p_bk = true;
                            kind = EVX_DIED_HOME;
                            nw = RH_SET_STATE(nw, RS_DEAD) & ~RH_HASLIST;
                        } else if (sev >= RV_SEVERE) {
                            p_ev = true;
                            kind = EV_HOSPITALIZE;
                        } else {
                            p_bk = true;
                            kind = EVX_RECOVERED_HOME;
                            nw = RH_SET_STATE(nw, RS_RECOVERED) & ~RH_HASLIST;
                        }
                    }
                }
            } else {
                if (dl > 0) dl--;
                if (dl == 0) {
                    p_ev = true;
                    kind = st == RS_HOSPITALIZED ? (sev >= RV_CRITICAL ? EV_TO_ICU : EV_RELEASE_WARD) : EV_RELEASE_ICU;
                }
            }
        }
    }
    if (__any(p_exp)) strip_push(L, p_exp, i, w);
    if (__any(p_ill)) list_push(L, LIST_ILL, p_ill, i, nw);
    if (__any(p_ev)) {
        hosp_stage_event(P, B, p_ev, i, kind, day, ev_stage_n, ev_stage_key, ev_stage_cap);   // to its priority bucket (k_hospital.inc), by way of the workgroup's stage
        L.n_hosp += (uint32_t)__popcll(__ballot(p_ev && kind == EV_HOSPITALIZE));
        L.n_icu += (uint32_t)__popcll(__ballot(p_ev && kind == EV_TO_ICU));
    }
    if (__any(p_bk)) list_push(L, LIST_BOOK, p_bk, i, kind);
    return p_ill ? w : nw;
}

