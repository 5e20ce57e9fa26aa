// reina_hip.hip part: the bed / ICU event walk (workgroup 0 of k_hosp_contacts): gather, order, saturating scan, apply.
// Included by reina_hip.hip only (one translation unit); not a standalone header.
// ---------------------------------------------------------------------------------------------
// k_hospital: person_hospitalize / transfer_to_icu / release_from_hospital (main.pyx:321-367) +
// HealthcareSystem bed accounting (:617-651). One workgroup gathers the day's events from the scanning
// waves' lists into LDS; when capacity can bind they are sorted by (priority, agent) -- a register /
// shuffle bitonic network up to 1024 events, a bucket sort above -- and the saturating bed / ICU walk is
// replayed in that order as a workgroup scan; days with more events than LDS holds are walked in
// priority ranges (hospital_block below).
#define HOSP_SMALL_RANGES 32
static_assert((uint64_t)HOSP_SMALL_RANGES * 65536u >= REINA_HOSP_SMALL_AGENTS, "REINA_HOSP_RANGES of a population walked by one workgroup");

__device__ __forceinline__ int dies_in_hospital(const CAS DevParams *P, uint32_t i, uint32_t day, int sev, int v, int care) {
    if (sev == RV_FATAL) return 1;
    float p = 0.0f;
    if (sev == RV_CRITICAL) {
        if (care) return 0;
        p = P->dis.p_icu_death_no_beds[v];
    } else if (sev == RV_SEVERE) {
        if (care) return 0;
        p = P->dis.p_hospital_death_no_beds[v];
    }
    return rp_chance(p, rp_philox(P->k0, P->k1, i, day, RP_P_HOSPITAL, 0).v[0]);
}

// saturating-counter walk as a scan: every event acts on the free-bed count x as
// f(x) = max(x + a, m) (admission: a=-1, m=0; release: a=+1, m=-inf); such maps compose to the
// same form, (a1,m1) then (a2,m2) = (a1+a2, max(m1+a2, m2)), so "free beds just before event k"
// is a prefix composition -- computed by a workgroup scan instead of a serial loop.
typedef rp_sat_t SatFn;   // (reina_prims.h: the maps, their composition and their packed form are shared with the CPU checker)
#define SAT_NEG RP_SAT_NEG
__device__ __forceinline__ SatFn sat_then(SatFn f, SatFn g) { return rp_sat_then(f, g); }  // f first, then g
__device__ __forceinline__ int sat_apply(SatFn f, int x) { return rp_sat_apply(f, x); }
__device__ __forceinline__ SatFn bed_fn(int type) {
    SatFn f;
    f.m = SAT_NEG;
    f.a = 0;
    if (type == EV_HOSPITALIZE) { f.a = -1; f.m = 0; }
    else if (type == EV_TO_ICU || type == EV_RELEASE_WARD) f.a = 1;
    return f;
}
__device__ __forceinline__ SatFn icu_fn(int type) {
    SatFn f;
    f.m = SAT_NEG;
    f.a = 0;
    if (type == EV_TO_ICU) { f.a = -1; f.m = 0; }
    else if (type == EV_RELEASE_ICU) f.a = 1;
    return f;
}

enum { HL_INFECTED = 0, HL_DETECTED, HL_ALL_DETECTED, HL_HOSPITALIZED, HL_IN_WARD, HL_IN_ICU, HL_CUM_ICU,
       HL_DEAD, HL_NHD, HL_RECOVERED, HL_NR };

// Bitonic sort of n (power of two, <= E * 1024) 64-bit keys in LDS by the 1024-thread workgroup.
// Thread t keeps elements t*E .. t*E+E-1 in registers: compare-exchange strides below E stay in
// registers, strides below 64*E are wave shuffles, only the strides of 64*E and above go through
// LDS (element r of thread t at [r][t], conflict-free) -- 10 LDS round trips for 16384 keys
// instead of 105.
template <int E, int STRD>
__device__ __forceinline__ void hosp_sort_reg(uint64_t (&x)[E], int size, int tid) {
#pragma unroll
    for (int r = 0; r < E; r++) {
        if ((r & STRD) == 0 && (r | STRD) < E) {
            const bool up = (((tid * E) + r) & size) == 0;
            const uint64_t a = x[r], b = x[r | STRD];
            const bool sw = (a > b) == up;
            x[r] = sw ? b : a;
            x[r | STRD] = sw ? a : b;
        }
    }
}

template <int E>
__device__ __forceinline__ void hosp_sort(uint64_t *ev, int n, int tid) {
    uint64_t x[E];
    const int T = n / E > 0 ? n / E : 1;   // threads that hold keys; the others idle through the barriers
    const bool active = tid < T;            // (events past n in the same LDS array must stay untouched)
#pragma unroll
    for (int r = 0; r < E; r++) x[r] = (tid * E + r < n) ? ev[tid * E + r] : ~0ull;
    __syncthreads();
    for (int size = 2; size <= n; size <<= 1) {
        for (int strd = size >> 1; strd > 0; strd >>= 1) {
            if (strd >= 64 * E) {
                if (active) {
#pragma unroll
                    for (int r = 0; r < E; r++) ev[r * T + tid] = x[r];
                }
                __syncthreads();
                const int m = strd / E;
                const bool take_min = ((tid & m) == 0) == (((tid * E) & size) == 0);
                if (active) {
#pragma unroll
                    for (int r = 0; r < E; r++) {
                        const uint64_t o = ev[r * T + (tid ^ m)];
                        x[r] = take_min ? (o < x[r] ? o : x[r]) : (o > x[r] ? o : x[r]);
                    }
                }
                __syncthreads();
            } else if (strd >= E) {
                const int m = strd / E;   // partner lane = lane ^ m, m in 1..32
                const bool take_min = ((tid & m) == 0) == (((tid * E) & size) == 0);
#pragma unroll
                for (int r = 0; r < E; r++) {
                    const uint64_t o = __shfl_xor((unsigned long long)x[r], m);
                    x[r] = take_min ? (o < x[r] ? o : x[r]) : (o > x[r] ? o : x[r]);
                }
            } else {
                switch (strd) {
                    case 1: hosp_sort_reg<E, 1>(x, size, tid); break;
                    case 2: hosp_sort_reg<E, 2>(x, size, tid); break;
                    case 4: hosp_sort_reg<E, 4>(x, size, tid); break;
                    default: hosp_sort_reg<E, 8>(x, size, tid); break;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < E; r++)
        if (tid * E + r < n) ev[tid * E + r] = x[r];
    __syncthreads();
}

// One bucket of at most 64 * E keys sorted by ONE wave: the same network without its LDS steps (every stride stays in
// registers or in the wave), hence without workgroup barriers -- the small walk sorts its <= 32 buckets side by side,
// two per wave (the buckets are in priority order among themselves already).
template <int E>
__device__ __forceinline__ void hosp_sort_wave(uint64_t *seg, int n, int lane) {
    uint64_t x[E];
#pragma unroll
    for (int r = 0; r < E; r++) x[r] = (lane * E + r < n) ? seg[lane * E + r] : ~0ull;
    for (int size = 2; size <= 64 * E; size <<= 1) {
        for (int strd = size >> 1; strd > 0; strd >>= 1) {
            if (strd >= E) {
                const int m = strd / E;   // partner lane = lane ^ m, m in 1..32
                const bool take_min = ((lane & m) == 0) == (((lane * E) & size) == 0);
#pragma unroll
                for (int r = 0; r < E; r++) {
                    const uint64_t o = __shfl_xor((unsigned long long)x[r], m);
                    x[r] = take_min ? (o < x[r] ? o : x[r]) : (o > x[r] ? o : x[r]);
                }
            } else {
                switch (strd) {
                    case 1: hosp_sort_reg<E, 1>(x, size, lane); break;
                    default: hosp_sort_reg<E, 2>(x, size, lane); break;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < E; r++)
        if (lane * E + r < n) seg[lane * E + r] = x[r];
}


// One bed / ICU event applied to its agent: person_hospitalize / transfer_to_icu / release_from_hospital
// (main.pyx:321-367).  `w`, `od`: the agent's hot word and onset-to-removed duration; `granted`: the bed / ICU
// unit it asks for is free.  Per-age counter changes go to the workgroup's LDS histogram; returns the new word.
__device__ __forceinline__ uint32_t hosp_apply(const CAS DevParams *P, const GBuffers &B, const reina_day_t &dp, const int32_t *s_age_start,
                                               int32_t (*s_cnt)[REINA_MAX_AGES], int type, uint32_t i, uint32_t w, float od, bool granted) {
    const CAS reina_disease_t &d = P->dis;
    const int age = age_of(s_age_start, i, 0, (int)P->nr_ages - 1), v = RH_VARIANT(w), sev = RH_SEV(w);
    int died = -1;  // -1 stays in care, 0 recovers, 1 dies
    if (type == EV_HOSPITALIZE) {
        if (!(w & RH_DETECTED)) {
            w |= RH_DETECTED;
            atomicAdd(&s_cnt[HL_DETECTED][age], 1);
            atomicAdd(&s_cnt[HL_ALL_DETECTED][age], 1);
        }
        if (!granted) {
            died = dies_in_hospital(P, i, dp.day, sev, v, 0);
        } else {
            const float f = rp_ward_stay(sev, od, d.ratio_of_duration_before_hospitalisation[v], d.ratio_of_duration_in_ward[v]);
            w = RH_SET_DAYS_LEFT(RH_SET_STATE(w, RS_HOSPITALIZED), clamp_days(B.counters, rp_round_to_int(f)), dp.day);
            atomicAdd(&s_cnt[HL_HOSPITALIZED][age], 1);
            atomicAdd(&s_cnt[HL_IN_WARD][age], 1);
        }
    } else if (type == EV_TO_ICU) {
        if (!granted && dies_in_hospital(P, i, dp.day, sev, v, 0)) {
            atomicAdd(&s_cnt[HL_IN_WARD][age], -1);
            atomicAdd(&s_cnt[HL_HOSPITALIZED][age], -1);
            died = 1;
        } else {
            const float f = rp_icu_stay(sev, od, d.ratio_of_duration_before_hospitalisation[v], d.ratio_of_duration_in_ward[v]);
            w = RH_SET_DAYS_LEFT(RH_SET_STATE(w, RS_IN_ICU), clamp_days(B.counters, rp_round_to_int(f)), dp.day);
            atomicAdd(&s_cnt[HL_IN_WARD][age], -1);
            atomicAdd(&s_cnt[HL_IN_ICU][age], 1);
            atomicAdd(&s_cnt[HL_CUM_ICU][age], 1);
        }
    } else if (type == EV_RELEASE_WARD) {
        atomicAdd(&s_cnt[HL_IN_WARD][age], -1);
        atomicAdd(&s_cnt[HL_HOSPITALIZED][age], -1);
        died = dies_in_hospital(P, i, dp.day, sev, v, 1);
    } else {
        atomicAdd(&s_cnt[HL_IN_ICU][age], -1);
        atomicAdd(&s_cnt[HL_HOSPITALIZED][age], -1);
        died = dies_in_hospital(P, i, dp.day, sev, v, 1);
    }
    if (died == 1) {
        atomicAdd(&s_cnt[HL_INFECTED][age], -1);
        atomicAdd(&s_cnt[HL_DEAD][age], 1);
        if (w & RH_POD_OUTSIDE) atomicAdd(&s_cnt[HL_NHD][age], 1);
        w = RH_SET_STATE(w, RS_DEAD) & ~RH_HASLIST;
    } else if (died == 0) {
        atomicAdd(&s_cnt[HL_INFECTED][age], -1);
        atomicAdd(&s_cnt[HL_RECOVERED][age], 1);
        w = RH_SET_STATE(w, RS_RECOVERED) & ~RH_HASLIST;
    }
    return w;
}

// the workgroup's event histogram -> the global per-age counters
__device__ __forceinline__ void hosp_flush_counts(const GBuffers &B, int32_t (*s_cnt)[REINA_MAX_AGES], int nthreads) {
    for (int k = threadIdx.x; k < HL_NR * REINA_MAX_AGES; k += nthreads) {
        int32_t v = (&s_cnt[0][0])[k];
        if (v) {
            const int map[HL_NR] = {REINA_C_INFECTED, REINA_C_DETECTED, REINA_C_ALL_DETECTED, REINA_C_HOSPITALIZED,
                                    REINA_C_IN_WARD, REINA_C_IN_ICU, REINA_C_CUM_ICU, REINA_C_DEAD,
                                    REINA_C_NON_HOSPITAL_DEATHS, REINA_C_RECOVERED};
            atomicAdd(&B.counters[CNT_IDX(map[k / REINA_MAX_AGES], k % REINA_MAX_AGES)], v);
        }
    }
}

// Can a bed or an ICU unit run out today?  Only then does the ORDER of the day's events matter (and one workgroup
// replays them in priority order, hospital_block); otherwise every request is granted and the events are applied
// by all workgroups in parallel (install_block).  Decided from words that are stable during the day's last
// launch: the free beds / units when the day opened (k_open) and the day's admission / transfer counts (k_day).
__device__ __forceinline__ bool hosp_day_is_ordered(const GBuffers &B) {
    const int b0 = B.control[REINA_L_BEDS_OPEN], c0 = B.control[REINA_L_ICU_OPEN];
    const int nH = B.control[REINA_L_EV_HOSPITALIZE], nT = B.control[REINA_L_EV_TO_ICU];
    return b0 < nH || c0 < nT;
}

// Decisions for the n sorted keys ev[0..n) (LDS) given the free beds / units just before the first of them:
// bit 63 of a key is set when its request is refused.  Chunked scan of the saturating maps: thread t owns the
// keys [t * per, (t + 1) * per).  Returns the free counts after the last key in *b_out / *c_out (all threads).
template <int NT>
__device__ __forceinline__ void hosp_decide(uint64_t *ev, int n, int b_in, int c_in, SatFn *s_fb, SatFn *s_fc, int *b_out, int *c_out) {
    const int tid = threadIdx.x;
    const int per = (n + NT - 1) / NT;
    const int lo = min(n, tid * per), hi = min(n, lo + per);
    SatFn fb, fc;
    fb.a = fc.a = 0;
    fb.m = fc.m = SAT_NEG;
    for (int k = lo; k < hi; k++) {
        int type = (int)(ev[k] & 3);
        fb = sat_then(fb, bed_fn(type));
        fc = sat_then(fc, icu_fn(type));
    }
    s_fb[tid] = fb;
    s_fc[tid] = fc;
    __syncthreads();
    // inclusive Hillis-Steele scan of the per-thread maps (composition is associative)
    for (int off = 1; off < NT; off <<= 1) {
        SatFn pb = fb, pc = fc;
        if (tid >= off) {
            pb = sat_then(s_fb[tid - off], fb);
            pc = sat_then(s_fc[tid - off], fc);
        }
        __syncthreads();
        fb = pb;
        fc = pc;
        s_fb[tid] = fb;
        s_fc[tid] = fc;
        __syncthreads();
    }
    int b = b_in, c = c_in;
    if (tid > 0) {
        b = sat_apply(s_fb[tid - 1], b_in);
        c = sat_apply(s_fc[tid - 1], c_in);
    }
    for (int k = lo; k < hi; k++) {
        int type = (int)(ev[k] & 3);
        uint8_t ok = 1;
        if (type == EV_HOSPITALIZE) {
            if (b == 0) ok = 0; else b--;
        } else if (type == EV_TO_ICU) {
            b++;
            if (c == 0) ok = 0; else c--;
        } else if (type == EV_RELEASE_WARD) {
            b++;
        } else {
            c++;
        }
        if (!ok) ev[k] |= 1ull << 63;
    }
    *b_out = sat_apply(s_fb[NT - 1], b_in);
    *c_out = sat_apply(s_fc[NT - 1], c_in);
    __syncthreads();
}

// applies the decided events ev[0..n) (LDS): four per thread in flight, their hot words and onset durations
// requested together
template <int NT>
__device__ __forceinline__ void hosp_apply_all(const CAS DevParams *P, const GBuffers &B, const reina_day_t &dp, const int32_t *s_age_start,
                                               int32_t (*s_cnt)[REINA_MAX_AGES], const uint64_t *ev, int n) {
    const int tid = threadIdx.x;
    for (int k0 = tid; k0 < n; k0 += 4 * NT) {
        uint64_t e4[4];
        uint32_t w4[4];
        float od4[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (k0 + j * NT < n) {
                e4[j] = ev[k0 + j * NT];
                const uint32_t i = (uint32_t)((e4[j] >> 2) & 0xFFFFFFFFu);
                w4[j] = B.hot[i];
                od4[j] = B.cold[i].onset_days;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (k0 + j * NT >= n) break;
            const uint64_t e = e4[j];
            const uint32_t i = (uint32_t)((e >> 2) & 0xFFFFFFFFu);
            B.hot[i] = hosp_apply(P, B, dp, s_age_start, s_cnt, (int)(e & 3), i, w4[j], od4[j], !(e >> 63));
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Small populations (at most REINA_MAX_HOSP_EVENTS events a day by construction: DevParams.hosp_parallel == 0):
// ONE workgroup of k_hosp_install gathers the buckets into LDS, sorts and walks them.  `s_cnt`: the
// workgroup's [HL_NR][ages] histogram (LDS, shared with the parallel event path of install_block).
__device__ __forceinline__ void hospital_block(const MemberRef &mref_, const reina_day_t &dp, int32_t (*s_cnt)[REINA_MAX_AGES],
                                               SatFn (*s_f)[HOSP_THREADS]) {
    const CAS DevParams *P = (const CAS DevParams *)mref_.P;
    const GBuffers B = global_buffers(mref_.B);
    extern __shared__ __align__(16) unsigned char smem[];
    uint64_t *ev = reinterpret_cast<uint64_t *>(smem);               // [REINA_MAX_HOSP_EVENTS]
    __shared__ int32_t s_age_start[REINA_MAX_AGES + 1];
    // (a population this walk serves has at most HOSP_SMALL_RANGES buckets: one per 65 536 agents, include/reina_hip.h)
    __shared__ uint32_t s_base[HOSP_SMALL_RANGES + 1];               // exclusive prefix of the bucket counts
    DIAG_CLOCK(HOSP, hs_t);   // (-DREINA_HOSP_STAMPS: the walk's phases, reina_diag.h)
    const int tid = threadIdx.x;
    const uint32_t R = P->hosp_ranges, C = P->hosp_bucket_cap;
    __shared__ uint32_t s_n[HOSP_SMALL_RANGES];
    if ((uint32_t)tid < R) {   // (R <= 32 here) the counts come in side by side, one lane each; the prefix is then LDS arithmetic
        const uint32_t c = hosp_counts(B)[tid];
        s_n[tid] = c < C ? c : C;
    }
    if (tid <= REINA_MAX_AGES) s_age_start[tid] = P->age_start[tid];
    for (int k = tid; k < HL_NR * REINA_MAX_AGES; k += HOSP_THREADS) (&s_cnt[0][0])[k] = 0;
    __syncthreads();
    if (tid == 0) {
        uint32_t acc = 0;
        for (uint32_t r = 0; r < R; r++) {
            s_base[r] = acc;
            acc += s_n[r];
        }
        s_base[R] = acc;
    }
    __syncthreads();
    const int M = (int)s_base[R];
    if (M == 0) return;
    if (tid == 0 && M > B.control[REINA_L_HOSP_PEAK]) B.control[REINA_L_HOSP_PEAK] = M;
    if (M > REINA_MAX_HOSP_EVENTS - HOSP_THREADS) {   // (a run is padded to a power of two in place: room for that)
        if (tid == 0) set_problem(B.counters, REINA_PROBLEM_HOSPITAL_OVERFLOW);
        return;
    }
    // all keys of the day in one sweep: key p of the concatenation lives in the bucket r with s_base[r] <= p < s_base[r + 1]
    // (5 LDS steps to find it; one global round trip for the whole day instead of one per bucket)
    for (int p0 = tid; p0 < M; p0 += HOSP_THREADS) {
        uint32_t lo = 0, hi = R - 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (s_base[mid] <= (uint32_t)p0) lo = mid; else hi = mid - 1;
        }
        ev[p0] = hosp_bucket(P, B, lo)[(uint32_t)p0 - s_base[lo]];
    }
    __syncthreads();
    DIAG_LAP(HOSP, DIAG_HOSP_GATHER, DIAG_THREAD0, hs_t, B.mirror);
    // The buckets are in priority order among themselves.  Usual day: no bucket holds more than 256 keys, and every bucket
    // is sorted by one wave on its own (registers + shuffles, no barrier), two buckets per wave.  Otherwise: runs of whole
    // buckets holding at most 1024 keys are sorted one after the other by the workgroup's network.
    uint32_t n_max = 0;
    for (uint32_t r = 0; r < R; r++) n_max = s_n[r] > n_max ? s_n[r] : n_max;   // (uniform: LDS broadcast reads)
    if (n_max <= 256u) {
        const int lane = tid & 63, wave = tid >> 6;
        for (uint32_t r = (uint32_t)wave; r < R; r += HOSP_THREADS / 64) {
            const int n = (int)s_n[r];
            uint64_t *seg = ev + s_base[r];
            if (n <= 1) continue;
            if (n <= 64) hosp_sort_wave<1>(seg, n, lane);
            else if (n <= 128) hosp_sort_wave<2>(seg, n, lane);
            else hosp_sort_wave<4>(seg, n, lane);
        }
        __syncthreads();
    } else
    for (uint32_t r0 = 0; r0 < R;) {
        uint32_t r1 = r0 + 1;
        while (r1 < R && s_base[r1 + 1] - s_base[r0] <= (uint32_t)HOSP_THREADS) r1++;
        const int n = (int)(s_base[r1] - s_base[r0]);
        if (n > HOSP_THREADS) {   // a single bucket of more than 1024 keys: the day holds more than the walk can order
            if (tid == 0) set_problem(B.counters, REINA_PROBLEM_HOSPITAL_OVERFLOW);
            return;
        }
        if (n > 1) {
            // (the network sorts a power of two of keys in place; the keys behind this run are parked in registers)
            int n2 = 1;
            while (n2 < n) n2 <<= 1;
            uint64_t *seg = ev + s_base[r0];
            const int behind = (int)s_base[r0] + n + tid < M && tid < n2 - n;
            const uint64_t parked = behind ? seg[n + tid] : 0ull;
            __syncthreads();
            if (tid < n2 - n) seg[n + tid] = ~0ull;
            __syncthreads();
            hosp_sort<1>(seg, n2, tid);
            if (behind) seg[n + tid] = parked;
            __syncthreads();
        }
        r0 = r1;
    }
    DIAG_LAP(HOSP, DIAG_HOSP_SORT, DIAG_THREAD0, hs_t, B.mirror);
    int b_end, c_end;
    const int b0 = B.control[REINA_L_BEDS_OPEN], c0 = B.control[REINA_L_ICU_OPEN];
    hosp_decide<HOSP_THREADS>(ev, M, b0, c0, s_f[0], s_f[1], &b_end, &c_end);
    DIAG_LAP(HOSP, DIAG_HOSP_DECIDE, DIAG_THREAD0, hs_t, B.mirror);
    hosp_apply_all<HOSP_THREADS>(P, B, dp, s_age_start, s_cnt, ev, M);
    __syncthreads();
    DIAG_LAP(HOSP, DIAG_HOSP_APPLY, DIAG_THREAD0, hs_t, B.mirror);
    hosp_flush_counts(B, s_cnt, HOSP_THREADS);
    if (tid == 0) {
        B.counters[SC_IDX(REINA_S_AVAILABLE_BEDS)] = b_end;
        B.counters[SC_IDX(REINA_S_AVAILABLE_ICU)] = c_end;
    }
    DIAG_LAP(HOSP, DIAG_HOSP_FLUSH, DIAG_THREAD0, hs_t, B.mirror);
}

// ---------------------------------------------------------------------------------------------
// Large populations (DevParams.hosp_parallel): tens of thousands of events on the days a resource can run out -- one
// workgroup would take hundreds of microseconds for them.  The ordered walk rides in the day's LAST launch
// (k_hosp_install) as a role of its own: a few "walker" workgroups that leave at once on a day on which order does not
// matter (round 2 had two launches of their own for it, k_hosp_sort / k_hosp_walk: 9-15 us of empty launches a day).
//
// Buckets are handed out by TICKET (REINA_L_WALK_TICKET, zeroed by the day's opening; a ticket is sixteen consecutive
// buckets, one per wave of the workgroup that took it): whoever holds bucket b
//   1. sorts it (a wave in registers and shuffles for up to HOSP_WAVE_KEYS keys, the workgroup's network above),
//   2. PUBLISHES the bucket's composed saturating map (free beds, free units -> after the bucket) as ONE 64-bit word,
//   3. waits for the words of the buckets before its own, composes them in order -- the free beds / units when its first
//      event comes up --, decides its events and applies them.
// A holder publishes before it waits and waits only for LOWER tickets, all of them taken by waves that are already
// running: no assumption about which workgroups are resident together.  The wait is bounded by a poll count
// (REINA_PROBLEM_SYNC_TIMEOUT).  Same single ordered walk as oracle B's one sorted pass.
#define HOSP_P_THREADS HOSP_THREADS
#define HOSP_P_E 4           // keys per thread of the workgroup's network: buckets of up to 4096 keys
#define HOSP_WAVE_KEYS 256   // a bucket of at most this many keys is sorted and walked by ONE wave
static_assert(HOSP_P_THREADS * HOSP_P_E == REINA_HOSP_MAX_BUCKET_KEYS, "the workgroup network holds a full bucket");

__device__ __forceinline__ uint64_t sat_pack(SatFn fb, SatFn fc) { return rp_sat_pack(fb, fc); }
__device__ __forceinline__ void sat_unpack(uint64_t v, SatFn *fb, SatFn *fc) { rp_sat_unpack(v, fb, fc); }
__device__ __forceinline__ GAS uint64_t *hosp_agg64(const CAS DevParams *P, const GBuffers &B) {
    return B.hosp_events + HOSP_AGG_OFF(P->hosp_ranges);   // [R] published words (the day's opening zeroes them)
}
__device__ __forceinline__ SatFn sat_id() { return rp_sat_id(); }
// waits for the published word of bucket q (bounded; 0 = gave up, day flagged failed)
__device__ __forceinline__ uint64_t hosp_wait_agg(const GBuffers &B, const GAS uint64_t *agg, uint32_t q) {
    uint32_t polls = 0;
    for (;;) {
        const uint64_t v = __hip_atomic_load(&agg[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v >> 63) return v;
        __builtin_amdgcn_s_sleep(4);
        if (++polls > (1u << 22)) {
            set_problem(B.counters, REINA_PROBLEM_SYNC_TIMEOUT);
            return 0;
        }
    }
}
__device__ __forceinline__ SatFn sat_shfl_up(SatFn f, int off) {
    SatFn r;
    r.a = __shfl_up(f.a, off);
    r.m = __shfl_up(f.m, off);
    return r;
}
__device__ __forceinline__ SatFn sat_shfl(SatFn f, int src) {
    SatFn r;
    r.a = __shfl(f.a, src);
    r.m = __shfl(f.m, src);
    return r;
}

// A sharded population (exact pooled capacity, include/reina_hip.h: REINA_EXCHANGE_WORDS) does the same in two launches
// around its daily all-reduce: WALK_PRESORT (k_hosp_presort, before it) sorts every bucket in place and writes the bucket's
// map into this shard's segment of the exchange block; WALK_SHARDED (the walkers of k_hosp_install, after it) finds the
// sorted bucket, takes the composed map of EVERYTHING before its bucket in the global order (bucket, shard, priority,
// agent) from the table k_remote made of all shards' maps, and walks its events against the one pool.
enum { WALK_LOCAL = 0, WALK_PRESORT = 1, WALK_SHARDED = 2 };
// this shard's segment of the exchanged table / the prefix table k_remote derives from it (k_remote.inc)
__device__ __forceinline__ GAS uint64_t *hosp_exchange_maps(const CAS DevParams *P, const GBuffers &B, uint32_t shard) {
    return reinterpret_cast<GAS uint64_t *>(B.pressure + REINA_PRESSURE_WORDS) + (size_t)shard * P->hosp_ranges;
}
__device__ __forceinline__ GAS int32_t *hosp_prefix_table(const CAS DevParams *P, const GBuffers &B) {
    return reinterpret_cast<GAS int32_t *>(B.hosp_events + HOSP_AGG_OFF(P->hosp_ranges));   // [R][4]: bed map (a, m), ICU map (a, m)
}

// One bucket of n <= 64 * E keys, sorted, decided and applied by ONE wave: no LDS for the keys, no workgroup barrier.
// `s_delta`: [2] LDS accumulators of the pool's net change by this shard's events (WALK_SHARDED).
template <int E>
__device__ __forceinline__ void hosp_walk_bucket_wave(const CAS DevParams *P, const GBuffers &B, const reina_day_t &dp, const int32_t *s_age_start,
                                                      int32_t (*s_cnt)[REINA_MAX_AGES], uint32_t b, uint32_t n, int lane, int mode, int32_t *s_delta) {
    const uint32_t R = P->hosp_ranges;
    GAS uint64_t *bucket = hosp_bucket(P, B, b);
    GAS uint64_t *agg = hosp_agg64(P, B);
    uint64_t x[E];
#pragma unroll
    for (int r = 0; r < E; r++) x[r] = ((uint32_t)(lane * E + r) < n) ? bucket[lane * E + r] : ~0ull;
    if (n > 1) {
        for (int size = 2; size <= 64 * E; size <<= 1) {
            for (int strd = size >> 1; strd > 0; strd >>= 1) {
                if (strd >= E) {
                    const int m = strd / E;
                    const bool take_min = ((lane & m) == 0) == (((lane * E) & size) == 0);
#pragma unroll
                    for (int r = 0; r < E; r++) {
                        const uint64_t o = __shfl_xor((unsigned long long)x[r], m);
                        x[r] = take_min ? (o < x[r] ? o : x[r]) : (o > x[r] ? o : x[r]);
                    }
                } else {
                    switch (strd) {
                        case 1: hosp_sort_reg<E, 1>(x, size, lane); break;
                        default: hosp_sort_reg<E, 2>(x, size, lane); break;
                    }
                }
            }
        }
    }
    // the events' agents: hot word and onset-to-removed time requested now, they arrive while the maps are composed
    uint32_t w4[E];
    float od4[E];
#pragma unroll
    for (int r = 0; r < E; r++) {
        const bool in = x[r] != ~0ull && mode != WALK_PRESORT;
        const uint32_t i = (uint32_t)((x[r] >> 2) & 0xFFFFFFFFu);
        w4[r] = in ? (uint32_t)B.hot[i] : 0u;
        od4[r] = in ? (float)B.cold[i].onset_days : 0.0f;
    }
    // this lane's keys composed; inclusive scan over the lanes (lane order = key order)
    SatFn fb = sat_id(), fc = sat_id();
#pragma unroll
    for (int r = 0; r < E; r++)
        if (x[r] != ~0ull) {
            const int type = (int)(x[r] & 3u);
            fb = sat_then(fb, bed_fn(type));
            fc = sat_then(fc, icu_fn(type));
        }
    SatFn ib = fb, ic = fc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const SatFn pb = sat_shfl_up(ib, off), pc = sat_shfl_up(ic, off);
        if (lane >= off) {
            ib = sat_then(pb, ib);
            ic = sat_then(pc, ic);
        }
    }
    const SatFn tot_b = sat_shfl(ib, 63), tot_c = sat_shfl(ic, 63);
    if (mode == WALK_PRESORT) {
        // the sorted bucket goes back where it was, its map into this shard's segment of the exchange block (an empty
        // bucket leaves its word zero: no events)
#pragma unroll
        for (int r = 0; r < E; r++)
            if ((uint32_t)(lane * E + r) < n) bucket[lane * E + r] = x[r];
        if (lane == 0 && n) hosp_exchange_maps(P, B, P->shard_rank)[b] = sat_pack(tot_b, tot_c);
        return;
    }
    SatFn pfb = sat_id(), pfc = sat_id();
    if (mode == WALK_SHARDED) {
        // everything before this bucket in the global order, composed by k_remote from all shards' maps
        const GAS int32_t *pre = hosp_prefix_table(P, B) + 4u * b;
        pfb.a = pre[0]; pfb.m = pre[1]; pfc.a = pre[2]; pfc.m = pre[3];
    } else {
    if (lane == 0) __hip_atomic_store(&agg[b], sat_pack(tot_b, tot_c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the buckets before this one: lane l composes the run [l * per, (l + 1) * per) in order, the runs are scanned
    {
        const uint32_t per = (b + 63u) / 64u;   // <= 16 (REINA_HOSP_MAX_RANGES = 1024 buckets)
        const uint32_t lo = (uint32_t)lane * per;
        uint64_t v[16];
#pragma unroll
        for (uint32_t k = 0; k < 16u; k++) {
            const uint32_t q = lo + k;
            v[k] = (k < per && q < b) ? __hip_atomic_load(&agg[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : sat_pack(sat_id(), sat_id());
        }
#pragma unroll
        for (uint32_t k = 0; k < 16u; k++) {
            const uint32_t q = lo + k;
            if (k < per && q < b) {
                if (!(v[k] >> 63)) v[k] = hosp_wait_agg(B, agg, q);
                SatFn gb, gc;
                sat_unpack(v[k], &gb, &gc);
                pfb = sat_then(pfb, gb);
                pfc = sat_then(pfc, gc);
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const SatFn qb = sat_shfl_up(pfb, off), qc = sat_shfl_up(pfc, off);
            if (lane >= off) {
                pfb = sat_then(qb, pfb);
                pfc = sat_then(qc, pfc);
            }
        }
        pfb = sat_shfl(pfb, 63);
        pfc = sat_shfl(pfc, 63);
    }
    }
    const int b_in = sat_apply(pfb, B.control[REINA_L_BEDS_OPEN]), c_in = sat_apply(pfc, B.control[REINA_L_ICU_OPEN]);
    // free beds / units when this lane's first key comes up
    SatFn eb = sat_shfl_up(ib, 1), ec = sat_shfl_up(ic, 1);
    int fbeds = b_in, funits = c_in;
    if (lane > 0) {
        fbeds = sat_apply(eb, b_in);
        funits = sat_apply(ec, c_in);
    }
#pragma unroll
    for (int r = 0; r < E; r++) {
        if (x[r] == ~0ull) continue;
        const int type = (int)(x[r] & 3u);
        bool ok = true;
        if (type == EV_HOSPITALIZE) {
            if (fbeds == 0) ok = false; else fbeds--;
        } else if (type == EV_TO_ICU) {
            fbeds++;
            if (funits == 0) ok = false; else funits--;
        } else if (type == EV_RELEASE_WARD) {
            fbeds++;
        } else {
            funits++;
        }
        const uint32_t i = (uint32_t)((x[r] >> 2) & 0xFFFFFFFFu);
        B.hot[i] = hosp_apply(P, B, dp, s_age_start, s_cnt, type, i, w4[r], od4[r], ok);
    }
    if (mode == WALK_SHARDED && lane == 0) {
        // this shard's counters follow its OWN events' effect on the pool (the shards' counters add up to the pool)
        const int db = sat_apply(tot_b, b_in) - b_in, dc = sat_apply(tot_c, c_in) - c_in;
        if (db) atomicAdd(&s_delta[0], db);
        if (dc) atomicAdd(&s_delta[1], dc);
    }
    if (b + 1u == R) {   // the day's last bucket: free beds / units after the last event, and the statistics word
        uint32_t mine = 0;
        for (uint32_t q = (uint32_t)lane; q < R; q += 64u) mine += hosp_counts(B)[q];
        const int total = wave_sum((int)mine);
        if (lane == 0) {
            if (mode == WALK_LOCAL) {
                B.counters[SC_IDX(REINA_S_AVAILABLE_BEDS)] = sat_apply(tot_b, b_in);
                B.counters[SC_IDX(REINA_S_AVAILABLE_ICU)] = sat_apply(tot_c, c_in);
            }
            if (total > B.control[REINA_L_HOSP_PEAK]) B.control[REINA_L_HOSP_PEAK] = total;
        }
    }
}

// The walker role of k_hosp_install (an ordered day of a large population).  `ev`: LDS for HOSP_P_THREADS * HOSP_P_E keys
// (the launch's dynamic LDS), `s_f`: [2][HOSP_P_THREADS] maps -- both used only when some bucket holds more keys than a
// wave sorts.
// `mode`: WALK_LOCAL (unsharded), WALK_PRESORT (k_hosp_presort) or WALK_SHARDED (see hosp_walk_bucket_wave).
__device__ __forceinline__ void hosp_walker_block(const MemberRef &mref_, const reina_day_t &dp, int32_t (*s_cnt)[REINA_MAX_AGES],
                                                  uint64_t *ev, SatFn (*s_f)[HOSP_THREADS], int mode) {
    const CAS DevParams *P = (const CAS DevParams *)mref_.P;
    const GBuffers B = global_buffers(mref_.B);
    __shared__ int32_t s_age_start[REINA_MAX_AGES + 1];
    __shared__ uint32_t s_nmax, s_ticket;
    __shared__ int32_t s_delta[2];   // WALK_SHARDED: the pool's net change by this workgroup's events (beds, ICU units)
    const int tid = threadIdx.x, lane = tid & 63;
    const uint32_t R = P->hosp_ranges, C = P->hosp_bucket_cap;
    GAS int32_t *ticket = &B.control[mode == WALK_PRESORT ? REINA_L_SORT_TICKET : REINA_L_WALK_TICKET];
    for (int k = tid; k < HL_NR * REINA_MAX_AGES; k += HOSP_THREADS) (&s_cnt[0][0])[k] = 0;
    if (tid <= REINA_MAX_AGES) s_age_start[tid] = P->age_start[tid];
    if (tid == 0) s_nmax = 0;
    if (tid < 2) s_delta[tid] = 0;
    __syncthreads();
    {   // the fullest bucket decides the mode, for every walker alike (the counts are final: k_day wrote them)
        uint32_t m = 0;
        for (uint32_t q = (uint32_t)tid; q < R; q += HOSP_THREADS) {
            const uint32_t c = hosp_counts(B)[q];
            m = c > m ? c : m;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)m, off);
            m = o > m ? o : m;
        }
        if (lane == 0 && m) atomicMax(&s_nmax, m);
    }
    __syncthreads();
    GAS uint64_t *agg = hosp_agg64(P, B);
    if (s_nmax <= HOSP_WAVE_KEYS) {
        // the usual day: every wave walks a bucket on its own.  Tickets are taken per WORKGROUP, sixteen buckets each, one per
        // wave (a ticket per wave was 2 R returning atomics on one address: 20 us of serialised L2 traffic at R = 1024).
        // (The ticket itself is read by every lane from LDS: no branch on the lane number in front of wave-uniform values --
        // with `if (lane == 0) b = atomicAdd(..)` followed by a readfirstlane, the compiler threaded that branch into the
        // `if (lane == 0)` that ends the walk of the day's last bucket; lane 0 and the others then came round the loop on
        // different paths, the others read their own initial 0 and walked bucket 0 a second time: four events applied
        // twice on the first ordered day of the 2.5 M-agent test, found with tools/walk_diff.py.)
        const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
        for (;;) {
            __syncthreads();
            if (tid == 0) s_ticket = (uint32_t)atomicAdd(ticket, 1);
            __syncthreads();
            const uint32_t b0 = s_ticket * (HOSP_THREADS / 64u);
            if (b0 >= R) break;
            const uint32_t b = b0 + wave;
            if (b < R) {
                uint32_t n = hosp_counts(B)[b];
                if (n > C) n = C;   // (the overflow was flagged when it happened)
                if (n <= 64u) hosp_walk_bucket_wave<1>(P, B, dp, s_age_start, s_cnt, b, n, lane, mode, s_delta);
                else if (n <= 128u) hosp_walk_bucket_wave<2>(P, B, dp, s_age_start, s_cnt, b, n, lane, mode, s_delta);
                else hosp_walk_bucket_wave<4>(P, B, dp, s_age_start, s_cnt, b, n, lane, mode, s_delta);
            }
        }
    } else {
        // a day with a bucket of more than HOSP_WAVE_KEYS keys: the whole workgroup takes one bucket at a time
        for (;;) {
            __syncthreads();
            if (tid == 0) s_ticket = (uint32_t)atomicAdd(ticket, 1);
            __syncthreads();
            const uint32_t b = s_ticket;
            if (b >= R) break;
            uint32_t n = hosp_counts(B)[b];
            if (n > C) n = C;   // (the overflow was flagged when it happened)
            GAS uint64_t *bucket = hosp_bucket(P, B, b);
            int n2 = HOSP_P_E;   // the network needs at least one key per register slot
            while (n2 < (int)n) n2 <<= 1;
            for (int k = tid; k < n2; k += HOSP_P_THREADS) ev[k] = k < (int)n ? bucket[k] : ~0ull;
            __syncthreads();
            if (n > 1) hosp_sort<HOSP_P_E>(ev, n2, tid);
            // the bucket's composed map: thread t composes its chunk, then an ordered scan over the threads
            const int per = ((int)n + HOSP_P_THREADS - 1) / HOSP_P_THREADS;
            const int lo = min((int)n, tid * per), hi = min((int)n, lo + per);
            SatFn fb = sat_id(), fc = sat_id();
            for (int k = lo; k < hi; k++) {
                const int type = (int)(ev[k] & 3);
                fb = sat_then(fb, bed_fn(type));
                fc = sat_then(fc, icu_fn(type));
            }
            s_f[0][tid] = fb;
            s_f[1][tid] = fc;
            __syncthreads();
            for (int off = 1; off < HOSP_P_THREADS; off <<= 1) {
                SatFn pb = fb, pc = fc;
                if (tid >= off) {
                    pb = sat_then(s_f[0][tid - off], fb);
                    pc = sat_then(s_f[1][tid - off], fc);
                }
                __syncthreads();
                fb = pb;
                fc = pc;
                s_f[0][tid] = fb;
                s_f[1][tid] = fc;
                __syncthreads();
            }
            if (mode == WALK_PRESORT) {
                // the sorted bucket back in place, its map into this shard's segment of the exchange block
                if (tid == HOSP_P_THREADS - 1 && n) hosp_exchange_maps(P, B, P->shard_rank)[b] = sat_pack(fb, fc);
                for (int k = tid; k < (int)n; k += HOSP_P_THREADS) bucket[k] = ev[k];
                continue;
            }
            int b_in, c_in;
            if (mode == WALK_SHARDED) {
                // everything before this bucket in the global order, composed by k_remote from all shards' maps
                const GAS int32_t *pre = hosp_prefix_table(P, B) + 4u * b;
                SatFn pb, pc;
                pb.a = pre[0]; pb.m = pre[1]; pc.a = pre[2]; pc.m = pre[3];
                b_in = sat_apply(pb, B.control[REINA_L_BEDS_OPEN]);
                c_in = sat_apply(pc, B.control[REINA_L_ICU_OPEN]);
                __syncthreads();
            } else {
            if (tid == HOSP_P_THREADS - 1) __hip_atomic_store(&agg[b], sat_pack(fb, fc), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            // the maps of the buckets before this one, composed in order: thread t takes bucket t (R <= HOSP_P_THREADS)
            fb = sat_id();
            fc = sat_id();
            if ((uint32_t)tid < b) {
                const uint64_t v = hosp_wait_agg(B, agg, (uint32_t)tid);
                if (v) sat_unpack(v, &fb, &fc);
            }
            s_f[0][tid] = fb;
            s_f[1][tid] = fc;
            __syncthreads();
            for (int off = 1; off < HOSP_P_THREADS; off <<= 1) {
                SatFn pb = fb, pc = fc;
                if (tid >= off) {
                    pb = sat_then(s_f[0][tid - off], fb);
                    pc = sat_then(s_f[1][tid - off], fc);
                }
                __syncthreads();
                fb = pb;
                fc = pc;
                s_f[0][tid] = fb;
                s_f[1][tid] = fc;
                __syncthreads();
            }
            b_in = sat_apply(s_f[0][HOSP_P_THREADS - 1], B.control[REINA_L_BEDS_OPEN]);
            c_in = sat_apply(s_f[1][HOSP_P_THREADS - 1], B.control[REINA_L_ICU_OPEN]);
            __syncthreads();
            }
            int b_end, c_end;
            hosp_decide<HOSP_P_THREADS>(ev, (int)n, b_in, c_in, s_f[0], s_f[1], &b_end, &c_end);
            hosp_apply_all<HOSP_P_THREADS>(P, B, dp, s_age_start, s_cnt, ev, (int)n);
            if (mode == WALK_SHARDED && tid == 0) {   // this shard's counters follow its own events' effect on the pool
                if (b_end - b_in) atomicAdd(&s_delta[0], b_end - b_in);
                if (c_end - c_in) atomicAdd(&s_delta[1], c_end - c_in);
            }
            if (b + 1u == R) {   // free beds / units after the day's last event; the statistics word
                uint32_t mine = 0;
                for (uint32_t q = (uint32_t)tid; q < R; q += HOSP_P_THREADS) mine += hosp_counts(B)[q];
                const int part = wave_sum((int)mine);
                __shared__ int s_total;
                if (tid == 0) s_total = 0;
                __syncthreads();
                if (lane == 0 && part) atomicAdd(&s_total, part);
                __syncthreads();
                if (tid == 0) {
                    if (mode == WALK_LOCAL) {
                        B.counters[SC_IDX(REINA_S_AVAILABLE_BEDS)] = b_end;
                        B.counters[SC_IDX(REINA_S_AVAILABLE_ICU)] = c_end;
                    }
                    if (s_total > B.control[REINA_L_HOSP_PEAK]) B.control[REINA_L_HOSP_PEAK] = s_total;
                }
            }
        }
    }
    __syncthreads();
    if (mode == WALK_PRESORT) return;
    hosp_flush_counts(B, s_cnt, HOSP_THREADS);
    if (mode == WALK_SHARDED && tid < 2 && s_delta[tid])
        atomicAdd(&B.counters[SC_IDX(tid == 0 ? REINA_S_AVAILABLE_BEDS : REINA_S_AVAILABLE_ICU)], s_delta[tid]);
}

// k_hosp_presort: a sharded population, between the day's stream and its all-reduce -- every bucket of the day's bed / ICU
// events sorted in place, its map written to this shard's segment of the exchange block (hosp_walk_bucket_wave).
DAY_KERNEL __launch_bounds__(HOSP_THREADS) void k_hosp_presort(const MemberRef *M_, MemberRef one_, reina_day_t dp) {
    MEMBER_OF_LAUNCH;
    __shared__ int32_t s_hl[HL_NR][REINA_MAX_AGES];
    __shared__ SatFn s_f[2][HOSP_THREADS];
    extern __shared__ __align__(16) unsigned char smem_ps[];
    hosp_walker_block(mref_, dp, s_hl, reinterpret_cast<uint64_t *>(smem_ps), s_f, WALK_PRESORT);
    if (EXACT) {
        // exact attribution (round 6): the shard's four capacity words and the maps of its R buckets -- what a population under mirror
        // attribution all-reduces -- ride in the TRAILER of every peer's segment of the mid-day exchange (include/reina_hip.h:
        // REINA_XCHG_TRAILER_WORDS).  The workgroup of this launch that finishes last has every walker's map in front of it (its
        // acquire behind the arrival counter) and copies them; the demand words are final since k_day ended, the free words since
        // the day opened.
        const CAS DevParams *P = (const CAS DevParams *)mref_.P;
        const GBuffers B = global_buffers(mref_.B);
        __shared__ int s_last_ps;
        __threadfence();
        __syncthreads();
        if (threadIdx.x == 0) {
            const int done = atomicAdd(&B.control[REINA_L_PRESORT_DONE], 1) + 1;
            s_last_ps = done == (int)gridDim.x;
            if (s_last_ps) {
                B.control[REINA_L_PRESORT_DONE] = 0;
                __atomic_thread_fence(__ATOMIC_ACQUIRE);
            }
        }
        __syncthreads();
        if (s_last_ps) {
            const uint32_t R = P->hosp_ranges, G = P->n_shards, me = P->shard_rank;
            const GAS uint64_t *maps = hosp_exchange_maps(P, B, me);
            const uint64_t w0 = (uint64_t)(uint32_t)__hip_atomic_load(&B.pressure[REINA_PRESSURE_FREE_BEDS(me)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) |
                                ((uint64_t)(uint32_t)__hip_atomic_load(&B.pressure[REINA_PRESSURE_FREE_ICU(me)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) << 32);
            const uint64_t w1 = (uint64_t)(uint32_t)__hip_atomic_load(&B.pressure[REINA_PRESSURE_DEMAND_BEDS(me)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) |
                                ((uint64_t)(uint32_t)__hip_atomic_load(&B.pressure[REINA_PRESSURE_DEMAND_ICU(me)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) << 32);
            for (uint32_t k = threadIdx.x; k < (R + 2u) * G; k += HOSP_THREADS) {
                const uint32_t sh = k / (R + 2u), w = k - sh * (R + 2u);
                if (sh == me) continue;
                // (the maps were written by other workgroups of this launch: read past this compute unit's L1)
                xtrailer(P, B.xsend, sh)[w] = w == 0u ? w0 : w == 1u ? w1 : __hip_atomic_load(&maps[w - 2u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}
