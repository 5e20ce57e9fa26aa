// reina_hip.hip part: test queue, contact tracing, and k_open (opening + imports + testing in one launch).
// Included by reina_hip.hip only (one translation unit); not a standalone header.
// ---------------------------------------------------------------------------------------------
// testing queue + contact tracing (HealthcareSystem.iterate main.pyx:514-545,
// perform_contact_tracing :495-512, queue_for_testing :474-488)

__device__ __forceinline__ void queue_append(const CAS DevParams *P, const GBuffers &B, int which, uint32_t idx) {
    uint32_t pos = wave_alloc(&B.control[which ? REINA_L_QUEUE1 : REINA_L_QUEUE0]);
    if (pos >= P->max_queue) {
        set_problem(B.counters, REINA_PROBLEM_QUEUE_OVERFLOW);
        return;
    }
    (which ? B.queue1 : B.queue0)[pos] = idx;
}

// Q1: every queued test is positive (quirk Q8): clear QUEUED, set DETECTED
struct OpenTraceLds;   // (below)
__device__ __forceinline__ void test_detect_block(const MemberRef &mref_, const reina_day_t &dp, uint32_t bx, uint32_t nbx, unsigned char *lds) {
    const CAS DevParams *P = (const CAS DevParams *)mref_.P;
    const GBuffers B = global_buffers(mref_.B);  // by value: pointers live in SGPRs, never re-read after stores
    int32_t *s_det = reinterpret_cast<int32_t *>(lds);                  // [REINA_MAX_AGES]
    int32_t *s_age_start = s_det + REINA_MAX_AGES;                      // [REINA_MAX_AGES + 1]
    const int cur = dp.day & 1;
    const GAS uint32_t *q = cur ? B.queue1 : B.queue0;
    const int n = B.control[cur ? REINA_L_QUEUE1 : REINA_L_QUEUE0];
    const uint32_t ch_sh = (uint32_t)n > blockDim.x ? 6u : (uint32_t)__builtin_ctz(blockDim.x), ch = 1u << ch_sh;   // a long queue a wave at a time over the workgroups (test_trace_block)
    if (n <= (int)(bx * ch)) return;
    if (threadIdx.x <= REINA_MAX_AGES) s_age_start[threadIdx.x] = P->age_start[threadIdx.x];
    if (threadIdx.x < REINA_MAX_AGES) s_det[threadIdx.x] = 0;
    __syncthreads();
    for (uint32_t c = bx + nbx * (threadIdx.x >> ch_sh);; c += nbx * (blockDim.x >> ch_sh)) {
        const uint32_t k = c * ch + (threadIdx.x & (ch - 1u));
        if (c * ch >= (uint32_t)n) break;
        if (k >= (uint32_t)n) continue;
        uint32_t i = q[k];
        uint32_t w = B.hot[i];
        if (w & RH_DETECTED) set_problem(B.counters, 7 /* WRONG_STATE */);
        B.hot[i] = (w & ~RH_QUEUED) | RH_DETECTED;
        atomicAdd(&s_det[age_of(s_age_start, i, 0, (int)P->nr_ages - 1)], 1);
    }
    // hot words, queues and lists are free to touch from the first instruction of the launch; the detection COUNTERS are
    // not (the opening workgroup snapshots and zeroes them meanwhile): the day's detections by age go to a side block of the
    // control words that the day's last launch folds into the counters (k_install.inc) -- no waiting for the opening
    __syncthreads();
    if (threadIdx.x < REINA_MAX_AGES && s_det[threadIdx.x]) atomicAdd(&B.control[REINA_L_DET_SIDE + threadIdx.x], s_det[threadIdx.x]);
}

// the tracing success roll is keyed by (candidate, tracer): the SET of queued agents is order-free
// (in two halves so that a lane can have the word loads, and then the flag updates, of two
// candidates in flight together)
__device__ __forceinline__ bool trace_wants(const CAS DevParams *P, uint32_t cand, uint32_t cand_word, uint32_t tracer,
                                            const reina_day_t &dp) {
    if (RH_STATE(cand_word) == RS_DEAD || (cand_word & (RH_DETECTED | RH_QUEUED))) return false;
    rp_u4 r = rp_philox(P->k0, P->k1, cand, dp.day, RP_P_TRACE, tracer);
    return rp_chance(dp.p_successful_tracing, r.v[0]) != 0;
}
__device__ __forceinline__ bool try_queue(const CAS DevParams *P, const GBuffers &B, uint32_t cand,
                                          uint32_t tracer, const reina_day_t &dp) {
    if (!trace_wants(P, cand, ld_hot(&B.hot[cand]), tracer, dp)) return false;
    uint32_t old = atomicOr(&B.hot[cand], RH_QUEUED);
    return !(old & RH_QUEUED);
}

// level 0 (from the detected queue, accepted candidates also go to the level-1 list) and
// level 1 (from the level-1 list, no further recursion)
// Level 0 also performs the detection of its queue entry (k_test_detect's job) in the same pass:
// every member of today's queue carries QUEUED until its single store replaces it with DETECTED,
// so a tracer can never re-queue another member, whichever of the two runs first.
#define TRACE_STAGE 4096
// successes of a workgroup are staged in LDS and appended to the global lists with ONE allocation
// per list at the end (a returning global atomic per success would sit in every lane's dependent
// chain); overflow of the stage falls back to direct appends
struct TraceStage {
    uint32_t n;
    uint32_t base_q, base_l;
    uint32_t item[TRACE_STAGE];
};
template <int LEVEL>
__device__ __forceinline__ void trace_accept(const CAS DevParams *P, const GBuffers &B, TraceStage &S, int nxt, uint32_t cand) {
    const uint32_t pos = atomicAdd(&S.n, 1u);
    if (pos < TRACE_STAGE) {
        S.item[pos] = cand;
        return;
    }
    queue_append(P, B, nxt, cand);
    if (LEVEL == 0) {
        uint32_t p1 = wave_alloc(&B.control[REINA_L_LEVEL1]);
        if (p1 < P->max_queue) B.level1[p1] = cand; else set_problem(B.counters, REINA_PROBLEM_QUEUE_OVERFLOW);
    }
}

struct OpenTraceLds {
    int32_t s_det[REINA_MAX_AGES];
    int32_t s_age_start[REINA_MAX_AGES + 1];
    int s_last;
    TraceStage S;
};
template <int LEVEL, bool X>
__device__ __forceinline__ void test_trace_block(const MemberRef &mref_, const reina_day_t &dp, uint32_t bx, uint32_t nbx, unsigned char *lds,
                                                 int FOLD = 0) {
    const ParamsX<X> P{(const CAS DevParams *)mref_.P};
    const GBuffers B = global_buffers(mref_.B);  // by value: pointers live in SGPRs, never re-read after stores
    OpenTraceLds &TL = *reinterpret_cast<OpenTraceLds *>(lds);
    int32_t *s_det = TL.s_det, *s_age_start = TL.s_age_start;
    TraceStage &S = TL.S;
    const int cur = dp.day & 1, nxt = cur ^ 1;
    const GAS uint32_t *src = LEVEL == 0 ? (cur ? B.queue1 : B.queue0) : B.level1;
    // (the level-1 list may have been written by this very launch: its length is read past this XCD's L2)
    const int n = LEVEL == 0 ? B.control[cur ? REINA_L_QUEUE1 : REINA_L_QUEUE0]
                             : __hip_atomic_load(&B.control[REINA_L_LEVEL1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // The list is dealt out in chunks of `ch` entries, chunk c to workgroup c mod nbx: a long list one WAVE at a time, so
    // that its scattered reads start on as many CUs as there are waves of work.  (Measured, round 3: with 1024 consecutive
    // entries per workgroup the 3000 entries of a day at 10^8 agents sat on three CUs, and the first hop of the loop below
    // -- four scattered lines per lane -- took 14 us where one such read takes 2.6 us, tools/ubench_scatter.hip: a CU keeps
    // only so many misses in flight.)  A short list stays with one workgroup, which then walks level 1 without a fence.
    const uint32_t ch_sh = (uint32_t)n > blockDim.x ? 6u : (uint32_t)__builtin_ctz(blockDim.x), ch = 1u << ch_sh;   // (block sizes are powers of two)
    if (n <= (int)(bx * ch)) return;
    DIAG_CLOCK(OPEN, os_t);   // (-DREINA_OPEN_STAMPS: this workgroup's phases, and its slowest wave's way through an entry)
    if (LEVEL == 0) {
        if (threadIdx.x <= REINA_MAX_AGES) s_age_start[threadIdx.x] = P->age_start[threadIdx.x];
        if (threadIdx.x < REINA_MAX_AGES) s_det[threadIdx.x] = 0;
    }
    if (threadIdx.x == 0) S.n = 0;
    __syncthreads();
    for (uint32_t c = bx + nbx * (threadIdx.x >> ch_sh);; c += nbx * (blockDim.x >> ch_sh)) {
        const uint32_t k = c * ch + (threadIdx.x & (ch - 1u));
        if (c * ch >= (uint32_t)n) break;     // (uniform over a chunk: a wave leaves the loop as one)
        if (k >= (uint32_t)n) continue;
        const uint32_t i = src[k];
        DIAG_SINCE(TRACE, LEVEL ? DIAG_TRACE_L1_ENTRY : DIAG_TRACE_L0_ENTRY, DIAG_WAVE_LANE0, os_t, B.mirror);
        // everything that depends only on i is requested together: its word, its record (infector, head of the overflow
        // list) and its block of inline infectee slots -- three accesses, one round trip
        const int32_t inf = B.cold[i].infector;
        int32_t over = B.cold[i].first_infectee;
        const GAS v4u_ *slots = reinterpret_cast<const GAS v4u_ *>(B.infectees + (size_t)i * REINA_INLINE_INFECTEES);
        const v4u_ s_lo = slots[0], s_hi = slots[1];
        uint32_t wi;
        if (LEVEL == 0) {
            const uint32_t w0 = B.hot[i];
            if (w0 & RH_DETECTED) set_problem(B.counters, 7 /* WRONG_STATE */);
            wi = (w0 & ~RH_QUEUED) | RH_DETECTED;
            B.hot[i] = wi;
            atomicAdd(&s_det[age_of(s_age_start, i, 0, (int)P->nr_ages - 1)], 1);
        } else {
            wi = ld_hot(&B.hot[i]);
        }
        // the infector and the inline infectees (perform_contact_tracing, main.pyx:495-512).  queue_for_testing (:474-488)
        // rejects a dead, detected or already queued person, else rolls for success -- here the ROLL comes first (it is keyed
        // by (candidate, tracer): the candidate's word is not needed for it) and a success sets the QUEUED flag at once; the
        // word the atomic returns then says whether the candidate was eligible.  If not (dead or detected, not queued) the flag
        // is taken back; nobody can have acted on it meanwhile: another tracer that saw it would have been refused by the same
        // word, and a candidate is never susceptible (the import placement's compare-and-swap never meets it).  One round
        // trip instead of two (read the word, then set the flag) on the longest chain of the day's opening.
        const bool has = (wi & RH_HASLIST) != 0u;
        if (!has) over = -1;
        int32_t cand[1 + REINA_INLINE_INFECTEES];
        cand[0] = inf;
        cand[1] = has ? (int32_t)s_lo.x : -1; cand[2] = has ? (int32_t)s_lo.y : -1;
        cand[3] = has ? (int32_t)s_lo.z : -1; cand[4] = has ? (int32_t)s_lo.w : -1;
        cand[5] = has ? (int32_t)s_hi.x : -1; cand[6] = has ? (int32_t)s_hi.y : -1;
        cand[7] = has ? (int32_t)s_hi.z : -1; cand[8] = has ? (int32_t)s_hi.w : -1;
        DIAG_SINCE(TRACE, LEVEL ? DIAG_TRACE_L1_RECORD : DIAG_TRACE_L0_RECORD, DIAG_WAVE_LANE0, os_t, B.mirror);
        // (the candidates are GLOBAL ids where the population keeps them -- exact attribution: one that lives on another shard
        // becomes a request to its owner, which rolls with the same key, (candidate, tracer's global id); k_xtrace below)
        const uint32_t tracer = (uint32_t)gid_of(P, i);
        if (IS_EXACT(P)) {
            // (one copy of the push, walked slot by slot: an unsharded engine's launch jumps over it)
#pragma unroll 1
            for (int q = 0; q <= REINA_INLINE_INFECTEES; q++) {
                int32_t g = cand[0];
#pragma unroll
                for (int z = 1; z <= REINA_INLINE_INFECTEES; z++) g = q == z ? cand[z] : g;
                if (g >= 0 && !gid_local(P, g)) xsend_push(P, B, rp_gid_shard((uint32_t)g), rp_xrec(gid_index(P, g), 0u, tracer));
            }
        }
        bool want[1 + REINA_INLINE_INFECTEES];
#pragma unroll
        for (int q = 0; q <= REINA_INLINE_INFECTEES; q++) {
            const bool here = cand[q] >= 0 && gid_local(P, cand[q]);
            cand[q] = here ? (int32_t)gid_index(P, cand[q]) : -1;
            want[q] = here && rp_chance(dp.p_successful_tracing, rp_philox(P->k0, P->k1, (uint32_t)cand[q], dp.day, RP_P_TRACE, tracer).v[0]) != 0;
        }
        uint32_t old_w[1 + REINA_INLINE_INFECTEES];
#pragma unroll
        for (int q = 0; q <= REINA_INLINE_INFECTEES; q++) old_w[q] = want[q] ? atomicOr(&B.hot[cand[q]], RH_QUEUED) : RH_QUEUED;
#pragma unroll
        for (int q = 0; q <= REINA_INLINE_INFECTEES; q++) {
            if (old_w[q] & RH_QUEUED) continue;                                  // no roll, no success, or queued already
            if (RH_STATE(old_w[q]) == RS_DEAD || (old_w[q] & RH_DETECTED))
                atomicAnd(&B.hot[cand[q]], ~RH_QUEUED);                          // not eligible: the flag is taken back
            else
                trace_accept<LEVEL>(P, B, S, nxt, (uint32_t)cand[q]);
        }
        DIAG_SINCE(TRACE, LEVEL ? DIAG_TRACE_L1_FLAGS : DIAG_TRACE_L0_FLAGS, DIAG_WAVE_LANE0, os_t, B.mirror);
        // infectees beyond the inline slots (an agent that infected more than REINA_INLINE_INFECTEES others): the linked list --
        // through the infectees' own records, or (exact attribution) through the nodes of the pool
        int32_t sib = over;
        while (sib >= 0) {
            int32_t next, g = sib;
            if (IS_EXACT(P)) {
                g = (int32_t)B.infectee_pool[2u * (uint32_t)sib];
                next = (int32_t)B.infectee_pool[2u * (uint32_t)sib + 1u];
            } else {
                next = B.cold[sib].next_sibling;   // requested beside the candidate's hot word
            }
            if (!gid_local(P, g)) xsend_push(P, B, rp_gid_shard((uint32_t)g), rp_xrec(gid_index(P, g), 0u, tracer));
            else if (try_queue(P, B, gid_index(P, g), tracer, dp)) trace_accept<LEVEL>(P, B, S, nxt, gid_index(P, g));
            sib = next;
        }
        DIAG_SINCE(TRACE, LEVEL ? DIAG_TRACE_L1_OVERFLOW : DIAG_TRACE_L0_OVERFLOW, DIAG_WAVE_LANE0, os_t, B.mirror);
    }
    __syncthreads();
    {   // one allocation per list for the whole workgroup, then coalesced copies out of LDS
        const uint32_t cnt = S.n < TRACE_STAGE ? S.n : TRACE_STAGE;
        if (threadIdx.x == 0 && cnt) {
            S.base_q = (uint32_t)atomicAdd(&B.control[nxt ? REINA_L_QUEUE1 : REINA_L_QUEUE0], (int)cnt);
            if (LEVEL == 0) S.base_l = (uint32_t)atomicAdd(&B.control[REINA_L_LEVEL1], (int)cnt);
        }
        __syncthreads();
        if (cnt) {
            GAS uint32_t *q = nxt ? B.queue1 : B.queue0;
            if (S.base_q + cnt > P->max_queue || (LEVEL == 0 && S.base_l + cnt > P->max_queue)) {
                if (threadIdx.x == 0) set_problem(B.counters, REINA_PROBLEM_QUEUE_OVERFLOW);
            } else {
                for (uint32_t k = threadIdx.x; k < cnt; k += blockDim.x) {
                    const uint32_t x = S.item[k];
                    q[S.base_q + k] = x;
                    if (LEVEL == 0) B.level1[S.base_l + k] = x;
                }
            }
        }
    }
    DIAG_LAP(OPEN, LEVEL ? DIAG_OPEN_LEVEL1 : DIAG_OPEN_LEVEL0, DIAG_THREAD0, os_t, B.mirror);
    if (LEVEL == 0) {
        // the day's detections by age: to the side block the day's last launch folds into the counters (no waiting for the
        // opening workgroup's snapshot + zeroing: that wait was 5 us of every contact-tracing day at 10^8 agents)
        if (threadIdx.x < REINA_MAX_AGES && s_det[threadIdx.x]) atomicAdd(&B.control[REINA_L_DET_SIDE + threadIdx.x], s_det[threadIdx.x]);
        DIAG_LAP(OPEN, DIAG_OPEN_DETECTIONS, DIAG_THREAD0, os_t, B.mirror);
    }
    if (LEVEL == 0 && FOLD == 1) {
        // small populations: the level-0 workgroup that finishes last walks the level-1 list itself
        // (a few hundred entries) instead of a launch of its own
        int &s_last = TL.s_last;
        uint32_t busy = ((uint32_t)n + ch - 1) / ch;   // workgroups that had queue entries
        if (busy > nbx) busy = nbx;
        if (busy == 1) {
            __syncthreads();   // the only one: its own list writes are visible to itself
            DIAG_LAP(OPEN, DIAG_OPEN_ARRIVAL, DIAG_THREAD0, os_t, B.mirror);
            test_trace_block<1, X>(mref_, dp, 0, 1, lds);
            return;
        }
        __threadfence();
        __syncthreads();
        if (threadIdx.x == 0) {
            const int done = atomicAdd(&B.control[REINA_L_TRACE_DONE], 1) + 1;
            s_last = done == (int)busy;
            if (s_last) {
                B.control[REINA_L_TRACE_DONE] = 0;
                __atomic_thread_fence(__ATOMIC_ACQUIRE);   // see the other workgroups' list entries and flags
            }
        }
        __syncthreads();
        DIAG_LAP(OPEN, DIAG_OPEN_ARRIVAL, DIAG_THREAD0, os_t, B.mirror);
        if (s_last) test_trace_block<1, X>(mref_, dp, 0, 1, lds);
    }
    // (Measured dead end, round 3, twice: for a large population, level 1 shared by all the level-0 workgroups of this launch
    // behind a barrier -- arrival counter, bounded wait -- instead of a launch of its own.  With level 0 on three workgroups the
    // barrier waited 9 us for the slowest of them and the level-1 pass took 11 us behind it, against 8.5 us for the separate
    // launch; with the lists dealt out by the wave (level 0: 8 us) the opening launch still grew by 10 us at 10^8 agents and
    // by 10 us at 5 x 10^7 where the level-1 launch costs 7: the day went from 0.188 to 0.193 ms.  A third time with the polled
    // words (arrival counters, the day-open flag) moved to cache lines of their own, away from the queue counters and tickets:
    // the same 10 us, and nothing gained for the launches as they are either.)
}

DAY_KERNEL __launch_bounds__(256) void k_test_trace1(const MemberRef *M_, MemberRef one_, reina_day_t dp) {
    MEMBER_OF_LAUNCH;
    __shared__ __align__(16) unsigned char s_lds[sizeof(OpenTraceLds)];
    test_trace_block<1, EXACT>(mref_, dp, blockIdx.x, gridDim.x, s_lds);
}

// exact attribution: the tracing requests the other shards sent for candidates of this one (one launch per level, behind the
// level's exchange): queue_for_testing (main.pyx:474-488) with the roll the tracer's shard would have made -- keyed by
// (candidate, tracer's global id) --, a level-0 success also joins the level-1 list.  Then the segments are emptied for
// the next exchange.
DAY_KERNEL __launch_bounds__(256) void k_xtrace(const MemberRef *M_, MemberRef one_, reina_day_t dp, int level) {
    MEMBER_OF_LAUNCH;
    const CAS DevParams *P = (const CAS DevParams *)mref_.P;
    const GBuffers B = global_buffers(mref_.B);
    __shared__ uint32_t s_xpre[REINA_MAX_SHARDS + 1];
    xrecv_prefix(P, B, s_xpre);
    __syncthreads();
    const uint32_t total = s_xpre[P->n_shards];
    const int nxt = (dp.day & 1) ^ 1;
    for (uint32_t base = blockIdx.x * blockDim.x; base < total; base += gridDim.x * blockDim.x) {   // (a wave stays together: wave_alloc)
        const uint32_t idx = base + threadIdx.x;
        bool ok = false;
        uint32_t c = 0;
        if (idx < total) {
            uint32_t from;
            const uint64_t rec = xrecv_record(P, B, s_xpre, idx, &from);
            c = rp_xrec_index(rec);
            ok = c < P->n_agents && try_queue(P, B, c, rp_xrec_gid(rec), dp);
        }
        if (ok) {
            queue_append(P, B, nxt, c);
            if (level == 0) {
                const uint32_t p1 = wave_alloc(&B.control[REINA_L_LEVEL1]);
                if (p1 < P->max_queue) B.level1[p1] = c; else set_problem(B.counters, REINA_PROBLEM_QUEUE_OVERFLOW);
            }
        }
    }
    xsend_reset(P, B);
}

// exact attribution: the feedback records of the day's cross-shard infections -- the sources that live here take their
// infectees (person_infect's source half, main.pyx:219-233), so that counts and lists are true before the next morning
DAY_KERNEL __launch_bounds__(256) void k_feedback(const MemberRef *M_, MemberRef one_, reina_day_t dp) {
    MEMBER_OF_LAUNCH;
    const ParamsX<true> P{(const CAS DevParams *)mref_.P};   // (launched under exact attribution only)
    const GBuffers B = global_buffers(mref_.B);
    __shared__ uint32_t s_xpre[REINA_MAX_SHARDS + 1];
    xrecv_prefix(P, B, s_xpre);
    __syncthreads();
    const uint32_t total = s_xpre[P->n_shards];
    for (uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += gridDim.x * blockDim.x) {
        uint32_t from;
        const uint64_t rec = xrecv_record(P, B, s_xpre, idx, &from);
        if (rp_xrec_index(rec) < P->n_agents)
            source_gains_infectee(P, B, rp_xrec_index(rec), (int32_t)rp_xrec_gid(rec), rp_xrec_flags(rec) >> 2);
    }
    xsend_reset(P, B);
    (void)dp;
}

// The day-opening roles.  role 0 opens the day (prologue_block: snapshot, beds, intervention imports, daily zeroing),
// role 1 places the weekly imports, roles 2.. work off the test queue (mode 1: detection only, 2: detection + level-0
// contact tracing, 3: the same with level 1 walked by the workgroup that finishes last; mode 0: no testing yet, two roles).  The import placement
// touches only never-infected agents and infection counters, the test queue only infected agents and detection
// counters, so all of them start at once; only their COUNTER updates wait until the opening role signals that the
// snapshot and the daily zeroing are done (wait_day_open).  `lds`: sizeof(OpenLds) bytes of the workgroup's LDS.
union OpenLds {
    OpenImportsLds imports;
    OpenTraceLds trace;
};
template <bool X>
__device__ __forceinline__ void open_role(const MemberRef &mref_, const reina_day_t &dp, uint32_t hist_slot, int weekly_own, int mode,
                                          uint32_t role, uint32_t n_roles, unsigned char *lds) {
    // weekly_own > 0: that many workgroups (roles 1..) place the weekly imports between them, beside the opening.
    // weekly_own <= 0: the day has intervention imports, placed before the daily zeroing, and the weekly ones follow behind
    // them under the same claim keys: the opening workgroup does both, sharing them with -weekly_own helpers (roles 1..; none:
    // role 1 idles)
    // weekly_own == OPEN_WEEKLY_IN_STREAM: the weekly imports are placed in k_day's launch, beside the stream (k_open.inc:
    // day_imports_block); nothing of them here
    const bool in_stream = weekly_own == OPEN_WEEKLY_IN_STREAM;
    const uint32_t helpers = in_stream ? 0u : weekly_own > 0 ? (uint32_t)weekly_own : (uint32_t)-weekly_own;
    const uint32_t first_test = 1u + (helpers > 1u ? helpers : 1u);
    if (role == 0) {
        prologue_block(mref_, dp, hist_slot, weekly_own > 0, weekly_own < 0 ? helpers + 1u : 1u, lds);
    } else if (role < first_test) {
        if (in_stream) { }
        else if (weekly_own > 0) weekly_imports_block(mref_, dp, lds, role - 1u, helpers);
        else if (weekly_own < 0) weekly_imports_block(mref_, dp, lds, role, helpers + 1u, true);
    } else if (mode == 1) {
        test_detect_block(mref_, dp, role - first_test, n_roles - first_test, lds);
    } else if (mode == 2) {
        test_trace_block<0, X>(mref_, dp, role - first_test, n_roles - first_test, lds, 0);
    } else if (mode == 3) {
        test_trace_block<0, X>(mref_, dp, role - first_test, n_roles - first_test, lds, 1);
    }
}

// k_open: the day's opening as a launch of its own (days with a vaccination programme, whose pass over the agents
// must come between the test queue and the stream; otherwise the roles ride in k_day's launch).  Roles are handed out
// by ARRIVAL: every workgroup takes a ticket from a per-engine counter, so the opening role is by construction one
// that is already running when any other workgroup starts to wait for it: nothing depends on the order in which the
// dispatcher starts workgroups, nor on all of them being resident together (HIP promises neither; engine groups
// launch up to 128 x 66 workgroups of 1024 threads).  The workgroup that takes the launch's last ticket resets the
// counter for the next launch.
// `tickets` = 0 (round 4): a single engine's launch of at most one workgroup per compute unit is resident as a whole -- every
// workgroup runs from the start, whichever the dispatcher starts first --, so the role is the block number and the
// returning atomic of the ticket (a round trip to L2 in front of every workgroup's first useful instruction) is saved.
// (Were a workgroup started late after all, the others' waits are bounded polls that flag the day: REINA_PROBLEM_SYNC_TIMEOUT.)
DAY_KERNEL __launch_bounds__(PRO_THREADS) void k_open(const MemberRef *M_, MemberRef one_, reina_day_t dp, uint32_t hist_slot, int weekly_own, int mode,
                                                      int tickets) {
    MEMBER_OF_LAUNCH;
    __shared__ __align__(16) unsigned char s_lds[sizeof(OpenLds)];
    __shared__ uint32_t s_role;
    uint32_t role = blockIdx.x;
    if (tickets) {
        if (threadIdx.x == 0) {
            GAS int32_t *ctl = (GAS int32_t *)mref_.B.control;
            const int t = atomicAdd(&ctl[REINA_L_OPEN_TICKET], 1);
            if (t == (int)gridDim.x - 1) ctl[REINA_L_OPEN_TICKET] = 0;   // every ticket of this launch is out
            s_role = (uint32_t)t;
        }
        __syncthreads();
        role = s_role;
    }
    open_role<EXACT>(mref_, dp, hist_slot, weekly_own, mode, (uint32_t)__builtin_amdgcn_readfirstlane((int)role), gridDim.x, s_lds);
}
