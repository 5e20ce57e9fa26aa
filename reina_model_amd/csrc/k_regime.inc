// reina_hip.hip part: a policy and a log in one run, and the regime report (include/reina_regime.h; DESIGN.md section 6q).
// Included behind k_policy.inc, k_txlog.inc and k_course.inc: the run queues their launches and nothing of its own; the report
// is taken of a transmission log and takes its form (one engine, or a group's members at blockIdx.y: MEMBER_OF_LAUNCH).
//
// One kernel, bound by memory traffic:
//   k_regime_report  load_links<true> streams hot + log, skips a tile without an infected agent, gathers the cold record of
//                    the infected agents and hot + log of their infectors; the infector's age group costs one age_of of `src`
//                    per link.  The member's labels (at most 4096 bytes, padded to 16 with REINA_REGIME_NONE on the host, copied
//                    into the log's own device buffer ahead of the launch) come into LDS with the age tables ahead of the first
//                    __syncthreads(), 16 bytes a thread.  EVERY table is counted in LDS -- the block has none by day:
//                    5714 x 4 B, the cohorts' sums of n_infected 36 x 8 B, the labels 4096 B and the age tables 644 B,
//                    27 904 B static, so four workgroups fit a compute unit's 160 KiB -- and flushed once per workgroup
//                    (flush_lds): the flush is the kernel's only global atomic.
// One lane owns an agent; nothing but the report is written.
#include "../../include/reina_regime.h"

#define RGM_SLOTS ((uint32_t)REINA_REGIME_SLOTS)
#define RGM_NONE ((uint32_t)REINA_REGIME_MAX)                       // the slot of a day without a regime
#define RGM_SUMS (REINA_REGIME_SLOTS * REINA_REGIME_VARIANTS)       // cohort[slot][v]'s sum of n_infected, 64 bits a cell
static_assert(REINA_REGIME_REPORT_WORDS == 5714u, "report layout");
static_assert(REINA_REGIME_INFECTIONS == 9u && REINA_REGIME_COHORT == 585u && REINA_REGIME_OFFSPRING == 693u && REINA_REGIME_GENERATION == 981u &&
                  REINA_REGIME_SERIAL == 1557u && REINA_REGIME_TOST == 2709u && REINA_REGIME_LINK_PHASE == 3285u && REINA_REGIME_CROSSING == 3321u &&
                  REINA_REGIME_MIXING == 3402u && REINA_REGIME_SCALARS == 5706u,
              "report layout");
static_assert(REINA_REGIME_MAX == REINA_POLICY_MAX_LEVELS, "a policy's levels are regimes as they are");
static_assert(REINA_REGIME_MAX_GROUPS == REINA_TXLOG_MAX_GROUPS && REINA_REGIME_VARIANTS == REINA_TXLOG_VARIANTS, "the groups and variants are the log report's");
static_assert(REINA_REGIME_GENERATION_BINS == REINA_TXLOG_GENERATION_BINS && REINA_REGIME_SERIAL_BINS == REINA_TXLOG_SERIAL_BINS &&
                  REINA_REGIME_TOST_BINS == REINA_TXLOG_TOST_BINS && REINA_REGIME_PHASES == REINA_TXLOG_PHASES,
              "the intervals are the log report's");
static_assert(REINA_MAX_DAYS == 16u * REPORT_THREADS, "the labels come into LDS 16 bytes a thread");
static_assert(REINA_REGIME_REPORT_WORDS * 4u + RGM_SUMS * 8u + REINA_MAX_DAYS + sizeof(ReportAges) <= 28u * 1024u, "LDS budget of k_regime_report");

// the slot of day d, `in`: d is known and below n_days
__device__ __forceinline__ uint32_t rgm_slot(const uint8_t *lab, uint32_t d, bool in) {
    if (!in) return RGM_NONE;
    const uint32_t r = lab[d];
    return r < RGM_NONE ? r : RGM_NONE;
}

// 256 threads, tiles of 512 agents (two per thread), the workgroup's tiles strided over the grid.  labels: the members' rows
// of label_stride bytes (a multiple of 16, 16-byte aligned)
template <bool GROUP>
__global__ __launch_bounds__(REPORT_THREADS) void k_regime_report(const MemberRef *M_, const MemberRef one_, const uint32_t *log, size_t stride,
                                                                 const uint8_t *labels, uint32_t label_stride, uint64_t *report, const TxlArgs a) {
    __shared__ uint32_t s_t[REINA_REGIME_REPORT_WORDS];      // every table and the scalars, at the block's own offsets (the sums' cells stay 0)
    __shared__ unsigned long long s_sum[RGM_SUMS];           // cohort[slot][v]: the sum of n_infected
    __shared__ __attribute__((aligned(16))) uint8_t s_lab[REINA_MAX_DAYS];
    __shared__ ReportAges s_ages;
    MEMBER_OF_LAUNCH;
    const GAS uint32_t *hot = (const GAS uint32_t *)mref_.B.hot;
    const GAS reina_cold_t *cold = (const GAS reina_cold_t *)mref_.B.cold;
    const GAS uint32_t *L = member_block<GROUP>(log, stride);
    GAS unsigned long long *R = member_block<GROUP>((unsigned long long *)report, REINA_REGIME_REPORT_WORDS);
    const GAS uint8_t *lab_m = member_block<GROUP>(labels, label_stride);
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < REINA_REGIME_REPORT_WORDS; k += REPORT_THREADS) s_t[k] = 0u;
    if (tid < RGM_SUMS) s_sum[tid] = 0ull;
    {
        v4u_ q;
        q.x = q.y = q.z = q.w = 0xFFFFFFFFu;   // (beyond the member's row: no regime)
        if (16u * tid < label_stride) q = reinterpret_cast<const GAS v4u_ *>(lab_m)[tid];
        reinterpret_cast<v4u_ *>(s_lab)[tid] = q;
    }
    s_ages.load(a.p);
    __syncthreads();
    const uint32_t N = a.p.n_agents, D = a.n_days, tiles = (N + REPORT_TILE - 1u) / REPORT_TILE;
    uint32_t *s_sc = s_t + REINA_REGIME_SCALARS;
    if (blockIdx.x == 0u)   // the days by slot, once a member
        for (uint32_t d0 = 0u; d0 < D; d0 += REPORT_THREADS) wave_count(s_t, d0 + tid < D ? (int)(REINA_REGIME_DAYS + rgm_slot(s_lab, d0 + tid, true)) : -1);
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        Links l;
        if (!load_links<true>(l, t, N, hot, cold, L, s_sc, REINA_REGIME_S_INFECTED, -1, REINA_REGIME_S_LINKS, REINA_REGIME_S_BAD_LINKS)) continue;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint32_t w = l.w[j], v = RH_VARIANT(w), n = l.n[j];
            const uint32_t ti = l.lw[j] & 0xFFFFu, oi = l.lw[j] >> 16;
            const bool inf = l.inf[j], tk = inf && ti < TXL_BEFORE, ok = inf && oi < TXL_BEFORE;
            const uint32_t ts = l.sl[j] & 0xFFFFu, os = l.sl[j] >> 16;
            const bool linked = l.linked[j], tsk = linked && ts < TXL_BEFORE, osk = linked && os < TXL_BEFORE;
            const bool both = tk && tsk, in = tk && ti < D, closed = inf && RH_STATE(w) >= RS_RECOVERED;
            const uint32_t r = rgm_slot(s_lab, ti, in), rs = rgm_slot(s_lab, ts, tsk && ts < D);
            int g = 0, gs = 0;
            if (inf) g = s_ages.group_of(l.idx[j]);
            if (linked) gs = s_ages.group_of((uint32_t)l.src[j]);
            // the scalars beyond load_links' three
            wave_tally(&s_sc[REINA_REGIME_S_DATED], tk);
            wave_tally(&s_sc[REINA_REGIME_S_IN_RANGE], in);
            wave_tally(&s_sc[REINA_REGIME_S_UNLABELLED], in && r == RGM_NONE);
            wave_tally(&s_sc[REINA_REGIME_S_LINKS_DATED], both);
            wave_tally(&s_sc[REINA_REGIME_S_LINKS_CROSSING], linked && r < RGM_NONE && rs < RGM_NONE && r != rs);
            // the agent by the regime it was infected under
            const int cv = (int)(r * REINA_REGIME_VARIANTS + v);
            wave_count(s_t, inf ? (int)REINA_REGIME_INFECTIONS + cv * REINA_REGIME_MAX_GROUPS + g : -1);
            const int ck = (int)REINA_REGIME_COHORT + cv * REINA_REGIME_COHORT_FIELDS;
            wave_count(s_t, inf ? ck : -1);
            if (inf && n) atomicAdd(&s_sum[cv], (unsigned long long)n);
            wave_count(s_t, closed ? ck + 2 : -1);
            wave_count(s_t, closed ? (int)(REINA_REGIME_OFFSPRING + r * REINA_REGIME_OFFSPRING_BINS + (n < REINA_REGIME_OFFSPRING_BINS - 1u ? n : REINA_REGIME_OFFSPRING_BINS - 1u))
                                   : -1);
            // the link by the regime at transmission
            wave_count(s_t, both ? (int)(REINA_REGIME_GENERATION + r * REINA_REGIME_GENERATION_BINS) + txl_clip((int)ti - (int)ts, REINA_REGIME_GENERATION_BINS - 1) : -1);
            wave_count(s_t, ok && osk ? (int)(REINA_REGIME_SERIAL + r * REINA_REGIME_SERIAL_BINS) +
                                          txl_clip((int)oi - (int)os + REINA_TXLOG_SERIAL_SHIFT, REINA_REGIME_SERIAL_BINS - 1)
                                    : -1);
            wave_count(s_t, tk && osk ? (int)(REINA_REGIME_TOST + r * REINA_REGIME_TOST_BINS) +
                                          txl_clip((int)ti - (int)os + REINA_TXLOG_TOST_SHIFT, REINA_REGIME_TOST_BINS - 1)
                                    : -1);
            const uint32_t phase = tk && osk ? (ti < os ? 0u : 1u) : (tk && os == TXL_NONE ? 2u : 3u);
            wave_count(s_t, linked ? (int)(REINA_REGIME_LINK_PHASE + r * REINA_REGIME_PHASES + phase) : -1);
            wave_count(s_t, linked ? (int)(REINA_REGIME_CROSSING + rs * RGM_SLOTS + r) : -1);
            wave_count(s_t, linked ? (int)(REINA_REGIME_MIXING + (r * REINA_REGIME_MAX_GROUPS + (uint32_t)gs) * REINA_REGIME_MAX_GROUPS) + g : -1);
        }
    }
    __syncthreads();
    flush_lds(s_t, REINA_REGIME_REPORT_WORDS, R);
    if (tid < RGM_SUMS && s_sum[tid]) atomicAdd(&R[REINA_REGIME_COHORT + tid * REINA_REGIME_COHORT_FIELDS + 1u], s_sum[tid]);
}

// ---------------------------------------------------------------------------------------------
// host side

// a policy and a log as one attachment of a run: `before` is the policy's launch, `after` the log's
struct regime_pair : attachment {
    reina_policy *p = nullptr;
    reina_txlog *l = nullptr;
};
static int regime_before_day(attachment *a, const reina_day_t &d, hipStream_t s) { return policy_launch_day(static_cast<regime_pair *>(a)->p, d, s); }
static int regime_after_day(attachment *a, const reina_day_t &d, hipStream_t s) { return txlog_launch_day(static_cast<regime_pair *>(a)->l, d.day, s); }

// what both run entry points refuse before a day is queued
static int regime_check_run(const reina_policy *p, const reina_txlog *l, const reina_day_t *days, uint32_t n_days, bool group, const char *what) {
    const std::string w(what);
    if (!p || !l) return refuse(w + ": a null policy or log");
    if (!days) return refuse(w + ": a null day list");
    if ((p->g != nullptr) != (l->g != nullptr)) return refuse(w + ": the policy and the log are not of one kind (one was made for an engine, the other for a group)");
    if (int rc = attachment_kind(p, group, what)) return rc;
    if (p->g != l->g || p->members != l->members) return refuse(w + ": the policy and the log were made for different engines or groups");
    return policy_check_days(days, n_days);   // (the log's own limit is the same one: attachment_check_day)
}

// page-locked blocks the labels of a call are written to: one ring for the process (a report owns nothing)
static std::mutex g_regime_stage_mu;
static StageRing g_regime_stages;
static const size_t REGIME_MAX_STAGES = 4;

static int regime_report(reina_txlog *l, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days, const uint8_t *labels, uint64_t *dev_report, hipStream_t s) {
    // day_report's checks in its order, then the labels: a refused call queues nothing
    TxlArgs a;
    if (int rc = day_report_args(l, "regime report", REINA_REGIME_MAX_GROUPS, age_group, n_groups, n_days, dev_report, &a)) return rc;
    if (!labels) return refuse("regime report: labels is null");
    const size_t K = l->members.size(), row = ((size_t)n_days + 15u) & ~(size_t)15u;
    if (row * K > REINA_REGIME_STAGE_BYTES) return refuse("regime report: members x n_days is beyond REINA_REGIME_STAGE_BYTES");
    for (size_t k = 0; k < K * n_days; k++)
        if (labels[k] >= REINA_REGIME_MAX && labels[k] != REINA_REGIME_NONE)
            return refuse("regime report: a label is neither below REINA_REGIME_MAX nor REINA_REGIME_NONE");
    // (the log's label buffer is made once, by its first report)
    if (!l->d_labels) HIP_CHECK(hipMalloc(&l->d_labels, (size_t)REINA_MAX_DAYS * K));
    {
        // staged in page-locked memory and copied once to the device: the workgroups read their member's row from HBM
        std::lock_guard<std::mutex> lock(g_regime_stage_mu);
        void *block = nullptr, *dsrc = nullptr;
        if (int rc = g_regime_stages.acquire(REINA_REGIME_STAGE_BYTES, REGIME_MAX_STAGES, &block, &dsrc)) return rc;
        std::memset(block, 0xFF, row * K);
        for (size_t m = 0; m < K; m++) std::memcpy(static_cast<char *>(block) + row * m, labels + (size_t)n_days * m, n_days);
        HIP_CHECK(hipMemcpyAsync(l->d_labels, block, row * K, hipMemcpyHostToDevice, s));
        if (int rc = g_regime_stages.release_behind(s)) return rc;
    }
    return day_report_queue(l, REINA_REGIME_REPORT_WORDS, a, dev_report, s, [&](const TxlArgs &args, uint32_t grid, uint32_t members) -> int {
        launch_members(k_regime_report, l->g, grid, members, REPORT_THREADS, s, l->d_refs, l->e0->h_ref, l->d_log, l->stride,
                       static_cast<const uint8_t *>(l->d_labels), (uint32_t)row, dev_report, args);
        return REINA_OK;
    });
}

extern "C" {

int reina_regime_version(void) { return REINA_REGIME_VERSION; }

int reina_policy_txlog_run_days(reina_policy_t *p, reina_txlog_t *log, const reina_day_t *days, uint32_t n_days, int32_t *history_base, void *stream) {
    if (int rc = regime_check_run(p, log, days, n_days, false, "reina_policy_txlog_run_days")) return rc;
    if (int rc = policy_begin_run(p)) return rc;
    regime_pair pair;
    pair.p = p, pair.l = log;
    const int rc = engine_run_days(p->e0, days, n_days, history_base, stream, day_hooks{&pair, regime_before_day, regime_after_day});
    policy_end_run(p);
    return rc;
}

int reina_group_policy_txlog_run_days(reina_policy_t *p, reina_txlog_t *log, const reina_day_t *days, uint32_t n_days, int32_t *const *history_bases,
                                      void *stream) {
    if (int rc = regime_check_run(p, log, days, n_days, true, "reina_group_policy_txlog_run_days")) return rc;
    if (int rc = policy_begin_run(p)) return rc;
    regime_pair pair;
    pair.p = p, pair.l = log;
    const int rc = group_run_days(p->g, days, n_days, history_bases, stream, day_hooks{&pair, regime_before_day, regime_after_day});
    policy_end_run(p);
    return rc;
}

int reina_regime_report(reina_txlog_t *log, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days, const uint8_t *labels, uint64_t *dev_report,
                        void *stream) {
    if (!log) return refuse("reina_regime_report: a null log");
    if (int rc = attachment_kind(log, false, "reina_regime_report")) return rc;
    return regime_report(log, age_group, n_groups, n_days, labels, dev_report, (hipStream_t)stream);
}

int reina_group_regime_report(reina_txlog_t *log, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days, const uint8_t *labels, uint64_t *dev_report,
                              void *stream) {
    if (!log) return refuse("reina_group_regime_report: a null log");
    if (int rc = attachment_kind(log, true, "reina_group_regime_report")) return rc;
    return regime_report(log, age_group, n_groups, n_days, labels, dev_report, (hipStream_t)stream);
}

}  // extern "C"
