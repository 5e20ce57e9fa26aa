// reina_hip.hip part: the dated transmission log (include/reina_txlog.h; DESIGN.md section 6f).
// Included at the end of reina_hip.hip (it uses the host helpers, the group and k_addons.inc above).
//
// Three kernels, each bound by memory traffic:
//   k_txlog_begin   streams the hot words (16 bytes a lane) and writes every log word.
//   k_txlog_day     ONE launch a day, queued behind the day's last launch.  It streams the ACTIVE bit plane (N / 8 bytes), one
//                   512-agent tile a wave (k_addons.inc's active_tile has the geometry).  Two forms of the update, chosen per
//                   launch:
//                     by_hot = 0  reads the log word of every active agent and applies the definition to it;
//                     by_hot = 1  decides from the hot word alone -- INCUBATION with the day in bits 24-31: the agent was infected
//                                 today, a full-word store; ILLNESS with day + 1 there: its onset was today, a 16-bit store of the
//                                 upper half -- and never reads the log.  tests/test_txlog.py keeps checked, on oracle B, that
//                                 the two coincide on simulated states.  The host takes by_hot = 0 on the first day a log
//                                 records and on any day that does not follow the last one recorded: the agents an initial
//                                 condition leaves incubating carry day 0 in bits 24-31 and are BEFORE, not "infected on day 0".
//   k_txlog_report  streams hot + log, gathers the cold record of infected agents and hot + log of their infectors; the interval
//                   histograms (wave_count) and the scalars (wave_tally) are counted in LDS and flushed once per workgroup; the
//                   tables indexed by day (too large for LDS at 4096 days) go to global atomics aggregated in the wave
//                   (wave_add): the lanes that share the first lane's cell add once (agents are sorted by age and an epidemic's
//                   days are few: most of a wave's lanes do).
// GROUP: the member is element blockIdx.y of the group's member table (MEMBER_OF_LAUNCH), its log words and report block the
// blockIdx.y-th of the log's (member_block); otherwise the one engine by value.  One lane owns an agent: no atomics on the log,
// no fences (a kernel boundary lies on either side of every launch).
#include "../../include/reina_txlog.h"

#define TXL_NONE ((uint32_t)REINA_TXLOG_NONE)
#define TXL_BEFORE ((uint32_t)REINA_TXLOG_BEFORE)
static_assert(REINA_MAX_DAYS < REINA_TXLOG_BEFORE, "day numbers lie below the codes");
static_assert(REINA_TXLOG_FIXED_WORDS == 1312u && REINA_TXLOG_DAY_WORDS == 80u, "report layout");
static_assert(REINA_TXLOG_VARIANTS == REINA_MAX_VARIANTS && REINA_TXLOG_MAX_GROUPS == REINA_TX_MAX_GROUPS, "RH_VARIANT has two bits; the groups are the tree reports'");

__host__ __device__ __forceinline__ uint32_t txl_begin_word(uint32_t w) {
    const uint32_t st = RH_STATE(w);
    return (st >= RS_ILLNESS ? TXL_BEFORE : TXL_NONE) << 16 | (st != RS_SUSCEPTIBLE ? TXL_BEFORE : TXL_NONE);
}

// the log is padded to whole tiles (its words beyond n_agents: NONE | NONE, never read back); the hot words are not
template <bool GROUP>
__global__ __launch_bounds__(REPORT_THREADS) void k_txlog_begin(const MemberRef *M_, const MemberRef one_, uint32_t *log, size_t stride, uint32_t N) {
    MEMBER_OF_LAUNCH;
    const GAS uint32_t *hot = (const GAS uint32_t *)mref_.B.hot;
    GAS uint32_t *L = member_block<GROUP>(log, stride);
    const uint32_t quads = (N + 3u) / 4u;
    for (uint32_t q = blockIdx.x * REPORT_THREADS + threadIdx.x; q < quads; q += gridDim.x * REPORT_THREADS) {
        const uint32_t i = 4u * q;
        v4u_ w;
        if (i + 3u < N) {
            w = *reinterpret_cast<const GAS v4u_ *>(hot + i);
        } else {
            w.x = hot[i];
            w.y = i + 1u < N ? hot[i + 1u] : 0u;
            w.z = i + 2u < N ? hot[i + 2u] : 0u;
            w.w = 0u;
        }
        v4u_ o;
        o.x = txl_begin_word(w.x);
        o.y = txl_begin_word(w.y);
        o.z = txl_begin_word(w.z);
        o.w = txl_begin_word(w.w);
        *reinterpret_cast<GAS v4u_ *>(L + i) = o;
    }
}

// the day's update of one infected agent's log word, in both forms (the header comment: by_hot): shared by k_txlog_day and
// k_course_day (k_course.inc), so that the two cannot disagree.  d8 / o8: day and day + 1 as bits 24-31 hold them.
__device__ __forceinline__ void txl_day_update(GAS uint32_t *L, uint32_t i, uint32_t w, uint32_t day, uint32_t d8, uint32_t o8, uint32_t by_hot) {
    const uint32_t st = RH_STATE(w);
    if (by_hot) {
        if (st == RS_INCUBATION && (w >> 24) == d8)
            L[i] = TXL_NONE << 16 | day;
        else if (st == RS_ILLNESS && (w >> 24) == o8)
            reinterpret_cast<GAS uint16_t *>(L)[2u * i + 1u] = (uint16_t)day;
    } else {
        const uint32_t lw = L[i];
        uint32_t nw = lw;
        if ((lw & 0xFFFFu) == TXL_NONE) nw = (nw & 0xFFFF0000u) | day;
        if ((lw >> 16) == TXL_NONE && st >= RS_ILLNESS) nw = (nw & 0xFFFFu) | day << 16;
        if (nw != lw) L[i] = nw;
    }
}

// four waves a workgroup, one tile a wave and round, the tiles strided over the grid
template <bool GROUP>
__global__ __launch_bounds__(REPORT_THREADS) void k_txlog_day(const MemberRef *M_, const MemberRef one_, uint32_t *log, size_t stride, uint32_t N, uint32_t day,
                                                              uint32_t by_hot) {
    MEMBER_OF_LAUNCH;
    const GAS uint32_t *hot = (const GAS uint32_t *)mref_.B.hot;
    const GAS uint32_t *plane = (const GAS uint32_t *)mref_.B.active_bits;
    GAS uint32_t *L = member_block<GROUP>(log, stride);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t tiles = (N + REPORT_TILE - 1u) / REPORT_TILE;
    const uint32_t d8 = day & 0xFFu, o8 = (day + 1u) & 0xFFu;
    for (uint32_t t = blockIdx.x * (REPORT_THREADS / 64u) + wave; t < tiles; t += gridDim.x * (REPORT_THREADS / 64u)) {
        uint32_t w[8];
        if (!active_tile(plane, hot, t, N, lane, w)) continue;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t i = t * REPORT_TILE + (uint32_t)j * 64u + lane;
            if (RH_STATE(w[j]) == RS_SUSCEPTIBLE) continue;
            txl_day_update(L, i, w[j], day, d8, o8, by_hot);
        }
    }
}

__device__ __forceinline__ int txl_clip(int x, int hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

// 256 threads, tiles of 512 agents (two per thread), the workgroup's tiles strided over the grid
template <bool GROUP>
__global__ __launch_bounds__(REPORT_THREADS) void k_txlog_report(const MemberRef *M_, const MemberRef one_, const uint32_t *log, size_t stride,
                                                                 uint64_t *report, const TxlArgs a) {
    __shared__ uint32_t s_h[REINA_TXLOG_SCALARS];   // the interval histograms and the link phases, at the block's own offsets
    __shared__ uint32_t s_c[REINA_TXLOG_S_NR];
    __shared__ ReportAges s_ages;
    MEMBER_OF_LAUNCH;
    const GAS uint32_t *hot = (const GAS uint32_t *)mref_.B.hot;
    const GAS reina_cold_t *cold = (const GAS reina_cold_t *)mref_.B.cold;
    const GAS uint32_t *L = member_block<GROUP>(log, stride);
    GAS unsigned long long *R = member_block<GROUP>((unsigned long long *)report, REINA_TXLOG_REPORT_WORDS(a.n_days));
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t k = tid; k < REINA_TXLOG_SCALARS; k += REPORT_THREADS) s_h[k] = 0u;
    if (tid < REINA_TXLOG_S_NR) s_c[tid] = tid == REINA_TXLOG_S_FIRST_DAY ? 0xFFFFFFFFu : 0u;
    s_ages.load(a.p);
    __syncthreads();
    const uint32_t N = a.p.n_agents, D = a.n_days, tiles = (N + REPORT_TILE - 1u) / REPORT_TILE;
    GAS unsigned long long *inc_t = R + REINA_TXLOG_INCIDENCE(D), *ons_t = R + REINA_TXLOG_ONSETS(D), *coh_t = R + REINA_TXLOG_COHORT(D);
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        Links l;
        if (!load_links<true>(l, t, N, hot, cold, L, s_c, REINA_TXLOG_S_INFECTED, -1, REINA_TXLOG_S_LINKS, REINA_TXLOG_S_BAD_LINKS)) continue;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint32_t i = l.idx[j], w = l.w[j], v = RH_VARIANT(w);
            const uint32_t ti = l.lw[j] & 0xFFFFu, oi = l.lw[j] >> 16;
            const bool tk = l.inf[j] && ti < TXL_BEFORE, ok = l.inf[j] && oi < TXL_BEFORE;
            const uint32_t ts = l.sl[j] & 0xFFFFu, os = l.sl[j] >> 16;
            const bool linked = l.linked[j], tsk = linked && ts < TXL_BEFORE, osk = linked && os < TXL_BEFORE;
            const bool both = tk && tsk;
            // the scalars (out_of_range: one predicate a date)
            wave_tally(&s_c[REINA_TXLOG_S_DATED], tk);
            wave_tally(&s_c[REINA_TXLOG_S_BEFORE], l.inf[j] && ti == TXL_BEFORE);
            wave_tally(&s_c[REINA_TXLOG_S_WITH_ONSET], ok);
            wave_tally(&s_c[REINA_TXLOG_S_LINKS_DATED], both);
            wave_tally(&s_c[REINA_TXLOG_S_GENERATION_NONPOSITIVE], both && ti <= ts);
            wave_tally(&s_c[REINA_TXLOG_S_OUT_OF_RANGE], tk && ti >= D);
            wave_tally(&s_c[REINA_TXLOG_S_OUT_OF_RANGE], ok && oi >= D);
            // (the first and the last day are a minimum and a maximum, not tallies; lo keeps all ones in a wave without a dated agent)
            const uint32_t lo = wave_min(tk ? ti : 0xFFFFFFFFu), hi = wave_max(tk ? ti : 0u);
            if (lane == 0 && lo != 0xFFFFFFFFu) {
                atomicMin(&s_c[REINA_TXLOG_S_FIRST_DAY], lo);
                atomicMax(&s_c[REINA_TXLOG_S_LAST_DAY], hi);
            }
            // the interval histograms (LDS)
            wave_count(s_h, tk && ok ? (int)(REINA_TXLOG_INCUBATION + v * REINA_TXLOG_INCUBATION_BINS) +
                                         txl_clip((int)oi - (int)ti, REINA_TXLOG_INCUBATION_BINS - 1)
                                   : -1);
            wave_count(s_h, both ? (int)(REINA_TXLOG_GENERATION + v * REINA_TXLOG_GENERATION_BINS) +
                                     txl_clip((int)ti - (int)ts, REINA_TXLOG_GENERATION_BINS - 1)
                               : -1);
            wave_count(s_h, ok && osk ? (int)(REINA_TXLOG_SERIAL + v * REINA_TXLOG_SERIAL_BINS) +
                                          txl_clip((int)oi - (int)os + REINA_TXLOG_SERIAL_SHIFT, REINA_TXLOG_SERIAL_BINS - 1)
                                    : -1);
            wave_count(s_h, tk && osk ? (int)(REINA_TXLOG_TOST + v * REINA_TXLOG_TOST_BINS) +
                                          txl_clip((int)ti - (int)os + REINA_TXLOG_TOST_SHIFT, REINA_TXLOG_TOST_BINS - 1)
                                    : -1);
            const uint32_t phase = tk && osk ? (ti < os ? 0u : 1u) : (tk && os == TXL_NONE ? 2u : 3u);
            wave_count(s_h, linked ? (int)(REINA_TXLOG_LINK_PHASE + v * REINA_TXLOG_PHASES + phase) : -1);
            // the tables by day (global, aggregated in the wave)
            const bool in = tk && ti < D;
            int g = 0;
            if (in) g = s_ages.group_of(i);
            wave_add(inc_t, in ? (int)((ti * REINA_TXLOG_VARIANTS + v) * REINA_TXLOG_MAX_GROUPS) + g : -1, 1ull);
            wave_add(ons_t, ok && oi < D ? (int)(oi * REINA_TXLOG_VARIANTS + v) : -1, 1ull);
            const int ck = in ? (int)((ti * REINA_TXLOG_VARIANTS + v) * REINA_TXLOG_COHORT_FIELDS) : -1;
            wave_add(coh_t, ck, 1ull);
            wave_add(coh_t + 1, ck, (unsigned long long)l.n[j]);
            wave_add(coh_t + 2, ck, RH_STATE(w) >= RS_RECOVERED ? 1ull : 0ull);
        }
    }
    __syncthreads();
    flush_lds(s_h, REINA_TXLOG_SCALARS, R);
    if (tid < REINA_TXLOG_S_NR) {
        GAS unsigned long long *S = R + REINA_TXLOG_SCALARS;
        if (tid == REINA_TXLOG_S_FIRST_DAY) {
            if (s_c[tid] != 0xFFFFFFFFu) atomicMin(&S[tid], (unsigned long long)s_c[tid]);
        } else if (tid == REINA_TXLOG_S_LAST_DAY) {
            if (s_c[tid]) atomicMax(&S[tid], (unsigned long long)s_c[tid]);
        } else if (s_c[tid]) {
            atomicAdd(&S[tid], (unsigned long long)s_c[tid]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host side

struct reina_course;                         // (k_course.inc: the clinical course log attached to a log)
struct reina_txlog : attachment {            // (last_day: the last day recorded)
    uint32_t *d_log = nullptr;               // [members][stride]
    size_t stride = 0;                       // words a member: n_agents rounded up to whole tiles
    bool by_hot = true;                      // k_txlog_day's form (REINA_TXLOG_FORM=log: the log word of every active agent; measurement handle)
    reina_course *course = nullptr;          // attached: the day's launch is k_course_day, which records both
    uint8_t *d_labels = nullptr;             // [members][REINA_MAX_DAYS]: the labels of a regime report (k_regime.inc), made by the first one
};
static int course_launch_day(reina_txlog *l, uint32_t grid, uint32_t day, uint32_t by_hot, hipStream_t s);   // (k_course.inc)
static void course_detach(reina_course *c);   // (the log goes first: the course refuses from then on)

static void free_txlog(reina_txlog *l) {
    if (l->course) course_detach(l->course);
    if (l->d_log) (void)hipFree(l->d_log);
    if (l->d_labels) (void)hipFree(l->d_labels);
    delete l;
}

// a launch that streams: eight workgroups a compute unit
static uint32_t txlog_grid(const reina_txlog *l, uint32_t units) { return member_grid(l->e0->n_cus, (uint32_t)l->members.size(), units, 8u); }

static int txlog_create(const std::vector<reina_engine_t *> &members, reina_group *g, const MemberRef *d_refs, hipStream_t s, reina_txlog_t **out) {
    if (!out) return REINA_E_INVALID;
    if (int rc = attachment_check_members(members, "txlog", "links are global ids, and a shard sees only its own agents' onsets")) return rc;
    for (auto m : members)
        if (reinterpret_cast<uintptr_t>(m->buf.hot) & 15u) return refuse("txlog: the hot words must be 16-byte aligned");
    std::unique_ptr<reina_txlog, void (*)(reina_txlog *)> l(new reina_txlog(), free_txlog);   // (freed by a failing return)
    l->e0 = members[0], l->g = g, l->members = members, l->d_refs = d_refs;
    const char *form = std::getenv("REINA_TXLOG_FORM");
    l->by_hot = !(form && std::strcmp(form, "log") == 0);
    const uint32_t N = l->e0->cfg.n_agents, K = (uint32_t)members.size();
    l->stride = ((size_t)N + REPORT_TILE - 1u) / REPORT_TILE * REPORT_TILE;
    HIP_CHECK(hipMalloc(&l->d_log, sizeof(uint32_t) * l->stride * K));
    const uint32_t grid = txlog_grid(l.get(), ((N + 3u) / 4u + REPORT_THREADS - 1u) / REPORT_THREADS);
    launch_members(k_txlog_begin, g, grid, K, REPORT_THREADS, s, d_refs, l->e0->h_ref, l->d_log, l->stride, N);
    *out = l.release();
    return REINA_OK;
}

// behind a day's last launch
static int txlog_launch_day(reina_txlog *l, uint32_t day, hipStream_t s) {
    if (int rc = attachment_check_day(day)) return rc;
    const uint32_t N = l->e0->cfg.n_agents, K = (uint32_t)l->members.size();
    // (the hot-word tests hold for the days that follow a recorded day: the first day, and a day after a gap, read the log)
    const uint32_t by_hot = l->by_hot && l->last_day >= 0 && (int64_t)day == l->last_day + 1 ? 1u : 0u;
    const uint32_t tiles = (N + REPORT_TILE - 1u) / REPORT_TILE;
    const uint32_t grid = txlog_grid(l, (tiles + REPORT_THREADS / 64u - 1u) / (REPORT_THREADS / 64u));
    if (l->course) {
        if (int rc = course_launch_day(l, grid, day, by_hot, s)) return rc;
    } else {
        launch_members(k_txlog_day, l->g, grid, K, REPORT_THREADS, s, l->d_refs, l->e0->h_ref, l->d_log, l->stride, N, day, by_hot);
    }
    l->last_day = day;
    return REINA_OK;
}
static int txlog_after_day(attachment *a, const reina_day_t &d, hipStream_t s) { return txlog_launch_day(static_cast<reina_txlog *>(a), d.day, s); }

static int txlog_report(reina_txlog *l, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days, uint64_t *dev_report, hipStream_t s) {
    return day_report(l, "txlog report", REINA_TXLOG_MAX_GROUPS, REINA_TXLOG_REPORT_WORDS(n_days), age_group, n_groups, n_days, dev_report, s,
                      [&](const TxlArgs &a, uint32_t grid, uint32_t K) -> int {
                          // (the first day is a minimum: every member's cell starts at all ones)
                          HIP_CHECK(hipMemset2DAsync(dev_report + REINA_TXLOG_SCALARS + REINA_TXLOG_S_FIRST_DAY, REINA_TXLOG_REPORT_WORDS(n_days) * 8u, 0xFF, 8u, K, s));
                          launch_members(k_txlog_report, l->g, grid, K, REPORT_THREADS, s, l->d_refs, l->e0->h_ref, l->d_log, l->stride, dev_report, a);
                          return REINA_OK;
                      });
}

extern "C" {

int reina_txlog_version(void) { return REINA_TXLOG_VERSION; }

int reina_txlog_create(reina_engine_t *e, void *stream, reina_txlog_t **out) {
    if (!e) return REINA_E_INVALID;
    if (!e->bound) return REINA_E_NOT_BOUND;
    return txlog_create(std::vector<reina_engine_t *>(1, e), nullptr, e->d_ref, (hipStream_t)stream, out);
}

int reina_group_txlog_create(reina_group_t *g, void *stream, reina_txlog_t **out) {
    if (!g || g->members.empty()) return REINA_E_INVALID;
    return txlog_create(g->members, g, g->d_refs, (hipStream_t)stream, out);
}

int reina_txlog_destroy(reina_txlog_t *log) {
    if (!log) return REINA_E_INVALID;
    free_txlog(log);
    return REINA_OK;
}

int reina_txlog_record_day(reina_txlog_t *log, uint32_t day, void *stream) {
    if (!log) return REINA_E_INVALID;
    return txlog_launch_day(log, day, (hipStream_t)stream);
}

int reina_txlog_run_days(reina_txlog_t *log, const reina_day_t *days, uint32_t n_days, int32_t *history_base, void *stream) {
    if (!days) return REINA_E_INVALID;
    if (int rc = attachment_kind(log, false, "reina_txlog_run_days")) return rc;
    return engine_run_days(log->e0, days, n_days, history_base, stream, day_hooks{log, nullptr, txlog_after_day});
}

int reina_group_txlog_run_days(reina_txlog_t *log, const reina_day_t *days, uint32_t n_days, int32_t *const *history_bases, void *stream) {
    if (!days) return REINA_E_INVALID;
    if (int rc = attachment_kind(log, true, "reina_group_txlog_run_days")) return rc;
    for (uint32_t k = 0; k < n_days; k++)   // (before any day runs: the record launch comes behind its day)
        if (int rc = attachment_check_day(days[k].day)) return rc;
    return group_run_days(log->g, days, n_days, history_bases, stream, day_hooks{log, nullptr, txlog_after_day});
}

int reina_txlog_report(reina_txlog_t *log, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days, uint64_t *dev_report, void *stream) {
    if (int rc = attachment_kind(log, false, "reina_txlog_report")) return rc;
    return txlog_report(log, age_group, n_groups, n_days, dev_report, (hipStream_t)stream);
}

int reina_group_txlog_report(reina_txlog_t *log, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days, uint64_t *dev_report, void *stream) {
    if (int rc = attachment_kind(log, true, "reina_group_txlog_report")) return rc;
    return txlog_report(log, age_group, n_groups, n_days, dev_report, (hipStream_t)stream);
}

int reina_txlog_read(reina_txlog_t *log, uint32_t member, uint32_t *out_host, void *stream) {
    if (!log || !out_host) return REINA_E_INVALID;
    return member_copy(log, log->d_log, log->stride, sizeof(uint32_t), member, out_host, true, "txlog", (hipStream_t)stream);
}

int reina_txlog_write(reina_txlog_t *log, uint32_t member, const uint32_t *in_host, void *stream) {
    if (!log || !in_host) return REINA_E_INVALID;
    return member_copy(log, log->d_log, log->stride, sizeof(uint32_t), member, const_cast<uint32_t *>(in_host), false, "txlog", (hipStream_t)stream);
}

}  // extern "C"
