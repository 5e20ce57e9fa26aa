// reina_hip.hip part: lineage reports -- mixing by period and trees by seeding period (include/reina_lineage.h; DESIGN.md
// section 6i).  Included at the end of reina_hip.hip, behind k_transmission.inc and k_txlog.inc: a report joins the trees of the
// one with the dates of the other, through k_addons.inc's load_links, so the three reports agree on what a link is.
//
// A report reads the hot words, the cold records and the log and writes nothing but the caller's scratch and report block.  The
// member is a TxMember (k_transmission.inc): scratch = pairs [2][N] | size [N] | alive [N], the last at size + N; the member's
// log words are its block of the log's (member_block), as in k_txlog_report.  Five kinds of launch:
//   k_lineage_links   streams hot + log, gathers the cold record of infected agents and hot + log of their infectors; the tables
//                     by period (too large for LDS at 256 periods) go to global atomics aggregated in the wave, the link
//                     scalars to LDS; writes every agent's (parent, distance) pair exactly as k_tx_links does and zeroes its
//                     size and alive words.
//   k_tx_jump         k_transmission.inc's, unchanged.
//   k_lineage_tally   converged agents: the root's log word (one scattered line, shared by a whole tree) gives the seed class;
//                     lineage and seed[..][2..3] through wave_add; the agent (and the agent if alive) into its root's size and
//                     alive words as k_tx_tally counts sizes: the lanes that share the first lane's root add once, the rest go
//                     through a per-workgroup LDS hash, global atomics only when its probes fail.
//   k_lineage_roots   streams the size and alive words: a non-zero size is a tree; its own log word gives the seed class;
//                     tree_sizes and seed[..][0..1] in LDS, flushed once per workgroup; the largest tree by a 64-bit max.
//   k_lineage_finish  one lane per member: rounds, the largest tree decoded.
#include "../../include/reina_lineage.h"

#define LIN_Q_MAX (REINA_LINEAGE_MAX_PERIODS + 1u)
static_assert(REINA_LINEAGE_MAX_GROUPS == REINA_TX_MAX_GROUPS && REINA_LINEAGE_SIZE_BINS == REINA_TX_CLUSTER_BINS, "the groups and size bins are the tree reports'");
static_assert(REINA_LINEAGE_REPORT_WORDS(53) == 34306u && REINA_LINEAGE_SCRATCH_BYTES(32) == 768u, "report layout");
static_assert(REINA_LINEAGE_REPORT_WORDS(REINA_LINEAGE_MAX_PERIODS) < (1u << 30), "table cells are int keys");

struct LinArgs {
    TxArgs t;
    uint32_t period_days, P;
};

// the period class of a log half word
__device__ __forceinline__ uint32_t lin_pc(uint32_t d, const LinArgs &a) {
    if (d >= TXL_BEFORE) return a.P;
    const uint32_t q = d / a.period_days;
    return q < a.P ? q : a.P;
}

__device__ __forceinline__ bool lin_alive(uint32_t w) { return RH_STATE(w) >= RS_INCUBATION && RH_STATE(w) <= RS_IN_ICU; }

// 256 threads, tiles of 512 agents (two per thread), the workgroup's tiles strided over the grid
template <bool GROUP>
__global__ __launch_bounds__(REPORT_THREADS) void k_lineage_links(const TxMember *M_, const TxMember one_, const uint32_t *log, size_t stride,
                                                                  const LinArgs a) {
    __shared__ uint32_t s_cnt[5];   // infected, roots, linked, bad links, undated
    __shared__ ReportAges s_ages;
    const TxMember m = tx_member<GROUP>(M_, one_);
    const GAS uint32_t *hot = (const GAS uint32_t *)m.hot;
    const GAS reina_cold_t *cold = (const GAS reina_cold_t *)m.cold;
    const GAS uint32_t *L = member_block<GROUP>(log, stride);
    const uint32_t N = a.t.p.n_agents, P = a.P, tiles = (N + REPORT_TILE - 1u) / REPORT_TILE;
    GAS uint64_t *pairs = (GAS uint64_t *)m.pairs;
    GAS uint32_t *size = (GAS uint32_t *)m.size, *alive = size + N;
    GAS unsigned long long *R = (GAS unsigned long long *)m.report;
    GAS unsigned long long *coh = R + REINA_LINEAGE_COHORT(P), *mix_t = R + REINA_LINEAGE_MIXING_T(P), *mix_c = R + REINA_LINEAGE_MIXING_C(P);
    const uint32_t tid = threadIdx.x;
    if (tid < 5) s_cnt[tid] = 0u;
    s_ages.load(a.t.p);
    __syncthreads();
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        Links l;
        const bool any = load_links<true>(l, t, N, hot, cold, L, s_cnt, 0, 1, 2, 3);   // (a tile without infected agents still writes its pairs)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint32_t i = l.idx[j];
            if (any) {
                const uint32_t ci = lin_pc(l.lw[j] & 0xFFFFu, a), cs = lin_pc(l.sl[j] & 0xFFFFu, a);
                int gi = 0, gs = 0;
                if (l.inf[j]) gi = s_ages.group_of(i);
                if (l.linked[j]) gs = s_ages.group_of((uint32_t)l.src[j]);
                wave_tally(&s_cnt[4], l.inf[j] && ci == P);
                const int ck = l.inf[j] ? (int)((ci * REINA_LINEAGE_MAX_GROUPS + (uint32_t)gi) * REINA_LINEAGE_COHORT_FIELDS) : -1;
                wave_add(coh, ck, 1ull);
                wave_add(coh + 1, ck, RH_STATE(l.w[j]) >= RS_RECOVERED ? 1ull : 0ull);
                const int cell = gs * (int)REINA_LINEAGE_MAX_GROUPS + gi;
                wave_add(mix_t, l.linked[j] ? (int)(ci * REINA_LINEAGE_MAX_GROUPS * REINA_LINEAGE_MAX_GROUPS) + cell : -1, 1ull);
                wave_add(mix_c, l.linked[j] ? (int)(cs * REINA_LINEAGE_MAX_GROUPS * REINA_LINEAGE_MAX_GROUPS) + cell : -1, 1ull);
            }
            if (i < N) {
                pairs[i] = !l.inf[j]     ? (uint64_t)TX_MARK
                           : l.linked[j] ? ((uint64_t)(uint32_t)l.src[j] | (1ull << 32))
                                         : ((uint64_t)i | ((uint64_t)TX_ROOTED << 32));
                size[i] = 0u;
                alive[i] = 0u;
            }
        }
    }
    __syncthreads();
    if (tid < 5 && s_cnt[tid]) {
        const uint32_t at[5] = {REINA_LINEAGE_S_INFECTED, REINA_LINEAGE_S_ROOTS, REINA_LINEAGE_S_LINKS, REINA_LINEAGE_S_BAD_LINKS, REINA_LINEAGE_S_UNDATED};
        atomicAdd(&R[REINA_LINEAGE_SCALARS + at[tid]], (unsigned long long)s_cnt[tid]);
    }
}

// 256 threads, one agent per thread, strided over the grid
template <bool GROUP>
__global__ __launch_bounds__(REPORT_THREADS) void k_lineage_tally(const TxMember *M_, const TxMember one_, const uint32_t *log, size_t stride,
                                                                  const LinArgs a) {
    __shared__ uint32_t s_key[TX_HASH], s_size[TX_HASH], s_alive[TX_HASH];
    __shared__ uint32_t s_unconv, s_alive_agents;
    const TxMember m = tx_member<GROUP>(M_, one_);
    const GAS uint32_t *L = member_block<GROUP>(log, stride);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t k = tid; k < TX_HASH; k += REPORT_THREADS) {
        s_key[k] = TX_MARK;
        s_size[k] = s_alive[k] = 0u;
    }
    if (tid == 0) s_unconv = s_alive_agents = 0u;
    __syncthreads();
    const uint32_t N = a.t.p.n_agents, P = a.P, Q = P + 1u;
    const uint64_t *pairs = m.pairs + (size_t)(tx_member_rounds(m, a.t) & 1u) * N;
    uint32_t *size = m.size, *alive = m.size + N;
    GAS unsigned long long *R = (GAS unsigned long long *)m.report;
    GAS unsigned long long *seed = R + REINA_LINEAGE_SEED(P), *lin = R + REINA_LINEAGE_LINEAGE(P);
    const uint32_t step = gridDim.x * REPORT_THREADS;
    const uint32_t end = (N + REPORT_THREADS - 1u) / REPORT_THREADS * REPORT_THREADS;   // (whole waves run the loop)
    for (uint32_t i = blockIdx.x * REPORT_THREADS + tid; i < end; i += step) {
        uint64_t p = (uint64_t)TX_MARK;
        uint32_t w = 0u, lw = 0u;
        if (i < N) {
            p = pairs[i];
            w = m.hot[i];
            lw = L[i];
        }
        const uint32_t parent = (uint32_t)p, d = (uint32_t)(p >> 32);
        const bool infected = parent != TX_MARK;
        const bool conv = infected && (d & TX_ROOTED) && parent < N;   // (every pair of an infected agent points below N)
        const bool al = conv && lin_alive(w);
        const uint32_t rl = conv ? L[parent] : 0u;
        const uint32_t sc = lin_pc(rl & 0xFFFFu, a), ci = lin_pc(lw & 0xFFFFu, a);
        wave_add(lin, conv ? (int)(sc * Q + ci) : -1, 1ull);
        const int sk = conv ? (int)(sc * REINA_LINEAGE_SEED_FIELDS) : -1;
        wave_add(seed + 2, sk, 1ull);
        wave_add(seed + 3, sk, al ? 1ull : 0ull);
        wave_tally(&s_unconv, infected && !conv);
        wave_tally(&s_alive_agents, al);
        // tree sizes and alive counts: the lanes that share the first converged lane's root add once
        const uint32_t key = conv ? parent : TX_MARK;
        const uint64_t act = __ballot(conv);
        if (act) {
            const int lead = __ffsll((unsigned long long)act) - 1;
            const uint32_t lk = (uint32_t)__shfl((int)key, lead);
            const uint64_t same = __ballot(key == lk), same_alive = __ballot(key == lk && al);
            if (key == lk) {
                if ((int)lane == lead) {
                    tx_hash_add(s_key, s_size, size, lk, (uint32_t)__popcll(same));
                    if (same_alive) tx_hash_add(s_key, s_alive, alive, lk, (uint32_t)__popcll(same_alive));   // (the key's slot, or its probes fail again)
                }
            } else if (conv) {
                tx_hash_add(s_key, s_size, size, key, 1u);
                if (al) tx_hash_add(s_key, s_alive, alive, key, 1u);
            }
        }
    }
    __syncthreads();
    for (uint32_t k = tid; k < TX_HASH; k += REPORT_THREADS)
        if (s_key[k] != TX_MARK) {
            if (s_size[k]) atomicAdd(&size[s_key[k]], s_size[k]);
            if (s_alive[k]) atomicAdd(&alive[s_key[k]], s_alive[k]);
        }
    if (tid == 0) {
        if (s_unconv) atomicAdd(&R[REINA_LINEAGE_SCALARS + REINA_LINEAGE_S_UNCONVERGED], (unsigned long long)s_unconv);
        if (s_alive_agents) atomicAdd(&R[REINA_LINEAGE_SCALARS + REINA_LINEAGE_S_ALIVE_AGENTS], (unsigned long long)s_alive_agents);
    }
}

// 256 threads, one agent per thread, strided over the grid; a non-zero size is the head of a tree
template <bool GROUP>
__global__ __launch_bounds__(REPORT_THREADS) void k_lineage_roots(const TxMember *M_, const TxMember one_, const uint32_t *log, size_t stride,
                                                                  const LinArgs a) {
    __shared__ uint32_t s_ts[LIN_Q_MAX * REINA_LINEAGE_SIZE_BINS];
    __shared__ uint32_t s_seed[LIN_Q_MAX * 2u];   // trees, alive trees
    __shared__ uint32_t s_trees, s_alive_trees;
    __shared__ unsigned long long s_big;
    const TxMember m = tx_member<GROUP>(M_, one_);
    const GAS uint32_t *L = member_block<GROUP>(log, stride);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t N = a.t.p.n_agents, P = a.P, Q = P + 1u;
    for (uint32_t k = tid; k < Q * REINA_LINEAGE_SIZE_BINS; k += REPORT_THREADS) s_ts[k] = 0u;
    for (uint32_t k = tid; k < Q * 2u; k += REPORT_THREADS) s_seed[k] = 0u;
    if (tid == 0) {
        s_trees = s_alive_trees = 0u;
        s_big = 0ull;
    }
    __syncthreads();
    const uint32_t *size = m.size, *alive = m.size + N;
    const uint32_t step = gridDim.x * REPORT_THREADS;
    const uint32_t end = (N + REPORT_THREADS - 1u) / REPORT_THREADS * REPORT_THREADS;
    for (uint32_t i = blockIdx.x * REPORT_THREADS + tid; i < end; i += step) {
        const uint32_t s = i < N ? size[i] : 0u;
        unsigned long long key = 0ull;
        bool al = false;
        if (s) {
            al = alive[i] != 0u;
            const uint32_t sc = lin_pc(L[i] & 0xFFFFu, a);
            atomicAdd(&s_ts[sc * REINA_LINEAGE_SIZE_BINS + (31u - (uint32_t)__clz((int)s))], 1u);
            atomicAdd(&s_seed[sc * 2u], 1u);
            if (al) atomicAdd(&s_seed[sc * 2u + 1u], 1u);
            key = ((unsigned long long)s << 32) | (unsigned long long)(~i);
        }
        wave_tally(&s_trees, s != 0u);
        wave_tally(&s_alive_trees, al);
        key = wave_max(key);
        if (lane == 0 && key) atomicMax(&s_big, key);
    }
    __syncthreads();
    GAS unsigned long long *R = (GAS unsigned long long *)m.report;
    flush_lds(s_ts, Q * REINA_LINEAGE_SIZE_BINS, R + REINA_LINEAGE_TREE_SIZES(P));
    for (uint32_t k = tid; k < Q * 2u; k += REPORT_THREADS)
        if (s_seed[k]) atomicAdd(&R[REINA_LINEAGE_SEED(P) + (k >> 1) * REINA_LINEAGE_SEED_FIELDS + (k & 1u)], (unsigned long long)s_seed[k]);
    if (tid == 0) {
        if (s_trees) atomicAdd(&R[REINA_LINEAGE_SCALARS + REINA_LINEAGE_S_TREES], (unsigned long long)s_trees);
        if (s_alive_trees) atomicAdd(&R[REINA_LINEAGE_SCALARS + REINA_LINEAGE_S_ALIVE_TREES], (unsigned long long)s_alive_trees);
        if (s_big) atomicMax(&R[REINA_LINEAGE_SCALARS + REINA_LINEAGE_S_LARGEST_KEY], s_big);
    }
}

// one lane per member (grid.y)
template <bool GROUP>
__global__ __launch_bounds__(64) void k_lineage_finish(const TxMember *M_, const TxMember one_, const LinArgs a) {
    const TxMember m = tx_member<GROUP>(M_, one_);
    if (threadIdx.x != 0) return;
    uint64_t *S = m.report + REINA_LINEAGE_SCALARS;
    const uint64_t key = S[REINA_LINEAGE_S_LARGEST_KEY];
    S[REINA_LINEAGE_S_ROUNDS] = tx_member_rounds(m, a.t);
    S[REINA_LINEAGE_S_LARGEST_TREE] = key >> 32;
    S[REINA_LINEAGE_S_LARGEST_ROOT] = key ? (uint64_t)(uint32_t)~(uint32_t)key : ~0ull;
}

// ---------------------------------------------------------------------------------------------
// host side

static int lineage_args(const reina_txlog *l, const uint8_t *age_group, uint32_t n_groups, uint32_t period_days, uint32_t n_periods, uint32_t max_depth,
                        LinArgs *a) {
    if (period_days < 1u || period_days > REINA_MAX_DAYS) return refuse("lineage report: period_days must be in [1, REINA_MAX_DAYS]");
    if (n_periods < 1u || n_periods > REINA_LINEAGE_MAX_PERIODS) return refuse("lineage report: n_periods must be in [1, REINA_LINEAGE_MAX_PERIODS]");
    a->period_days = period_days;
    a->P = n_periods;
    a->t.host_rounds = max_depth ? tx_rounds(max_depth) : 0xFFFFFFFFu;
    return age_group_args(l->e0, age_group, n_groups, REINA_LINEAGE_MAX_GROUPS, "lineage report", &a->t.p);
}

// every pass of a report: the K members of the device table `d_m`, or (d_m = nullptr) the one member `one`
static int lineage_launch(const reina_txlog *l, const TxMember *d_m, const TxMember &one, const LinArgs &a, uint64_t *report, hipStream_t s) {
    const uint32_t K = (uint32_t)l->members.size(), n_cus = l->e0->n_cus;
    HIP_CHECK(hipMemsetAsync(report, 0, (size_t)K * REINA_LINEAGE_REPORT_WORDS(a.P) * 8u, s));
    const ForestPasses f = forest_passes(a.t.p.n_agents, K, n_cus, a.t.host_rounds);
    launch_members(k_lineage_links, d_m, f.g_links, K, REPORT_THREADS, s, d_m, one, l->d_log, l->stride, a);
    for (uint32_t r = 0; r < f.rounds; r++) launch_members(k_tx_jump, d_m, f.g_jump, K, REPORT_THREADS, s, d_m, one, a.t, r);
    launch_members(k_lineage_tally, d_m, f.g_tally, K, REPORT_THREADS, s, d_m, one, l->d_log, l->stride, a);
    launch_members(k_lineage_roots, d_m, f.g_tally, K, REPORT_THREADS, s, d_m, one, l->d_log, l->stride, a);
    launch_members(k_lineage_finish, d_m, 1u, K, 64, s, d_m, one, a);
    return REINA_OK;
}

extern "C" {

int reina_lineage_version(void) { return REINA_LINEAGE_VERSION; }

int reina_lineage_report(reina_txlog_t *log, const uint8_t *age_group, uint32_t n_groups, uint32_t period_days, uint32_t n_periods,
                         uint32_t max_depth, void *dev_scratch, uint64_t *dev_report, void *stream) {
    if (int rc = attachment_kind(log, false, "reina_lineage_report")) return rc;
    if (int rc = tx_engine_ok(log->e0)) return rc;
    if (!tx_aligned(dev_scratch) || !tx_aligned(dev_report)) return refuse("reina_lineage_report: scratch and report must be 16-byte aligned device buffers");
    LinArgs a;
    if (int rc = lineage_args(log, age_group, n_groups, period_days, n_periods, max_depth, &a)) return rc;
    return lineage_launch(log, nullptr, tx_member_of(log->e0, dev_scratch, dev_report), a, dev_report, (hipStream_t)stream);
}

int reina_group_lineage_report(reina_txlog_t *log, const uint8_t *age_group, uint32_t n_groups, uint32_t period_days, uint32_t n_periods,
                               uint32_t max_depth, void *const *dev_scratch, uint64_t *dev_report, void *stream) {
    if (int rc = attachment_kind(log, true, "reina_group_lineage_report")) return rc;
    if (!dev_scratch) return REINA_E_INVALID;
    if (!tx_aligned(dev_report)) return refuse("reina_group_lineage_report: the reports must be a 16-byte aligned device buffer");
    LinArgs a;
    if (int rc = lineage_args(log, age_group, n_groups, period_days, n_periods, max_depth, &a)) return rc;
    std::vector<TxMember> h;
    if (int rc = member_table(log->members, dev_scratch, dev_report, REINA_LINEAGE_REPORT_WORDS(a.P), "reina_group_lineage_report", &h)) return rc;
    hipStream_t s = (hipStream_t)stream;
    return with_member_table(h, "reina_group_lineage_report", s, [&](const TxMember *d_m) { return lineage_launch(log, d_m, h[0], a, dev_report, s); });
}

}  // extern "C"
