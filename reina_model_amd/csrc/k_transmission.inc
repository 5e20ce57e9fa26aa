// reina_hip.hip part: transmission-tree reports of an unsharded engine between two days (include/reina_transmission.h;
// DESIGN.md "Transmission reports").  Included at the end of reina_hip.hip (it uses the host helpers, the group and
// k_addons.inc above: the wave helpers, load_links, the age-group arguments, the launch geometry, and TxMember with the
// passes and member table a forest report shares with the lineage report).
//
// A report reads the hot words and the cold records and writes nothing but the caller's scratch and report block.  Five kinds
// of launch, each bound by memory bandwidth:
//   k_tx_links     streams the hot words, gathers the cold record of infected agents (and the hot word of their infector),
//                  counts offspring, sums, the age matrix and the link kinds in LDS (flushed once per workgroup), and writes
//                  every agent's (parent, distance) pair: a root or a bad link (self, 0 | ROOTED), a link (infector, 1), a
//                  susceptible agent (TX_MARK, 0).  It also zeroes the tree sizes.
//   k_tx_jump      one round of pointer jumping: round r reads pair buffer r & 1 and writes the other, so after r rounds every
//                  distance up to 2^r is resolved whatever the schedule.  Rounds beyond the member's count return at once.
//   k_tx_tally     generations (and their maximum) of the agents whose pair reached a root, and every such agent counted into
//                  its root's tree size: the lanes of a wave that share the first lane's root add once, the others go through a
//                  per-workgroup LDS hash (global atomics only when its probes fail), so a giant tree does not serialise on one
//                  address.
//   k_tx_clusters  streams the tree sizes: the log2 bins and the largest tree (64-bit max of size << 32 | ~root).
//   k_tx_finish    one lane per member: rounds, sum_n_infected, the largest tree decoded.
// GROUP: the member is element blockIdx.y of a table read through the constant address space; otherwise `one_`, by value.
#include "../../include/reina_transmission.h"

#define TX_MARK 0xFFFFFFFFu        // parent of an agent that is not infected (and an empty hash slot)
#define TX_ROOTED 0x80000000u      // distance word: the parent is a root
#define TX_DIST_MAX 0x7FFFFFFFu    // distances saturate (a cycle of bad data doubles them every round)
#define TX_HASH 4096u              // k_tx_tally's LDS hash slots
#define TX_HASH_PROBES 8
#define TX_CELLS (REINA_TX_VARIANTS * REINA_TX_SEVERITIES * REINA_TX_OUTCOMES * 2u * REINA_TX_BINS)
#define TX_MATRIX_CELLS (REINA_TX_VARIANTS * REINA_TX_MAX_GROUPS * REINA_TX_MAX_GROUPS)
#define TX_SUMS (REINA_TX_VARIANTS * REINA_TX_OUTCOMES)
static_assert(REINA_TX_OFFSPRING_SUM == TX_CELLS && REINA_TX_REPORT_WORDS == 9834u, "report layout");
static_assert(REINA_MAX_VARIANTS == REINA_TX_VARIANTS, "RH_VARIANT has two bits");

struct TxArgs {
    AgeGroupArgs p;
    uint32_t host_rounds;   // ~0: from the member's day word
};

// smallest r with 2^r >= max_depth + 1
__host__ __device__ __forceinline__ uint32_t tx_rounds(uint64_t max_depth) {
    uint32_t r = 0;
    while ((1ull << r) < max_depth + 1u) r++;
    return r;
}

template <bool GROUP>
__device__ __forceinline__ TxMember tx_member(const TxMember *M_, const TxMember &one_) {
    if (!GROUP) return one_;
    TxMember m;
    member_from_constant(&m, M_ + blockIdx.y);
    return m;
}

__device__ __forceinline__ uint32_t tx_member_rounds(const TxMember &m, const TxArgs &a) {
    if (a.host_rounds != 0xFFFFFFFFu) return a.host_rounds;
    int32_t day = m.counters[SC_IDX(REINA_S_DAY)];
    day = day < 0 ? 0 : (day > (int32_t)REINA_MAX_DAYS ? (int32_t)REINA_MAX_DAYS : day);
    return tx_rounds((uint64_t)day + 1u);
}

// ---------------------------------------------------------------------------------------------
// k_tx_links: 256 threads, tiles of 512 agents (two per thread), the workgroup's tiles strided over the grid
template <bool GROUP>
__global__ __launch_bounds__(REPORT_THREADS) void k_tx_links(const TxMember *M_, const TxMember one_, const TxArgs a) {
    __shared__ uint32_t s_off[TX_CELLS];
    __shared__ uint32_t s_mat[TX_MATRIX_CELLS];
    __shared__ unsigned long long s_sum[TX_SUMS], s_sq[TX_SUMS];
    __shared__ uint32_t s_cnt[4];   // infected, roots, linked, bad links
    __shared__ ReportAges s_ages;
    const TxMember m = tx_member<GROUP>(M_, one_);
    const GAS uint32_t *hot = (const GAS uint32_t *)m.hot;
    const GAS reina_cold_t *cold = (const GAS reina_cold_t *)m.cold;
    GAS uint64_t *pairs = (GAS uint64_t *)m.pairs;
    GAS uint32_t *size = (GAS uint32_t *)m.size;
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < TX_CELLS; k += REPORT_THREADS) s_off[k] = 0u;
    for (uint32_t k = tid; k < TX_MATRIX_CELLS; k += REPORT_THREADS) s_mat[k] = 0u;
    if (tid < TX_SUMS) s_sum[tid] = s_sq[tid] = 0ull;
    if (tid < 4) s_cnt[tid] = 0u;
    s_ages.load(a.p);
    __syncthreads();
    const uint32_t N = a.p.n_agents, tiles = (N + REPORT_TILE - 1u) / REPORT_TILE;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        Links l;
        load_links<false>(l, t, N, hot, cold, nullptr, s_cnt, 0, 1, 2, 3);   // (a tile without infected agents still writes its pairs)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint32_t i = l.idx[j], w = l.w[j], n = l.n[j], st = RH_STATE(w), v = RH_VARIANT(w);
            const uint32_t sev = RH_SEV(w) < 4u ? RH_SEV(w) : 4u;
            const uint32_t o = st <= RS_IN_ICU ? 0u : ((w & RH_INCLUDED) ? 1u : 2u);
            const uint32_t det = (w & RH_DETECTED) ? 1u : 0u;
            wave_count(s_off, l.inf[j] ? (int)((((v * REINA_TX_SEVERITIES + sev) * REINA_TX_OUTCOMES + o) * 2u + det) * REINA_TX_BINS +
                                               (n < REINA_TX_BINS - 1u ? n : REINA_TX_BINS - 1u))
                                       : -1);
            if (l.inf[j] && n) {
                atomicAdd(&s_sum[v * REINA_TX_OUTCOMES + o], (unsigned long long)n);
                atomicAdd(&s_sq[v * REINA_TX_OUTCOMES + o], (unsigned long long)n * n);
            }
            if (l.linked[j]) {
                const uint32_t gs = (uint32_t)s_ages.group_of(i), gi = (uint32_t)s_ages.group_of((uint32_t)l.src[j]);
                atomicAdd(&s_mat[(v * REINA_TX_MAX_GROUPS + gi) * REINA_TX_MAX_GROUPS + gs], 1u);
            }
            if (i < N) {
                pairs[i] = !l.inf[j]     ? (uint64_t)TX_MARK
                           : l.linked[j] ? ((uint64_t)(uint32_t)l.src[j] | (1ull << 32))
                                         : ((uint64_t)i | ((uint64_t)TX_ROOTED << 32));
                size[i] = 0u;
            }
        }
    }
    __syncthreads();
    GAS unsigned long long *R = (GAS unsigned long long *)m.report;
    flush_lds(s_off, TX_CELLS, R + REINA_TX_OFFSPRING);
    flush_lds(s_mat, TX_MATRIX_CELLS, R + REINA_TX_MATRIX);
    flush_lds(s_sum, TX_SUMS, R + REINA_TX_OFFSPRING_SUM);
    flush_lds(s_sq, TX_SUMS, R + REINA_TX_OFFSPRING_SUMSQ);
    if (tid < 4 && s_cnt[tid]) {
        const uint32_t at[4] = {REINA_TX_S_N_INFECTED_AGENTS, REINA_TX_S_N_ROOTS, REINA_TX_S_N_LINKED, REINA_TX_S_BAD_LINKS};
        atomicAdd(&R[REINA_TX_SCALARS + at[tid]], (unsigned long long)s_cnt[tid]);
    }
}

// k_tx_jump: round r of pointer jumping, one thread per agent (grid-strided)
template <bool GROUP>
__global__ __launch_bounds__(REPORT_THREADS) void k_tx_jump(const TxMember *M_, const TxMember one_, const TxArgs a, uint32_t r) {
    const TxMember m = tx_member<GROUP>(M_, one_);
    if (r >= tx_member_rounds(m, a)) return;
    const uint32_t N = a.p.n_agents;
    const uint64_t *src = m.pairs + (size_t)(r & 1u) * N;
    uint64_t *dst = m.pairs + (size_t)((r + 1u) & 1u) * N;
    for (uint32_t i = blockIdx.x * REPORT_THREADS + threadIdx.x; i < N; i += gridDim.x * REPORT_THREADS) {
        uint64_t p = src[i];
        const uint32_t parent = (uint32_t)p, d = (uint32_t)(p >> 32);
        if (parent < N && !(d & TX_ROOTED)) {
            const uint64_t q = src[parent];
            const uint32_t dq = (uint32_t)(q >> 32);
            const uint64_t sum = (uint64_t)(d & TX_DIST_MAX) + (dq & TX_DIST_MAX);
            const uint32_t dist = (sum < TX_DIST_MAX ? (uint32_t)sum : TX_DIST_MAX) | (dq & TX_ROOTED);
            p = (uint64_t)(uint32_t)q | ((uint64_t)dist << 32);
        }
        dst[i] = p;
    }
}

// the agents of key's tree (counted by this workgroup) into the LDS hash, or the global size when its probes fail
__device__ __forceinline__ void tx_hash_add(uint32_t *keys, uint32_t *cnt, uint32_t *size, uint32_t key, uint32_t c) {
    const uint32_t h = (key * 2654435761u) >> 20;   // (12 bits: TX_HASH slots)
    for (uint32_t probe = 0; probe < TX_HASH_PROBES; probe++) {
        const uint32_t s = (h + probe) & (TX_HASH - 1u);
        const uint32_t k = atomicCAS(&keys[s], TX_MARK, key);
        if (k == TX_MARK || k == key) {
            atomicAdd(&cnt[s], c);
            return;
        }
    }
    atomicAdd(&size[key], c);
}

// k_tx_tally: 256 threads, one agent per thread, strided over the grid
template <bool GROUP>
__global__ __launch_bounds__(REPORT_THREADS) void k_tx_tally(const TxMember *M_, const TxMember one_, const TxArgs a) {
    static_assert(TX_HASH == 1u << 12, "tx_hash_add takes 12 bits");
    __shared__ uint32_t s_gen[REINA_TX_VARIANTS * REINA_TX_GENERATIONS];
    __shared__ uint32_t s_key[TX_HASH], s_cnt[TX_HASH];
    __shared__ uint32_t s_unconv, s_maxgen;
    const TxMember m = tx_member<GROUP>(M_, one_);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t k = tid; k < REINA_TX_VARIANTS * REINA_TX_GENERATIONS; k += REPORT_THREADS) s_gen[k] = 0u;
    for (uint32_t k = tid; k < TX_HASH; k += REPORT_THREADS) {
        s_key[k] = TX_MARK;
        s_cnt[k] = 0u;
    }
    if (tid == 0) s_unconv = s_maxgen = 0u;
    __syncthreads();
    const uint32_t N = a.p.n_agents;
    const uint64_t *pairs = m.pairs + (size_t)(tx_member_rounds(m, a) & 1u) * N;
    const uint32_t stride = gridDim.x * REPORT_THREADS;
    const uint32_t end = (N + REPORT_THREADS - 1u) / REPORT_THREADS * REPORT_THREADS;   // (whole waves run the loop)
    for (uint32_t i = blockIdx.x * REPORT_THREADS + tid; i < end; i += stride) {
        uint64_t p = (uint64_t)TX_MARK;
        uint32_t w = 0u;
        if (i < N) {
            p = pairs[i];
            w = m.hot[i];
        }
        const uint32_t parent = (uint32_t)p, d = (uint32_t)(p >> 32);
        const bool infected = parent != TX_MARK;
        const bool conv = infected && (d & TX_ROOTED) && parent < N;   // (every pair of an infected agent points below N)
        const uint32_t gen = d & TX_DIST_MAX;
        wave_count(s_gen, conv ? (int)(RH_VARIANT(w) * REINA_TX_GENERATIONS + (gen < 255u ? gen : 255u)) : -1);
        wave_tally(&s_unconv, infected && !conv);
        const uint32_t g = wave_max(conv ? gen : 0u);
        if (lane == 0 && g) atomicMax(&s_maxgen, g);
        // tree sizes: the lanes that share the first converged lane's root add once
        const uint32_t key = conv ? parent : TX_MARK;
        const uint64_t act = __ballot(conv);
        if (act) {
            const int lead = __ffsll((unsigned long long)act) - 1;
            const uint32_t lk = (uint32_t)__shfl((int)key, lead);
            const uint64_t same = __ballot(key == lk);
            if (key == lk) {
                if ((int)lane == lead) tx_hash_add(s_key, s_cnt, m.size, lk, (uint32_t)__popcll(same));
            } else if (conv) {
                tx_hash_add(s_key, s_cnt, m.size, key, 1u);
            }
        }
    }
    __syncthreads();
    GAS unsigned long long *R = (GAS unsigned long long *)m.report;
    for (uint32_t k = tid; k < TX_HASH; k += REPORT_THREADS)
        if (s_key[k] != TX_MARK) atomicAdd(&m.size[s_key[k]], s_cnt[k]);
    flush_lds(s_gen, REINA_TX_VARIANTS * REINA_TX_GENERATIONS, R + REINA_TX_GENERATION);
    if (tid == 0) {
        if (s_unconv) atomicAdd(&R[REINA_TX_SCALARS + REINA_TX_S_UNCONVERGED], (unsigned long long)s_unconv);
        if (s_maxgen) atomicMax(&R[REINA_TX_SCALARS + REINA_TX_S_MAX_GENERATION], (unsigned long long)s_maxgen);
    }
}

// k_tx_clusters: 256 threads, one agent per thread, strided over the grid; a non-zero size is a root's tree
template <bool GROUP>
__global__ __launch_bounds__(REPORT_THREADS) void k_tx_clusters(const TxMember *M_, const TxMember one_, const TxArgs a) {
    __shared__ uint32_t s_cl[REINA_TX_CLUSTER_BINS];
    __shared__ unsigned long long s_ca[REINA_TX_CLUSTER_BINS];
    __shared__ unsigned long long s_key;
    const TxMember m = tx_member<GROUP>(M_, one_);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < REINA_TX_CLUSTER_BINS) {
        s_cl[tid] = 0u;
        s_ca[tid] = 0ull;
    }
    if (tid == 0) s_key = 0ull;
    __syncthreads();
    const uint32_t N = a.p.n_agents;
    const uint32_t stride = gridDim.x * REPORT_THREADS;
    const uint32_t end = (N + REPORT_THREADS - 1u) / REPORT_THREADS * REPORT_THREADS;
    for (uint32_t i = blockIdx.x * REPORT_THREADS + tid; i < end; i += stride) {
        const uint32_t s = i < N ? m.size[i] : 0u;
        unsigned long long key = 0ull;
        if (s) {
            const uint32_t bin = 31u - (uint32_t)__clz((int)s);
            atomicAdd(&s_cl[bin], 1u);
            atomicAdd(&s_ca[bin], (unsigned long long)s);
            key = ((unsigned long long)s << 32) | (unsigned long long)(~i);
        }
        key = wave_max(key);
        if (lane == 0 && key) atomicMax(&s_key, key);
    }
    __syncthreads();
    GAS unsigned long long *R = (GAS unsigned long long *)m.report;
    flush_lds(s_cl, REINA_TX_CLUSTER_BINS, R + REINA_TX_CLUSTERS);
    flush_lds(s_ca, REINA_TX_CLUSTER_BINS, R + REINA_TX_CLUSTER_AGENTS);
    if (tid == 0 && s_key) atomicMax(&R[REINA_TX_SCALARS + REINA_TX_S_LARGEST_KEY], s_key);
}

// k_tx_finish: one lane per member (grid.y)
template <bool GROUP>
__global__ __launch_bounds__(64) void k_tx_finish(const TxMember *M_, const TxMember one_, const TxArgs a) {
    const TxMember m = tx_member<GROUP>(M_, one_);
    if (threadIdx.x != 0) return;
    uint64_t *S = m.report + REINA_TX_SCALARS;
    uint64_t sum = 0;
    for (uint32_t k = 0; k < TX_SUMS; k++) sum += m.report[REINA_TX_OFFSPRING_SUM + k];
    const uint64_t key = S[REINA_TX_S_LARGEST_KEY];
    S[REINA_TX_S_SUM_N_INFECTED] = sum;
    S[REINA_TX_S_ROUNDS] = tx_member_rounds(m, a);
    S[REINA_TX_S_LARGEST_CLUSTER] = key >> 32;
    S[REINA_TX_S_LARGEST_ROOT] = key ? (uint64_t)(uint32_t)~(uint32_t)key : ~0ull;
}

// ---------------------------------------------------------------------------------------------
// host side

static int tx_args(const reina_engine_t *e, const uint8_t *age_group, uint32_t n_groups, uint32_t max_depth, TxArgs *a) {
    a->host_rounds = max_depth ? tx_rounds(max_depth) : 0xFFFFFFFFu;
    return age_group_args(e, age_group, n_groups, REINA_TX_MAX_GROUPS, "reina_tx_report", &a->p);
}

// every pass of a report: the K members of the device table `d_m`, or (d_m = nullptr) the one member `one`
static int tx_launch(const TxMember *d_m, const TxMember &one, const TxArgs &a, uint32_t K, uint32_t n_cus, uint64_t *report, hipStream_t s) {
    HIP_CHECK(hipMemsetAsync(report, 0, (size_t)K * REINA_TX_REPORT_WORDS * 8u, s));
    const ForestPasses f = forest_passes(a.p.n_agents, K, n_cus, a.host_rounds);
    launch_members(k_tx_links, d_m, f.g_links, K, REPORT_THREADS, s, d_m, one, a);
    for (uint32_t r = 0; r < f.rounds; r++) launch_members(k_tx_jump, d_m, f.g_jump, K, REPORT_THREADS, s, d_m, one, a, r);
    launch_members(k_tx_tally, d_m, f.g_tally, K, REPORT_THREADS, s, d_m, one, a);
    launch_members(k_tx_clusters, d_m, f.g_tally, K, REPORT_THREADS, s, d_m, one, a);
    launch_members(k_tx_finish, d_m, 1u, K, 64, s, d_m, one, a);
    return REINA_OK;
}

extern "C" {

int reina_tx_version(void) { return REINA_TX_VERSION; }

int reina_tx_report(reina_engine_t *e, const uint8_t *age_group, uint32_t n_groups, uint32_t max_depth, void *dev_scratch,
                    uint64_t *dev_report, void *stream) {
    if (int rc = tx_engine_ok(e)) return rc;
    if (!tx_aligned(dev_scratch) || !tx_aligned(dev_report)) return refuse("reina_tx_report: scratch and report must be 16-byte aligned device buffers");
    TxArgs a;
    if (int rc = tx_args(e, age_group, n_groups, max_depth, &a)) return rc;
    return tx_launch(nullptr, tx_member_of(e, dev_scratch, dev_report), a, 1u, e->n_cus, dev_report, (hipStream_t)stream);
}

int reina_group_tx_report(reina_group_t *g, const uint8_t *age_group, uint32_t n_groups, uint32_t max_depth,
                          void *const *dev_scratch, uint64_t *dev_report, void *stream) {
    if (!g || g->members.empty() || !dev_scratch) return REINA_E_INVALID;
    if (!tx_aligned(dev_report)) return refuse("reina_group_tx_report: the reports must be a 16-byte aligned device buffer");
    std::vector<TxMember> h;
    if (int rc = member_table(g->members, dev_scratch, dev_report, REINA_TX_REPORT_WORDS, "reina_group_tx_report", &h)) return rc;
    TxArgs a;
    if (int rc = tx_args(g->members[0], age_group, n_groups, max_depth, &a)) return rc;
    hipStream_t s = (hipStream_t)stream;
    return with_member_table(h, "reina_group_tx_report", s, [&](const TxMember *d_m) {
        return tx_launch(d_m, h[0], a, (uint32_t)h.size(), g->members[0]->n_cus, dev_report, s);
    });
}

}  // extern "C"
