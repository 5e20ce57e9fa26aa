// reina_hip.hip part: transmission-tree reports of an unsharded engine between two days (include/reina_transmission.h;
// DESIGN.md "Transmission reports").  Included at the end of reina_hip.hip (it uses the host helpers and the group above).
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

#define TX_THREADS 256
#define TX_TILE 512u
#define TX_MARK 0xFFFFFFFFu        // parent of an agent that is not infected (and an empty hash slot)
#define TX_ROOTED 0x80000000u      // distance word: the parent is a root
#define TX_DIST_MAX 0x7FFFFFFFu    // distances saturate (a cycle of bad data doubles them every round)
#define TX_HASH 4096u              // k_tx_tally's LDS hash slots
#define TX_HASH_PROBES 8
#define TX_DAY_ROUNDS 13u          // ceil(log2(REINA_MAX_DAYS + 1 + 1)): the most rounds the day word can ask for
#define TX_CELLS (REINA_TX_VARIANTS * REINA_TX_SEVERITIES * REINA_TX_OUTCOMES * 2u * REINA_TX_BINS)
#define TX_MATRIX_CELLS (REINA_TX_VARIANTS * REINA_TX_MAX_GROUPS * REINA_TX_MAX_GROUPS)
#define TX_SUMS (REINA_TX_VARIANTS * REINA_TX_OUTCOMES)
static_assert(REINA_TX_OFFSPRING_SUM == TX_CELLS && REINA_TX_REPORT_WORDS == 9834u, "report layout");
static_assert(REINA_MAX_VARIANTS == REINA_TX_VARIANTS, "RH_VARIANT has two bits");
static_assert((1u << (TX_DAY_ROUNDS - 1u)) < REINA_MAX_DAYS + 2u && (1u << TX_DAY_ROUNDS) >= REINA_MAX_DAYS + 2u, "day rounds");

struct TxMember {
    const uint32_t *hot;
    const reina_cold_t *cold;
    const int32_t *counters;
    uint64_t *pairs;     // [2][n_agents] (parent | distance << 32)
    uint32_t *size;      // [n_agents] agents in the tree of each root
    uint64_t *report;    // [REINA_TX_REPORT_WORDS]
};
static_assert(sizeof(TxMember) % 8 == 0, "copied as 64-bit words");

struct TxArgs {
    uint32_t n_agents, nr_ages, host_rounds;   // host_rounds ~0: from the member's day word
    int32_t age_start[REINA_MAX_AGES + 1];
    uint8_t group[REINA_MAX_AGES];
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
    const CAS uint64_t *s = (const CAS uint64_t *)(M_ + blockIdx.y);
    uint64_t *d = reinterpret_cast<uint64_t *>(&m);
#pragma unroll
    for (size_t k = 0; k < sizeof(TxMember) / 8; k++) d[k] = s[k];
    return m;
}

__device__ __forceinline__ uint32_t tx_member_rounds(const TxMember &m, const TxArgs &a) {
    if (a.host_rounds != 0xFFFFFFFFu) return a.host_rounds;
    int32_t day = m.counters[SC_IDX(REINA_S_DAY)];
    day = day < 0 ? 0 : (day > (int32_t)REINA_MAX_DAYS ? (int32_t)REINA_MAX_DAYS : day);
    return tx_rounds((uint64_t)day + 1u);
}

// +1 in LDS histogram cell b of every lane with b >= 0; the lanes that share the first such lane's cell add once.
// Called by whole waves.
__device__ __forceinline__ void tx_count(uint32_t *hist, int b) {
    const uint64_t act = __ballot(b >= 0);
    if (!act) return;
    const int lead = __ffsll((unsigned long long)act) - 1;
    const int lb = __shfl(b, lead);
    const uint64_t same = __ballot(b == lb);
    if (b == lb) {
        if ((int)(threadIdx.x & 63u) == lead) atomicAdd(&hist[lb], (uint32_t)__popcll(same));
    } else if (b >= 0) {
        atomicAdd(&hist[b], 1u);
    }
}

// ---------------------------------------------------------------------------------------------
// k_tx_links: 256 threads, tiles of 512 agents (two per thread), the workgroup's tiles strided over the grid
template <bool GROUP>
__global__ __launch_bounds__(TX_THREADS) void k_tx_links(const TxMember *M_, const TxMember one_, const TxArgs a) {
    __shared__ uint32_t s_off[TX_CELLS];
    __shared__ uint32_t s_mat[TX_MATRIX_CELLS];
    __shared__ unsigned long long s_sum[TX_SUMS], s_sq[TX_SUMS];
    __shared__ uint32_t s_cnt[4];   // infected, roots, linked, bad links
    __shared__ int32_t s_as[REINA_MAX_AGES + 1];
    __shared__ uint8_t s_grp[REINA_MAX_AGES];
    const TxMember m = tx_member<GROUP>(M_, one_);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t k = tid; k < TX_CELLS; k += TX_THREADS) s_off[k] = 0u;
    for (uint32_t k = tid; k < TX_MATRIX_CELLS; k += TX_THREADS) s_mat[k] = 0u;
    if (tid < TX_SUMS) s_sum[tid] = s_sq[tid] = 0ull;
    if (tid < 4) s_cnt[tid] = 0u;
    if (tid <= REINA_MAX_AGES) s_as[tid] = a.age_start[tid];
    if (tid < REINA_MAX_AGES) s_grp[tid] = a.group[tid];
    __syncthreads();
    const uint32_t N = a.n_agents, tiles = (N + TX_TILE - 1u) / TX_TILE;
    const int top = (int)a.nr_ages - 1;
    uint64_t *pairs = m.pairs;
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        uint32_t idx[2], w[2];
        bool inf[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            idx[j] = t * TX_TILE + (uint32_t)j * TX_THREADS + tid;
            w[j] = idx[j] < N ? m.hot[idx[j]] : 0u;
            inf[j] = RH_STATE(w[j]) != RS_SUSCEPTIBLE;
        }
        int32_t src[2] = {-1, -1};
        uint32_t n[2] = {0u, 0u};
#pragma unroll
        for (int j = 0; j < 2; j++) {
            if (inf[j]) {
                const v2u_ c = *reinterpret_cast<const v2u_ *>(&m.cold[idx[j]].infector);   // infector, n_infected
                src[j] = (int32_t)c.x;
                n[j] = c.y;
            }
        }
        uint32_t sw[2] = {0u, 0u};
#pragma unroll
        for (int j = 0; j < 2; j++)
            if (inf[j] && src[j] >= 0 && (uint32_t)src[j] < N && (uint32_t)src[j] != idx[j]) sw[j] = m.hot[src[j]];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint32_t i = idx[j], st = RH_STATE(w[j]), v = RH_VARIANT(w[j]);
            const uint32_t sev = RH_SEV(w[j]) < 4u ? RH_SEV(w[j]) : 4u;
            const uint32_t o = st <= RS_IN_ICU ? 0u : ((w[j] & RH_INCLUDED) ? 1u : 2u);
            const uint32_t det = (w[j] & RH_DETECTED) ? 1u : 0u;
            const bool root = inf[j] && src[j] == -1;
            const bool linked = inf[j] && !root && RH_STATE(sw[j]) != RS_SUSCEPTIBLE;   // (sw = 0 for an infector out of range or itself)
            const bool bad = inf[j] && !root && !linked;
            tx_count(s_off, inf[j] ? (int)((((v * REINA_TX_SEVERITIES + sev) * REINA_TX_OUTCOMES + o) * 2u + det) * REINA_TX_BINS +
                                           (n[j] < REINA_TX_BINS - 1u ? n[j] : REINA_TX_BINS - 1u))
                                   : -1);
            if (inf[j] && n[j]) {
                atomicAdd(&s_sum[v * REINA_TX_OUTCOMES + o], (unsigned long long)n[j]);
                atomicAdd(&s_sq[v * REINA_TX_OUTCOMES + o], (unsigned long long)n[j] * n[j]);
            }
            if (linked) {
                const uint32_t gs = s_grp[age_of(s_as, i, 0, top)], gi = s_grp[age_of(s_as, (uint32_t)src[j], 0, top)];
                atomicAdd(&s_mat[(v * REINA_TX_MAX_GROUPS + gi) * REINA_TX_MAX_GROUPS + gs], 1u);
            }
            const uint32_t ci = (uint32_t)__popcll(__ballot(inf[j])), cr = (uint32_t)__popcll(__ballot(root));
            const uint32_t cl = (uint32_t)__popcll(__ballot(linked)), cb = (uint32_t)__popcll(__ballot(bad));
            if (lane == 0) {
                if (ci) atomicAdd(&s_cnt[0], ci);
                if (cr) atomicAdd(&s_cnt[1], cr);
                if (cl) atomicAdd(&s_cnt[2], cl);
                if (cb) atomicAdd(&s_cnt[3], cb);
            }
            if (i < N) {
                const uint64_t p = !inf[j] ? (uint64_t)TX_MARK
                                 : linked  ? ((uint64_t)(uint32_t)src[j] | (1ull << 32))
                                           : ((uint64_t)i | ((uint64_t)TX_ROOTED << 32));
                pairs[i] = p;
                m.size[i] = 0u;
            }
        }
    }
    __syncthreads();
    uint64_t *R = m.report;
    for (uint32_t k = tid; k < TX_CELLS; k += TX_THREADS)
        if (s_off[k]) atomicAdd((unsigned long long *)&R[REINA_TX_OFFSPRING + k], (unsigned long long)s_off[k]);
    for (uint32_t k = tid; k < TX_MATRIX_CELLS; k += TX_THREADS)
        if (s_mat[k]) atomicAdd((unsigned long long *)&R[REINA_TX_MATRIX + k], (unsigned long long)s_mat[k]);
    if (tid < TX_SUMS) {
        if (s_sum[tid]) atomicAdd((unsigned long long *)&R[REINA_TX_OFFSPRING_SUM + tid], s_sum[tid]);
        if (s_sq[tid]) atomicAdd((unsigned long long *)&R[REINA_TX_OFFSPRING_SUMSQ + tid], s_sq[tid]);
    }
    if (tid < 4 && s_cnt[tid]) {
        const uint32_t at[4] = {REINA_TX_S_N_INFECTED_AGENTS, REINA_TX_S_N_ROOTS, REINA_TX_S_N_LINKED, REINA_TX_S_BAD_LINKS};
        atomicAdd((unsigned long long *)&R[REINA_TX_SCALARS + at[tid]], (unsigned long long)s_cnt[tid]);
    }
}

// k_tx_jump: round r of pointer jumping, one thread per agent (grid-strided)
template <bool GROUP>
__global__ __launch_bounds__(TX_THREADS) void k_tx_jump(const TxMember *M_, const TxMember one_, const TxArgs a, uint32_t r) {
    const TxMember m = tx_member<GROUP>(M_, one_);
    if (r >= tx_member_rounds(m, a)) return;
    const uint32_t N = a.n_agents;
    const uint64_t *src = m.pairs + (size_t)(r & 1u) * N;
    uint64_t *dst = m.pairs + (size_t)((r + 1u) & 1u) * N;
    for (uint32_t i = blockIdx.x * TX_THREADS + threadIdx.x; i < N; i += gridDim.x * TX_THREADS) {
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
__global__ __launch_bounds__(TX_THREADS) void k_tx_tally(const TxMember *M_, const TxMember one_, const TxArgs a) {
    static_assert(TX_HASH == 1u << 12, "tx_hash_add takes 12 bits");
    __shared__ uint32_t s_gen[REINA_TX_VARIANTS * REINA_TX_GENERATIONS];
    __shared__ uint32_t s_key[TX_HASH], s_cnt[TX_HASH];
    __shared__ uint32_t s_unconv, s_maxgen;
    const TxMember m = tx_member<GROUP>(M_, one_);
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    for (uint32_t k = tid; k < REINA_TX_VARIANTS * REINA_TX_GENERATIONS; k += TX_THREADS) s_gen[k] = 0u;
    for (uint32_t k = tid; k < TX_HASH; k += TX_THREADS) {
        s_key[k] = TX_MARK;
        s_cnt[k] = 0u;
    }
    if (tid == 0) s_unconv = s_maxgen = 0u;
    __syncthreads();
    const uint32_t N = a.n_agents;
    const uint64_t *pairs = m.pairs + (size_t)(tx_member_rounds(m, a) & 1u) * N;
    const uint32_t stride = gridDim.x * TX_THREADS;
    const uint32_t end = (N + TX_THREADS - 1u) / TX_THREADS * TX_THREADS;   // (whole waves run the loop)
    for (uint32_t i = blockIdx.x * TX_THREADS + tid; i < end; i += stride) {
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
        tx_count(s_gen, conv ? (int)(RH_VARIANT(w) * REINA_TX_GENERATIONS + (gen < 255u ? gen : 255u)) : -1);
        const uint32_t nu = (uint32_t)__popcll(__ballot(infected && !conv));
        uint32_t g = conv ? gen : 0u;
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)g, off);
            g = o > g ? o : g;
        }
        if (lane == 0) {
            if (nu) atomicAdd(&s_unconv, nu);
            if (g) atomicMax(&s_maxgen, g);
        }
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
    uint64_t *R = m.report;
    for (uint32_t k = tid; k < TX_HASH; k += TX_THREADS)
        if (s_key[k] != TX_MARK) atomicAdd(&m.size[s_key[k]], s_cnt[k]);
    for (uint32_t k = tid; k < REINA_TX_VARIANTS * REINA_TX_GENERATIONS; k += TX_THREADS)
        if (s_gen[k]) atomicAdd((unsigned long long *)&R[REINA_TX_GENERATION + k], (unsigned long long)s_gen[k]);
    if (tid == 0) {
        if (s_unconv) atomicAdd((unsigned long long *)&R[REINA_TX_SCALARS + REINA_TX_S_UNCONVERGED], (unsigned long long)s_unconv);
        if (s_maxgen) atomicMax((unsigned long long *)&R[REINA_TX_SCALARS + REINA_TX_S_MAX_GENERATION], (unsigned long long)s_maxgen);
    }
}

// k_tx_clusters: 256 threads, one agent per thread, strided over the grid; a non-zero size is a root's tree
template <bool GROUP>
__global__ __launch_bounds__(TX_THREADS) void k_tx_clusters(const TxMember *M_, const TxMember one_, const TxArgs a) {
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
    const uint32_t N = a.n_agents;
    const uint32_t stride = gridDim.x * TX_THREADS;
    const uint32_t end = (N + TX_THREADS - 1u) / TX_THREADS * TX_THREADS;
    for (uint32_t i = blockIdx.x * TX_THREADS + tid; i < end; i += stride) {
        const uint32_t s = i < N ? m.size[i] : 0u;
        unsigned long long key = 0ull;
        if (s) {
            const uint32_t bin = 31u - (uint32_t)__clz((int)s);
            atomicAdd(&s_cl[bin], 1u);
            atomicAdd(&s_ca[bin], (unsigned long long)s);
            key = ((unsigned long long)s << 32) | (unsigned long long)(~i);
        }
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), off);
            const unsigned long long o = ((unsigned long long)hi << 32) | lo;
            key = o > key ? o : key;
        }
        if (lane == 0 && key) atomicMax(&s_key, key);
    }
    __syncthreads();
    uint64_t *R = m.report;
    if (tid < REINA_TX_CLUSTER_BINS && s_cl[tid]) {
        atomicAdd((unsigned long long *)&R[REINA_TX_CLUSTERS + tid], (unsigned long long)s_cl[tid]);
        atomicAdd((unsigned long long *)&R[REINA_TX_CLUSTER_AGENTS + tid], s_ca[tid]);
    }
    if (tid == 0 && s_key) atomicMax((unsigned long long *)&R[REINA_TX_SCALARS + REINA_TX_S_LARGEST_KEY], s_key);
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

static int tx_engine_ok(const reina_engine_t *e) {
    if (!e) return REINA_E_INVALID;
    if (!e->bound) return REINA_E_NOT_BOUND;
    if (e->cfg.n_shards > 1 || e->exact) {
        g_last_error = "transmission reports are taken of unsharded engines only";
        return REINA_E_INVALID;
    }
    return REINA_OK;
}

static int tx_args(const reina_engine_t *e, const uint8_t *age_group, uint32_t n_groups, uint32_t max_depth, TxArgs *a) {
    if (!age_group || n_groups < 1u || n_groups > REINA_TX_MAX_GROUPS) {
        g_last_error = "reina_tx_report: age_group must be a table of groups, 1 <= n_groups <= REINA_TX_MAX_GROUPS";
        return REINA_E_INVALID;
    }
    std::memset(a, 0, sizeof(*a));
    a->n_agents = e->cfg.n_agents;
    a->nr_ages = e->cfg.nr_ages;
    a->host_rounds = max_depth ? tx_rounds(max_depth) : 0xFFFFFFFFu;
    std::memcpy(a->age_start, e->cfg.age_start, sizeof(a->age_start));
    for (uint32_t k = 0; k < e->cfg.nr_ages; k++) {
        if (age_group[k] >= n_groups) {
            g_last_error = "reina_tx_report: an age's group is not below n_groups";
            return REINA_E_INVALID;
        }
        a->group[k] = age_group[k];
    }
    return REINA_OK;
}

static bool tx_aligned(const void *p) { return p && ((uintptr_t)p & 15u) == 0u; }

static TxMember tx_member_of(const reina_engine_t *e, void *scratch, uint64_t *report) {
    TxMember m;
    m.hot = e->buf.hot;
    m.cold = e->buf.cold;
    m.counters = e->buf.counters;
    m.pairs = static_cast<uint64_t *>(scratch);
    m.size = reinterpret_cast<uint32_t *>(static_cast<char *>(scratch) + 16u * (size_t)e->cfg.n_agents);
    m.report = report;
    return m;
}

// every pass of a report: members = 1 (`one`) or the K members of the device table `d_m`
template <bool GROUP>
static int tx_launch(const TxMember *d_m, const TxMember &one, const TxArgs &a, uint32_t K, uint32_t n_cus, uint64_t *report, hipStream_t s) {
    HIP_CHECK(hipMemsetAsync(report, 0, (size_t)K * REINA_TX_REPORT_WORDS * 8u, s));
    const uint32_t N = a.n_agents;
    const uint32_t tiles = (N + TX_TILE - 1u) / TX_TILE, waves = (N + TX_THREADS - 1u) / TX_THREADS;
    uint32_t per = 4u * n_cus / K;   // workgroups per member of the passes that flush LDS tables
    if (per < 1u) per = 1u;
    const uint32_t g_links = tiles < per ? (tiles ? tiles : 1u) : per;
    const uint32_t g_tally = waves < per ? (waves ? waves : 1u) : per;
    const uint32_t g_jump = waves < 32768u ? (waves ? waves : 1u) : 32768u;
    hipLaunchKernelGGL((k_tx_links<GROUP>), dim3(g_links, K), dim3(TX_THREADS), 0, s, d_m, one, a);
    HIP_CHECK(hipGetLastError());
    const uint32_t rounds = a.host_rounds != 0xFFFFFFFFu ? a.host_rounds : TX_DAY_ROUNDS;
    for (uint32_t r = 0; r < rounds; r++) {
        hipLaunchKernelGGL((k_tx_jump<GROUP>), dim3(g_jump, K), dim3(TX_THREADS), 0, s, d_m, one, a, r);
        HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL((k_tx_tally<GROUP>), dim3(g_tally, K), dim3(TX_THREADS), 0, s, d_m, one, a);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((k_tx_clusters<GROUP>), dim3(g_tally, K), dim3(TX_THREADS), 0, s, d_m, one, a);
    HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((k_tx_finish<GROUP>), dim3(1, K), dim3(64), 0, s, d_m, one, a);
    HIP_CHECK(hipGetLastError());
    return REINA_OK;
}

extern "C" {

int reina_tx_version(void) { return REINA_TX_VERSION; }

int reina_tx_report(reina_engine_t *e, const uint8_t *age_group, uint32_t n_groups, uint32_t max_depth, void *dev_scratch,
                    uint64_t *dev_report, void *stream) {
    if (int rc = tx_engine_ok(e)) return rc;
    if (!tx_aligned(dev_scratch) || !tx_aligned(dev_report)) {
        g_last_error = "reina_tx_report: scratch and report must be 16-byte aligned device buffers";
        return REINA_E_INVALID;
    }
    TxArgs a;
    if (int rc = tx_args(e, age_group, n_groups, max_depth, &a)) return rc;
    return tx_launch<false>(nullptr, tx_member_of(e, dev_scratch, dev_report), a, 1u, e->n_cus, dev_report, (hipStream_t)stream);
}

int reina_group_tx_report(reina_group_t *g, const uint8_t *age_group, uint32_t n_groups, uint32_t max_depth,
                          void *const *dev_scratch, uint64_t *dev_report, void *stream) {
    if (!g || g->members.empty() || !dev_scratch) return REINA_E_INVALID;
    if (!tx_aligned(dev_report)) {
        g_last_error = "reina_group_tx_report: the reports must be a 16-byte aligned device buffer";
        return REINA_E_INVALID;
    }
    const uint32_t K = (uint32_t)g->members.size();
    std::vector<TxMember> h(K);
    for (uint32_t k = 0; k < K; k++) {
        if (int rc = tx_engine_ok(g->members[k])) return rc;
        if (!tx_aligned(dev_scratch[k])) {
            g_last_error = "reina_group_tx_report: every member's scratch must be a 16-byte aligned device buffer";
            return REINA_E_INVALID;
        }
        h[k] = tx_member_of(g->members[k], dev_scratch[k], dev_report + (size_t)k * REINA_TX_REPORT_WORDS);
    }
    TxArgs a;
    if (int rc = tx_args(g->members[0], age_group, n_groups, max_depth, &a)) return rc;
    hipStream_t s = (hipStream_t)stream;
    TxMember *d_m = nullptr;
    HIP_CHECK(hipMalloc(&d_m, sizeof(TxMember) * K));
    int rc = REINA_OK;
    if (hipMemcpyAsync(d_m, h.data(), sizeof(TxMember) * K, hipMemcpyHostToDevice, s) != hipSuccess) {
        g_last_error = "reina_group_tx_report: member table upload failed";
        rc = REINA_E_HIP;
    }
    if (rc == REINA_OK) rc = tx_launch<true>(d_m, h[0], a, K, g->members[0]->n_cus, dev_report, s);
    // (the member table and its host copy live until the passes have run)
    const hipError_t se = hipStreamSynchronize(s);
    (void)hipFree(d_m);
    if (rc == REINA_OK && se != hipSuccess) {
        g_last_error = std::string("reina_group_tx_report: ") + hipGetErrorString(se);
        rc = REINA_E_HIP;
    }
    return rc;
}

}  // extern "C"
