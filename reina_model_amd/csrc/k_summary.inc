// reina_hip.hip part: ensemble summaries -- quantile bands, sums, peaks and exceedance of the members' counter histories
// (include/reina_summary.h; DESIGN.md section 6j).  Included at the end of reina_hip.hip, behind k_addons.inc (the wave
// helpers).  The summary takes no engine: it reads history rows and writes nothing but the caller's scratch and report block.
//
// Scratch = head | series.  The head (SumHead, then the K member pointers) is filled on the host in a page-locked slot and
// copied by a kernel on the stream, as the contact tables are (stage_upload): the call never waits.  The series are int32
// [days][K][S]: a row's S values lie together, so the pass that streams the rows writes them coalesced, the pass over the days
// reads a (member, series) item's neighbours together, and the pass over the members reads runs of SUM_TILE series a member.
//   k_summary_head    the head from the page-locked slot into the scratch
//   k_summary_series  one wave a history row (7.3 KB, 16-byte loads): the 128 ages of a counter lie in 32 lanes, which reduce
//                     them to the G group sums by shuffles; the total is the sum of the group sums
//   k_summary_peak    256 threads = 16 (member, series) items x 16 slices of the days: a 64-bit maximum of
//                     (value biased to unsigned) << 32 | ~day gives the peak and its first day (the size << 32 | ~root idiom
//                     of the tree reports); the items behind K * S are the thresholds' (threshold, member) pairs, whose
//                     maximum of ~day over the days above the value gives the first such day
//   k_summary_order   a workgroup per (day, SUM_TILE series): the K values of each series into LDS, padded to a power of two
//                     with INT32_MAX; the 64-bit sums and the threshold counts are taken there, then a bitonic network in
//                     LDS sorts the tile's series side by side and the ranks are read off.  Every index into a per-lane
//                     value is known at compile time: nothing goes to scratch memory.
#include "../../include/reina_summary.h"

#define SUM_THREADS 256
#define SUM_TILE 8u              // series a workgroup of k_summary_order sorts
#define SUM_ROW_VEC (REINA_COUNTER_WORDS / 4u)   // 16-byte pieces of a history row
static_assert(REINA_COUNTER_WORDS % 4 == 0 && REINA_MAX_AGES == 128 && REINA_C_NR % 2 == 0 && REINA_S_NR == 32,
              "k_summary_series: two counters a round of 64 lanes, the scalars in 8 lanes");
static_assert(REINA_SUMMARY_SERIES(REINA_SUMMARY_MAX_GROUPS) == 270u && REINA_SUMMARY_HEAD_BYTES(1024) == 8704u &&
              REINA_SUMMARY_REPORT_WORDS(3, 5, 46, 2, 4) == 5u * 46u * 2u + 5u * 46u + 3u * 46u * 3u + 4u * 5u + 4u * 3u, "summary layout");

struct SumHead {
    uint32_t ranks[REINA_SUMMARY_MAX_RANKS];
    uint32_t thr_series[REINA_SUMMARY_MAX_THRESHOLDS];
    int32_t thr_value[REINA_SUMMARY_MAX_THRESHOLDS];
    uint8_t group[REINA_MAX_AGES];   // (0 for the ages >= nr_ages, which are masked)
    uint8_t pad[512 - 4 * REINA_SUMMARY_MAX_RANKS - 8 * REINA_SUMMARY_MAX_THRESHOLDS - REINA_MAX_AGES];
};
static_assert(sizeof(SumHead) == 512, "the member pointers sit at byte 512 of the head");

struct SumArgs {
    uint32_t K, days, nr_ages, G, S, Q, T;
};

__global__ __launch_bounds__(SUM_THREADS) void k_summary_head(uint64_t *dst, const uint64_t *src, uint32_t n) {
    for (uint32_t k = blockIdx.x * SUM_THREADS + threadIdx.x; k < n; k += gridDim.x * SUM_THREADS) dst[k] = src[k];
}

// sum over the 32 lanes of a half wave, in every lane of it
__device__ __forceinline__ uint32_t half_wave_sum(uint32_t x) {
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) x += (uint32_t)__shfl_xor((int)x, off);
    return x;
}

// one wave a row; row = day * K + member
__global__ __launch_bounds__(SUM_THREADS) void k_summary_series(const SumHead *head, int32_t *series, const SumArgs a) {
    __shared__ uint8_t s_grp[REINA_MAX_AGES];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, hl = lane & 31u;
    if (tid < REINA_MAX_AGES) s_grp[tid] = head->group[tid];
    __syncthreads();
    const size_t rows = (size_t)a.K * a.days;
    const size_t row = (size_t)blockIdx.x * (SUM_THREADS / 64u) + (tid >> 6);
    if (row >= rows) return;
    const uint32_t d = (uint32_t)(row / a.K), m = (uint32_t)(row % a.K);
    const int32_t *const *bases = reinterpret_cast<const int32_t *const *>(head + 1);
    const v4u_ *src = reinterpret_cast<const v4u_ *>(bases[m] + (size_t)d * REINA_COUNTER_WORDS);
    int32_t *out = series + row * a.S;
    // every piece of the row in flight at once: piece lane + 64 * i holds four ages of counter 2 * i + lane / 32
    v4u_ v[REINA_C_NR / 2];
#pragma unroll
    for (int i = 0; i < REINA_C_NR / 2; i++) v[i] = src[lane + 64u * (uint32_t)i];
    v4u_ sc = {0u, 0u, 0u, 0u};
    if (lane < REINA_S_NR / 4u) sc = src[REINA_C_NR * REINA_MAX_AGES / 4u + lane];
    const uint32_t a0 = 4u * hl;
    const uint32_t g0 = s_grp[a0], g1 = s_grp[a0 + 1u], g2 = s_grp[a0 + 2u], g3 = s_grp[a0 + 3u];
    const bool in0 = a0 < a.nr_ages, in1 = a0 + 1u < a.nr_ages, in2 = a0 + 2u < a.nr_ages, in3 = a0 + 3u < a.nr_ages;
#pragma unroll
    for (int i = 0; i < REINA_C_NR / 2; i++) {
        const uint32_t x0 = in0 ? v[i].x : 0u, x1 = in1 ? v[i].y : 0u, x2 = in2 ? v[i].z : 0u, x3 = in3 ? v[i].w : 0u;
        uint32_t total = 0u, mine = 0u;
        for (uint32_t g = 0; g < a.G; g++) {
            const uint32_t s = half_wave_sum((g0 == g ? x0 : 0u) + (g1 == g ? x1 : 0u) + (g2 == g ? x2 : 0u) + (g3 == g ? x3 : 0u));
            total += s;
            if (hl == g) mine = s;
        }
        int32_t *o = out + (2u * (uint32_t)i + (lane >> 5)) * (1u + a.G);
        if (hl == 0u) o[0] = (int32_t)total;
        if (hl < a.G) o[1u + hl] = (int32_t)mine;
    }
    if (lane < REINA_S_NR / 4u) {
        int32_t *o = out + REINA_C_NR * (1u + a.G) + 4u * lane;   // (S * 4 bytes is no multiple of 16: word stores)
        o[0] = (int32_t)sc.x;
        o[1] = (int32_t)sc.y;
        o[2] = (int32_t)sc.z;
        o[3] = (int32_t)sc.w;
    }
}

// 16 items a workgroup (threadIdx.x & 15), each by 16 slices of the days (threadIdx.x >> 4)
__global__ __launch_bounds__(SUM_THREADS) void k_summary_peak(const SumHead *head, const int32_t *series, int64_t *report, const SumArgs a) {
    __shared__ unsigned long long s_key[16][16];
    const uint32_t tid = threadIdx.x, it = tid & 15u, slice = tid >> 4;
    const size_t KS = (size_t)a.K * a.S, items = KS + (size_t)a.T * a.K;
    const size_t item = (size_t)blockIdx.x * 16u + it;
    const bool valid = item < items, thr = item >= KS;
    uint32_t m = 0u, s = 0u, t = 0u;
    int32_t value = 0;
    if (valid && !thr) {
        m = (uint32_t)(item / a.S);
        s = (uint32_t)(item % a.S);
    } else if (valid) {
        t = (uint32_t)((item - KS) / a.K);
        m = (uint32_t)((item - KS) % a.K);
        s = head->thr_series[t];
        value = head->thr_value[t];
    }
    const size_t day_stride = KS;
    const int32_t *p = series + (size_t)m * a.S + s;
    unsigned long long key = 0ull;   // (below every key of a day: ~day is never 0)
    if (valid)
#pragma unroll 4
        for (uint32_t d = slice; d < a.days; d += 16u) {
            const int32_t x = p[(size_t)d * day_stride];
            const unsigned long long k = thr ? (x > value ? (unsigned long long)(uint32_t)~d : 0ull)
                                             : (((unsigned long long)((uint32_t)x ^ 0x80000000u) << 32) | (unsigned long long)(uint32_t)~d);
            key = k > key ? k : key;
        }
    s_key[slice][it] = key;
    __syncthreads();
    if (slice != 0u || !valid) return;
#pragma unroll
    for (int j = 1; j < 16; j++) key = s_key[j][it] > key ? s_key[j][it] : key;
    if (!thr) {
        int64_t *pk = report + REINA_SUMMARY_PEAK(a.K, a.days, a.S, a.Q, a.T) + item * REINA_SUMMARY_PEAK_FIELDS;
        pk[0] = (int64_t)(int32_t)((uint32_t)(key >> 32) ^ 0x80000000u);
        pk[1] = (int64_t)(uint32_t)~(uint32_t)key;
        report[REINA_SUMMARY_FINAL(a.K, a.days, a.S, a.Q, a.T) + item] = (int64_t)p[(size_t)(a.days - 1u) * day_stride];
    } else {
        report[REINA_SUMMARY_FIRST_EXCEED(a.K, a.days, a.S, a.Q, a.T) + (size_t)t * a.K + m] = key ? (int64_t)(uint32_t)~(uint32_t)key : -1ll;
    }
}

// grid (tiles of SUM_TILE series, days); KP: the LDS row, a power of two >= the members padded to a power of two (kp, >= 2)
template <uint32_t KP>
__global__ __launch_bounds__(SUM_THREADS) void k_summary_order(const SumHead *head, const int32_t *series, int64_t *report, const SumArgs a,
                                                               const uint32_t kp, const uint32_t log2_kp) {
    __shared__ int32_t s_val[SUM_TILE][KP];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t tile = blockIdx.x, d = blockIdx.y, s0 = tile * SUM_TILE, K = a.K, S = a.S;
    const int32_t *day = series + (size_t)d * K * S;
    for (uint32_t k = tid; k < SUM_TILE * kp; k += SUM_THREADS) {
        const uint32_t ls = k % SUM_TILE, m = k / SUM_TILE;
        s_val[ls][m] = m < K && s0 + ls < S ? day[(size_t)m * S + s0 + ls] : INT32_MAX;
    }
    __syncthreads();
    {   // the sums: 32 lanes a series
        const uint32_t ls = tid >> 5, hl = tid & 31u;
        unsigned long long acc = 0ull;
        for (uint32_t m = hl; m < K; m += 32u) acc += (unsigned long long)(long long)s_val[ls][m];
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) acc += wave_xor(acc, off);
        if (hl == 0u && s0 + ls < S) report[REINA_SUMMARY_SUM(K, a.days, S, a.Q, a.T) + (size_t)d * S + s0 + ls] = (int64_t)acc;
    }
    // the thresholds of this tile's series: one wave a threshold
    for (uint32_t t = wave; t < a.T; t += SUM_THREADS / 64u) {
        const uint32_t st = head->thr_series[t];
        if (st / SUM_TILE != tile) continue;
        const int32_t value = head->thr_value[t];
        uint32_t c = 0u;
        for (uint32_t m = lane; m < K; m += 64u) c += s_val[st % SUM_TILE][m] > value ? 1u : 0u;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += wave_xor(c, off);
        if (lane == 0u) report[REINA_SUMMARY_EXCEED(K, a.days, S, a.Q, a.T) + (size_t)t * a.days + d] = (int64_t)c;
    }
    // bitonic network over kp values, SUM_TILE series side by side: pair q of a series is (i, i | j)
    const uint32_t pairs = SUM_TILE * (kp >> 1), half_mask = (kp >> 1) - 1u;
    for (uint32_t k = 2u; k <= kp; k <<= 1)
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            __syncthreads();
            for (uint32_t p = tid; p < pairs; p += SUM_THREADS) {
                const uint32_t ls = p >> (log2_kp - 1u), q = p & half_mask;
                const uint32_t i = ((q & ~(j - 1u)) << 1) | (q & (j - 1u)), l = i | j;
                const int32_t x = s_val[ls][i], y = s_val[ls][l];
                if ((x > y) == ((i & k) == 0u)) {
                    s_val[ls][i] = y;
                    s_val[ls][l] = x;
                }
            }
        }
    __syncthreads();
    for (uint32_t k = tid; k < SUM_TILE * a.Q; k += SUM_THREADS) {
        const uint32_t ls = k / a.Q, q = k % a.Q;
        if (s0 + ls < S)
            report[REINA_SUMMARY_ORDER(K, a.days, S, a.Q, a.T) + ((size_t)d * S + s0 + ls) * a.Q + q] = (int64_t)s_val[ls][head->ranks[q]];
    }
}

// ---------------------------------------------------------------------------------------------
// host side

// page-locked blocks the head is written to before k_summary_head copies it: one ring for the process (a summary has no engine)
static std::mutex g_sum_stage_mu;
static StageRing g_sum_stages;
static const size_t SUM_MAX_STAGES = 8;

static int summary_stage(const void *head, size_t bytes, void *dst, hipStream_t s) {
    std::lock_guard<std::mutex> lock(g_sum_stage_mu);
    void *block = nullptr, *dsrc = nullptr;
    if (int rc = g_sum_stages.acquire(REINA_SUMMARY_HEAD_BYTES(REINA_SUMMARY_MAX_MEMBERS), SUM_MAX_STAGES, &block, &dsrc)) return rc;
    std::memcpy(block, head, bytes);
    const uint32_t n = (uint32_t)(bytes / 8u);
    hipLaunchKernelGGL(k_summary_head, dim3((n + SUM_THREADS - 1u) / SUM_THREADS), dim3(SUM_THREADS), 0, s, (uint64_t *)dst, (const uint64_t *)dsrc, n);
    HIP_CHECK(hipGetLastError());
    return g_sum_stages.release_behind(s);
}

extern "C" {

int reina_summary_version(void) { return REINA_SUMMARY_VERSION; }

int reina_summary(const int32_t *const *history_bases, uint32_t K, uint32_t days, uint32_t nr_ages, const uint8_t *age_group, uint32_t n_groups,
                  const uint32_t *ranks, uint32_t n_ranks, const reina_summary_threshold_t *thresholds, uint32_t n_thresholds, void *dev_scratch,
                  int64_t *dev_report, void *stream) {
    if (K < 1u || K > REINA_SUMMARY_MAX_MEMBERS) return refuse("reina_summary: K must be in [1, REINA_SUMMARY_MAX_MEMBERS]");
    if (days < 1u || days > REINA_MAX_DAYS) return refuse("reina_summary: days must be in [1, REINA_MAX_DAYS]");
    if (nr_ages < 1u || nr_ages > REINA_MAX_AGES) return refuse("reina_summary: nr_ages must be in [1, REINA_MAX_AGES]");
    if (n_groups < 1u || n_groups > REINA_SUMMARY_MAX_GROUPS) return refuse("reina_summary: n_groups must be in [1, REINA_SUMMARY_MAX_GROUPS]");
    if (n_ranks > REINA_SUMMARY_MAX_RANKS) return refuse("reina_summary: n_ranks must be at most REINA_SUMMARY_MAX_RANKS");
    if (n_thresholds > REINA_SUMMARY_MAX_THRESHOLDS) return refuse("reina_summary: n_thresholds must be at most REINA_SUMMARY_MAX_THRESHOLDS");
    if (!history_bases || !age_group || (n_ranks && !ranks) || (n_thresholds && !thresholds) || !dev_scratch || !dev_report)
        return refuse("reina_summary: null pointer");
    if (((uintptr_t)dev_scratch & 15u) || ((uintptr_t)dev_report & 15u)) return refuse("reina_summary: scratch and report must be 16-byte aligned device buffers");
    const uint32_t S = REINA_SUMMARY_SERIES(n_groups);
    std::vector<uint64_t> block(REINA_SUMMARY_HEAD_BYTES(K) / 8u, 0ull);
    SumHead *h = reinterpret_cast<SumHead *>(block.data());
    for (uint32_t k = 0; k < nr_ages; k++) {
        if (age_group[k] >= n_groups) return refuse("reina_summary: an age's group is not below n_groups");
        h->group[k] = age_group[k];
    }
    for (uint32_t q = 0; q < n_ranks; q++) {
        if (ranks[q] >= K) return refuse("reina_summary: a rank is not below K");
        h->ranks[q] = ranks[q];
    }
    for (uint32_t t = 0; t < n_thresholds; t++) {
        if (thresholds[t].series >= S) return refuse("reina_summary: a threshold's series is not below S");
        h->thr_series[t] = thresholds[t].series;
        h->thr_value[t] = thresholds[t].value;
    }
    for (uint32_t m = 0; m < K; m++) {
        if (!history_bases[m]) return refuse("reina_summary: null pointer (a member's rows)");
        if ((uintptr_t)history_bases[m] & 15u) return refuse("reina_summary: every member's rows must be 16-byte aligned");
        block[sizeof(SumHead) / 8u + m] = (uint64_t)(uintptr_t)history_bases[m];
    }
    // (every pass is one workgroup a unit of work: the grids follow the shapes, not the chip's compute units)
    hipStream_t s = (hipStream_t)stream;
    if (int rc = summary_stage(block.data(), block.size() * 8u, dev_scratch, s)) return rc;
    const SumHead *d_head = reinterpret_cast<const SumHead *>(dev_scratch);
    int32_t *d_series = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(dev_scratch) + REINA_SUMMARY_HEAD_BYTES(K));
    const SumArgs a = {K, days, nr_ages, n_groups, S, n_ranks, n_thresholds};
    const size_t rows = (size_t)K * days;
    hipLaunchKernelGGL(k_summary_series, dim3((uint32_t)((rows + 3u) / 4u)), dim3(SUM_THREADS), 0, s, d_head, d_series, a);
    HIP_CHECK(hipGetLastError());
    const size_t items = (size_t)K * S + (size_t)n_thresholds * K;
    hipLaunchKernelGGL(k_summary_peak, dim3((uint32_t)((items + 15u) / 16u)), dim3(SUM_THREADS), 0, s, d_head, (const int32_t *)d_series, dev_report, a);
    HIP_CHECK(hipGetLastError());
    uint32_t kp = 2u, log2_kp = 1u;
    while (kp < K) {
        kp <<= 1;
        log2_kp++;
    }
    const dim3 grid((S + SUM_TILE - 1u) / SUM_TILE, days);
    if (kp <= 64u)
        hipLaunchKernelGGL(k_summary_order<64u>, grid, dim3(SUM_THREADS), 0, s, d_head, (const int32_t *)d_series, dev_report, a, kp, log2_kp);
    else if (kp <= 256u)
        hipLaunchKernelGGL(k_summary_order<256u>, grid, dim3(SUM_THREADS), 0, s, d_head, (const int32_t *)d_series, dev_report, a, kp, log2_kp);
    else
        hipLaunchKernelGGL(k_summary_order<1024u>, grid, dim3(SUM_THREADS), 0, s, d_head, (const int32_t *)d_series, dev_report, a, kp, log2_kp);
    HIP_CHECK(hipGetLastError());
    return REINA_OK;
}

}  // extern "C"
