// reina_hip.hip part: what the parts behind the day share -- the tree reports (k_transmission.inc), the triggered interventions
// (k_policy.inc) and the dated log (k_txlog.inc).  Included after the group code and ahead of those parts; not a standalone header.
// (A member's element of a table in constant memory comes from k_common.inc's member_from_constant, generic in the element:
// MEMBER_OF_LAUNCH, used by the day's kernels above, needs it there.)

// ---------------------------------------------------------------------------------------------
// wave helpers: all are called by whole waves

// (a 64-bit value is shuffled as its two halves)
__device__ __forceinline__ unsigned long long wave_xor(unsigned long long x, int off) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)x, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(x >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t wave_xor(uint32_t x, int off) { return (uint32_t)__shfl_xor((int)x, off); }

template <class T>
__device__ __forceinline__ T wave_max(T x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T o = wave_xor(x, off);
        x = o > x ? o : x;
    }
    return x;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t x) { return ~wave_max(~x); }
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += wave_xor(x, off);
    return x;
}

// +1 in an LDS cell that is the same for every lane (a scalar of a report), of every lane with p: one ballot, one popcount and
// one atomic by lane 0 where the count is not zero
__device__ __forceinline__ void wave_tally(uint32_t *cell, bool p) {
    const uint32_t n = (uint32_t)__popcll(__ballot(p));
    if ((threadIdx.x & 63u) == 0u && n) atomicAdd(cell, n);
}

// +1 in LDS histogram cell b of every lane with b >= 0, for cells that differ by lane (one cell for all: wave_tally, which needs
// neither the shuffle nor the second ballot); the lanes that share the first such lane's cell add once.
// (A ballot and a popcount: not wave_add with val = 1, whose butterfly costs twelve shuffles.)
__device__ __forceinline__ void wave_count(uint32_t *hist, int b) {
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

// val into cell `key` of a table in global memory for every lane with key >= 0: the lanes that share the first such lane's
// cell add their sum once.
__device__ __forceinline__ void wave_add(GAS unsigned long long *tab, int key, unsigned long long val) {
    const uint64_t act = __ballot(key >= 0);
    if (!act) return;
    const int lead = __ffsll((unsigned long long)act) - 1;
    const int lk = __shfl(key, lead);
    const bool same = key == lk;
    const unsigned long long s = wave_sum(same ? val : 0ull);
    if (same) {
        if ((int)(threadIdx.x & 63u) == lead && s) atomicAdd(&tab[lk], s);
    } else if (key >= 0 && val) {
        atomicAdd(&tab[key], val);
    }
}

// every report kernel runs workgroups of 256 threads over tiles of 512 agents, two a thread
#define REPORT_THREADS 256
#define REPORT_TILE 512u

// the non-zero cells of a workgroup's LDS table into the 64-bit table of the report (behind a __syncthreads())
template <class T>
__device__ __forceinline__ void flush_lds(const T *lds, uint32_t n, GAS unsigned long long *dst) {
    for (uint32_t k = threadIdx.x; k < n; k += REPORT_THREADS)
        if (lds[k]) atomicAdd(&dst[k], (unsigned long long)lds[k]);
}

// this launch's member's block of an array of `words_a_member` elements a member (log words, course records, report blocks):
// the blockIdx.y-th of a group's, the only one of an engine's
template <bool GROUP, class T>
__device__ __forceinline__ GAS T *member_block(T *p, size_t words_a_member) {
    return (GAS T *)p + (GROUP ? (size_t)blockIdx.y * words_a_member : 0u);
}

// a thread's two agents of tile t, t * REPORT_TILE + j * REPORT_THREADS + threadIdx.x, and their hot words (0 beyond the population)
__device__ __forceinline__ void tile_words(uint32_t t, uint32_t N, const GAS uint32_t *hot, uint32_t (&idx)[2], uint32_t (&w)[2]) {
#pragma unroll
    for (int j = 0; j < 2; j++) {
        idx[j] = t * REPORT_TILE + (uint32_t)j * REPORT_THREADS + threadIdx.x;
        w[j] = idx[j] < N ? hot[idx[j]] : 0u;
    }
}

// A wave's walk over tile t of the ACTIVE bit plane, in the 512-agent tiles of 16 plane words that k_day's sparse stream uses
// (the plane holds whole tiles: REINA_BITS_WORDS).  Lane l looks at agent t * REPORT_TILE + 64 j + l in round j -- bit l & 31 of
// plane word 2 j + (l >> 5), which lane 2 j + (l >> 5) holds -- so the hot words of a dense tile are fetched coalesced.
// false: no bit of the tile is set.  Otherwise w[j] is the hot word of round j's agent where its bit is set, 0 where it is not.
__device__ __forceinline__ bool active_tile(const GAS uint32_t *plane, const GAS uint32_t *hot, uint32_t t, uint32_t N, uint32_t lane, uint32_t (&w)[8]) {
    const uint32_t wd = plane[t * 16u + (lane & 15u)];
    if (!__ballot(wd != 0u)) return false;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t bits = (uint32_t)__shfl((int)wd, 2 * j + (int)(lane >> 5));
        const uint32_t i = t * REPORT_TILE + (uint32_t)j * 64u + lane;
        w[j] = ((bits >> (lane & 31u)) & 1u) && i < N ? hot[i] : 0u;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------
// the population by age group, as the reports' kernels take it

struct AgeGroupArgs {
    uint32_t n_agents, nr_ages;
    int32_t age_start[REINA_MAX_AGES + 1];
    uint8_t group[REINA_MAX_AGES];
};

// ... and as a report kernel keeps it in LDS: declared __shared__, loaded by the whole workgroup ahead of its __syncthreads().
// 644 bytes: age_of never looks at the closing entry of age_start (its `mid` stays at or below the top age), so the top age has
// that word.
struct ReportAges {
    int32_t start[REINA_MAX_AGES];
    int32_t top;
    uint8_t group[REINA_MAX_AGES];
    __device__ __forceinline__ void load(const AgeGroupArgs &p) {
        static_assert(REPORT_THREADS > REINA_MAX_AGES, "one thread an age, and one for the top");
        const uint32_t tid = threadIdx.x;
        if (tid < REINA_MAX_AGES) {
            start[tid] = p.age_start[tid];
            group[tid] = p.group[tid];
        }
        if (tid == REINA_MAX_AGES) top = (int32_t)p.nr_ages - 1;
    }
    __device__ __forceinline__ int age_of(uint32_t agent) const { return ::age_of(start, agent, 0, top); }
    __device__ __forceinline__ int group_of(uint32_t agent) const { return (int)group[age_of(agent)]; }
};
static_assert(sizeof(ReportAges) == (REINA_MAX_AGES + 1) * 4u + REINA_MAX_AGES, "the two tables and not a byte more");

static int age_group_args(const reina_engine_t *e, const uint8_t *age_group, uint32_t n_groups, uint32_t max_groups, const char *what, AgeGroupArgs *a) {
    if (!age_group || n_groups < 1u || n_groups > max_groups)
        return refuse(std::string(what) + ": age_group must be a table of groups, 1 <= n_groups <= " + std::to_string(max_groups));
    std::memset(a, 0, sizeof(*a));
    a->n_agents = e->cfg.n_agents;
    a->nr_ages = e->cfg.nr_ages;
    std::memcpy(a->age_start, e->cfg.age_start, sizeof(a->age_start));
    for (uint32_t k = 0; k < e->cfg.nr_ages; k++) {
        if (age_group[k] >= n_groups) return refuse(std::string(what) + ": an age's group is not below n_groups");
        a->group[k] = age_group[k];
    }
    return REINA_OK;
}

// ---------------------------------------------------------------------------------------------
// the links of a tile: what an agent's record says of its infection, classified once for the tree report and the dated log

struct Links {               // a thread's two agents of a tile
    uint32_t idx[2], w[2];   // the agent and its hot word (tile_words)
    bool inf[2];             // ever infected: nothing below is set of an agent that was not
    int32_t src[2];          // the cold record's infector (-1: none) ...
    uint32_t n[2];           // ... and n_infected
    uint32_t sw[2];          // the infector's hot word (0: out of range, or the agent itself)
    uint32_t lw[2], sl[2];   // LOG: the agent's log word and its infector's
    bool root[2], linked[2], bad[2];   // no infector | an infector that was infected itself | anything else
};

// false: the tile holds no infected agent (`k` then says so of both agents, and nothing was gathered or counted).  Otherwise
// `cnt[at_*]` (LDS) have the wave's infected agents, roots, links and bad links added (at_root < 0: not counted).  The loads
// stay in three rounds -- all hot words, then all cold gathers, then all infector gathers -- so that the gathers of both
// agents are in flight together.
template <bool LOG>
__device__ __forceinline__ bool load_links(Links &k, uint32_t tile, uint32_t N, const GAS uint32_t *hot, const GAS reina_cold_t *cold,
                                           const GAS uint32_t *log, uint32_t *cnt, int at_inf, int at_root, int at_linked, int at_bad) {
    k = Links();
    tile_words(tile, N, hot, k.idx, k.w);
#pragma unroll
    for (int j = 0; j < 2; j++) {
        k.lw[j] = LOG && k.idx[j] < N ? log[k.idx[j]] : 0u;
        k.inf[j] = RH_STATE(k.w[j]) != RS_SUSCEPTIBLE;
        k.src[j] = -1;
    }
    if (!__ballot(k.inf[0] || k.inf[1])) return false;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        if (k.inf[j]) {
            const v2u_ c = *reinterpret_cast<const GAS v2u_ *>(&cold[k.idx[j]].infector);   // infector, n_infected
            k.src[j] = (int32_t)c.x;
            k.n[j] = c.y;
        }
    }
#pragma unroll
    for (int j = 0; j < 2; j++)
        if (k.inf[j] && k.src[j] >= 0 && (uint32_t)k.src[j] < N && (uint32_t)k.src[j] != k.idx[j]) {
            k.sw[j] = hot[k.src[j]];
            if (LOG) k.sl[j] = log[k.src[j]];
        }
    // (not wave_tally: the counts of a thread's two agents are summed first, four LDS atomics a tile where it would take eight)
    uint32_t c[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int j = 0; j < 2; j++) {
        k.root[j] = k.inf[j] && k.src[j] == -1;
        k.linked[j] = k.inf[j] && !k.root[j] && RH_STATE(k.sw[j]) != RS_SUSCEPTIBLE;   // (sw = 0 for an infector out of range or itself)
        k.bad[j] = k.inf[j] && !k.root[j] && !k.linked[j];
        c[0] += (uint32_t)__popcll(__ballot(k.inf[j]));
        c[1] += (uint32_t)__popcll(__ballot(k.root[j]));
        c[2] += (uint32_t)__popcll(__ballot(k.linked[j]));
        c[3] += (uint32_t)__popcll(__ballot(k.bad[j]));
    }
    if ((threadIdx.x & 63u) == 0u) {
        atomicAdd(&cnt[at_inf], c[0]);
        if (at_root >= 0 && c[1]) atomicAdd(&cnt[at_root], c[1]);
        if (c[2]) atomicAdd(&cnt[at_linked], c[2]);
        if (c[3]) atomicAdd(&cnt[at_bad], c[3]);
    }
    return true;
}

// ---------------------------------------------------------------------------------------------
// launches over the members of an engine or a group

// workgroups a member: per_cu a compute unit shared among the K members, at least one and no more than `units` of work
static uint32_t member_grid(uint32_t n_cus, uint32_t K, uint32_t units, uint32_t per_cu) {
    const uint32_t per = per_cu * n_cus / K;
    const uint32_t most = per < 1u ? 1u : per;
    return units < most ? (units ? units : 1u) : most;
}

// KERNEL<GROUP> over grid_x workgroups a member: `group` picks the instantiation that finds its member at blockIdx.y of the
// member table (K members), anything else the one that takes the one member by value.  The rule is the caller's: what was
// made for a group says `group` whatever K is (the dated log: its words and reports are laid out by member), what only
// needs the table for K > 1 says that (the policy: a group of one decides like an engine).  Returns on a failed launch.
#define launch_members(KERNEL, group, grid_x, K, threads, stream, ...)                                          \
    do {                                                                                                        \
        if (group)                                                                                              \
            hipLaunchKernelGGL(KERNEL<true>, dim3(grid_x, K), dim3(threads), 0, stream, __VA_ARGS__);           \
        else                                                                                                    \
            hipLaunchKernelGGL(KERNEL<false>, dim3(grid_x, 1), dim3(threads), 0, stream, __VA_ARGS__);          \
        HIP_CHECK(hipGetLastError());                                                                           \
    } while (0)

// ---------------------------------------------------------------------------------------------
// attachments: what is made for an engine or a group, lives beside it and is queued around its days

struct attachment {
    reina_engine_t *e0 = nullptr;            // the engine, or the group's representative
    reina_group *g = nullptr;                // made for a group
    std::vector<reina_engine_t *> members;
    const MemberRef *d_refs = nullptr;       // the engine's / the group's member table (device)
    int64_t last_day = -1;                   // the last day it was queued for
};

// an attachment keeps something by day: its launches refuse the days beyond
static int attachment_check_day(uint32_t day) {
    if (day < REINA_MAX_DAYS) return REINA_OK;
    return refuse("day >= REINA_MAX_DAYS (4096)");
}

// attachments hold to bound, unsharded engines: `what` names the attachment, `why_unsharded` is its own reason
static int attachment_check_members(const std::vector<reina_engine_t *> &members, const char *what, const char *why_unsharded) {
    for (auto m : members) {
        if (!m->bound) return REINA_E_NOT_BOUND;
        if (m->cfg.n_shards > 1 || m->exact || m->coll_fn || m->a2a_fn)
            return refuse(std::string(what) + ": sharded engines are refused (" + why_unsharded + "), exact attribution included");
    }
    return REINA_OK;
}

// an entry point of one engine's attachments was handed a group's, or the other way round
static int attachment_kind(const attachment *a, bool group, const char *what) {
    if (!a) return REINA_E_INVALID;
    if ((a->g != nullptr) != group)
        return refuse(std::string(what) + (group ? ": made for one engine -- use the entry point without group_" : ": made for a group -- use the reina_group_ entry point"));
    return REINA_OK;
}

// one engine's days with an attachment's launches around them: always the three-launch day (reina_step_day), never the
// several-days-in-one-launch form
static int engine_run_days(reina_engine_t *e0, const reina_day_t *days, uint32_t n_days, int32_t *history_base, void *stream, const day_hooks &hooks) {
    for (uint32_t k = 0; k < n_days; k++) {
        reina_day_t d = days[k];
        d.history_row = history_base ? history_base + (size_t)k * REINA_COUNTER_WORDS : nullptr;
        if (int rc = attachment_check_day(d.day)) return rc;
        if (hooks.before)
            if (int rc = hooks.before(hooks.a, d, (hipStream_t)stream)) return rc;
        if (int rc = reina_step_day(e0, &d, stream)) return rc;
        if (hooks.after)
            if (int rc = hooks.after(hooks.a, d, (hipStream_t)stream)) return rc;
    }
    return REINA_OK;
}

// ---------------------------------------------------------------------------------------------
// what the entry points of the attachments share on the host.  A new attachment is expected to refuse through refuse and to
// stage what it uploads through a StageRing (k_common.inc), to take a flat report by day from front to launch through day_report
// and its members' words to and from the host from member_copy; forest_passes and the member table (member_table,
// with_member_table) are for reports that resolve the transmission forest by pointer jumping.  Its kernels are expected to find
// their member's blocks with member_block, to keep the age tables in a ReportAges, to walk the ACTIVE plane with active_tile or
// the tiles with tile_words (load_links where they need the links), to count a scalar with wave_tally -- out_of_range one
// predicate a date -- and a histogram with wave_count, to add to the tables by day with wave_add and to flush with flush_lds.

// a member's n_agents elements of `elem` bytes at member * stride of `base`, to the host or from it; waits for the stream
static int member_copy(const attachment *a, void *base, size_t stride, size_t elem, uint32_t member, void *host, bool to_host, const char *what, hipStream_t s) {
    if (member >= a->members.size()) return refuse(std::string(what) + ": member out of range");
    char *dev = static_cast<char *>(base) + (size_t)member * stride * elem;
    const size_t bytes = elem * a->e0->cfg.n_agents;
    if (to_host)
        HIP_CHECK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s));
    else
        HIP_CHECK(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return REINA_OK;
}

// a flat report by day of a log (the dated log's, the course log's)
struct TxlArgs {
    AgeGroupArgs p;
    uint32_t n_days;
};

// Such a report from front to launch: the age groups, n_days and the buffer checked in that order under the prefix `what`, the
// members' blocks of `words` 64-bit words (the header's REINA_*_REPORT_WORDS(n_days)) cleared, then launch(a, grid, K) with the
// kernel's arguments filled and the grid of the one launch: four workgroups a compute unit over the tiles (each flushes its LDS
// tables once).  The launch is the caller's callable, not a parameter: launch_members has to name KERNEL<true> and
// KERNEL<false>, and a callable also has room for what a report queues between the clearing and its kernel.
// (in two halves for a report that has more to check behind these: day_report_args queues nothing)
static int day_report_args(const attachment *l, const char *what, uint32_t max_groups, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days,
                           const uint64_t *dev_report, TxlArgs *a) {
    if (int rc = age_group_args(l->e0, age_group, n_groups, max_groups, what, &a->p)) return rc;
    a->n_days = n_days;
    if (n_days < 1u || n_days > REINA_MAX_DAYS) return refuse(std::string(what) + ": n_days must be in [1, REINA_MAX_DAYS]");
    if (!dev_report || (reinterpret_cast<uintptr_t>(dev_report) & 15u)) return refuse(std::string(what) + ": the report must be a 16-byte aligned device buffer");
    return REINA_OK;
}
template <class Launch>
static int day_report_queue(const attachment *l, size_t words, const TxlArgs &a, uint64_t *dev_report, hipStream_t s, Launch launch) {
    const uint32_t K = (uint32_t)l->members.size();
    HIP_CHECK(hipMemsetAsync(dev_report, 0, words * 8u * K, s));
    const uint32_t grid = member_grid(l->e0->n_cus, K, (a.p.n_agents + REPORT_TILE - 1u) / REPORT_TILE, 4u);
    return launch(a, grid, K);
}
template <class Launch>
static int day_report(const attachment *l, const char *what, uint32_t max_groups, size_t words, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days,
                      uint64_t *dev_report, hipStream_t s, Launch launch) {
    TxlArgs a;
    if (int rc = day_report_args(l, what, max_groups, age_group, n_groups, n_days, dev_report, &a)) return rc;
    return day_report_queue(l, words, a, dev_report, s, launch);
}

// the passes of a forest report (the tree report's, the lineage report's): links, `rounds` of pointer jumping, a tally, a
// third pass over the same grid as the tally, and one lane a member to finish
#define TX_DAY_ROUNDS 13u          // ceil(log2(REINA_MAX_DAYS + 1 + 1)): the most rounds the day word can ask for
static_assert((1u << (TX_DAY_ROUNDS - 1u)) < REINA_MAX_DAYS + 2u && (1u << TX_DAY_ROUNDS) >= REINA_MAX_DAYS + 2u, "day rounds");
struct ForestPasses {
    uint32_t g_links, g_tally, g_jump, rounds;
};
static ForestPasses forest_passes(uint32_t N, uint32_t K, uint32_t n_cus, uint32_t host_rounds) {
    const uint32_t tiles = (N + REPORT_TILE - 1u) / REPORT_TILE, waves = (N + REPORT_THREADS - 1u) / REPORT_THREADS;
    ForestPasses f;
    // (four workgroups a compute unit in the passes that flush LDS tables)
    f.g_links = member_grid(n_cus, K, tiles, 4u);
    f.g_tally = member_grid(n_cus, K, waves, 4u);
    f.g_jump = waves < 32768u ? (waves ? waves : 1u) : 32768u;
    f.rounds = host_rounds != 0xFFFFFFFFu ? host_rounds : TX_DAY_ROUNDS;   // (from the day word: the rounds beyond a member's count return at once)
    return f;
}

// a member of a forest report: its state, its scratch and its block of the report
struct TxMember {
    const uint32_t *hot;
    const reina_cold_t *cold;
    const int32_t *counters;
    uint64_t *pairs;     // [2][n_agents] (parent | distance << 32)
    uint32_t *size;      // [n_agents] agents in the tree of each root
    uint64_t *report;    // [the report's words]
};

static int tx_engine_ok(const reina_engine_t *e) {
    if (!e) return REINA_E_INVALID;
    if (!e->bound) return REINA_E_NOT_BOUND;
    if (e->cfg.n_shards > 1 || e->exact) return refuse("transmission reports are taken of unsharded engines only");
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

// A group report's member table on the host: every member checked (`what` names the entry point in the messages), member k
// with its scratch and block k of `words` words of the report.  Apart from with_member_table: the tree report checks its
// members before its arguments, the lineage report behind them.
static int member_table(const std::vector<reina_engine_t *> &members, void *const *dev_scratch, uint64_t *dev_report, size_t words, const char *what,
                        std::vector<TxMember> *h) {
    h->resize(members.size());
    for (size_t k = 0; k < members.size(); k++) {
        if (int rc = tx_engine_ok(members[k])) return rc;
        if (!tx_aligned(dev_scratch[k])) return refuse(std::string(what) + ": every member's scratch must be a 16-byte aligned device buffer");
        (*h)[k] = tx_member_of(members[k], dev_scratch[k], dev_report + k * words);
    }
    return REINA_OK;
}

// ... and on the device around the passes: launch(d_m) with the table uploaded; the table and its host copy live until the
// passes have run, so the stream is waited for before the table goes
template <class Launch>
static int with_member_table(const std::vector<TxMember> &h, const char *what, hipStream_t s, Launch launch) {
    TxMember *d_m = nullptr;
    HIP_CHECK(hipMalloc(&d_m, sizeof(TxMember) * h.size()));
    int rc = REINA_OK;
    if (hipMemcpyAsync(d_m, h.data(), sizeof(TxMember) * h.size(), hipMemcpyHostToDevice, s) != hipSuccess)
        rc = refuse(std::string(what) + ": member table upload failed", REINA_E_HIP);
    if (rc == REINA_OK) rc = launch(d_m);
    const hipError_t se = hipStreamSynchronize(s);
    (void)hipFree(d_m);
    if (rc == REINA_OK && se != hipSuccess) rc = refuse(std::string(what) + ": " + hipGetErrorString(se), REINA_E_HIP);
    return rc;
}
