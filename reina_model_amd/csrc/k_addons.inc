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

// +1 in LDS histogram cell b of every lane with b >= 0; the lanes that share the first such lane's cell add once.
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

// ---------------------------------------------------------------------------------------------
// the population by age group, as the reports' kernels take it

struct AgeGroupArgs {
    uint32_t n_agents, nr_ages;
    int32_t age_start[REINA_MAX_AGES + 1];
    uint8_t group[REINA_MAX_AGES];
};

static int age_group_args(const reina_engine_t *e, const uint8_t *age_group, uint32_t n_groups, uint32_t max_groups, const char *what, AgeGroupArgs *a) {
    if (!age_group || n_groups < 1u || n_groups > max_groups) {
        g_last_error = std::string(what) + ": age_group must be a table of groups, 1 <= n_groups <= " + std::to_string(max_groups);
        return REINA_E_INVALID;
    }
    std::memset(a, 0, sizeof(*a));
    a->n_agents = e->cfg.n_agents;
    a->nr_ages = e->cfg.nr_ages;
    std::memcpy(a->age_start, e->cfg.age_start, sizeof(a->age_start));
    for (uint32_t k = 0; k < e->cfg.nr_ages; k++) {
        if (age_group[k] >= n_groups) {
            g_last_error = std::string(what) + ": an age's group is not below n_groups";
            return REINA_E_INVALID;
        }
        a->group[k] = age_group[k];
    }
    return REINA_OK;
}

// ---------------------------------------------------------------------------------------------
// the links of a tile: what an agent's record says of its infection, classified once for the tree report and the dated log

struct Links {               // a thread's two agents of a tile: tile * REPORT_TILE + j * REPORT_THREADS + threadIdx.x
    uint32_t idx[2], w[2];   // the agent and its hot word (0 beyond the population)
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
#pragma unroll
    for (int j = 0; j < 2; j++) {
        k.idx[j] = tile * REPORT_TILE + (uint32_t)j * REPORT_THREADS + threadIdx.x;
        k.w[j] = k.idx[j] < N ? hot[k.idx[j]] : 0u;
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
    g_last_error = "day >= REINA_MAX_DAYS (4096)";
    return REINA_E_INVALID;
}

// attachments hold to bound, unsharded engines: `what` names the attachment, `why_unsharded` is its own reason
static int attachment_check_members(const std::vector<reina_engine_t *> &members, const char *what, const char *why_unsharded) {
    for (auto m : members) {
        if (!m->bound) return REINA_E_NOT_BOUND;
        if (m->cfg.n_shards > 1 || m->exact || m->coll_fn || m->a2a_fn) {
            g_last_error = std::string(what) + ": sharded engines are refused (" + why_unsharded + "), exact attribution included";
            return REINA_E_INVALID;
        }
    }
    return REINA_OK;
}

// an entry point of one engine's attachments was handed a group's, or the other way round
static int attachment_kind(const attachment *a, bool group, const char *what) {
    if (!a) return REINA_E_INVALID;
    if ((a->g != nullptr) != group) {
        g_last_error = std::string(what) + (group ? ": made for one engine -- use the entry point without group_" : ": made for a group -- use the reina_group_ entry point");
        return REINA_E_INVALID;
    }
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
