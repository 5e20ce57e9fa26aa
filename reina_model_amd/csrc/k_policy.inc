// reina_hip.hip part: triggered interventions (include/reina_policy.h; DESIGN.md section 6e).
// Included at the end of reina_hip.hip (it uses the host helpers, the group and k_addons.inc above); not a standalone header.
//
// ONE launch a day, k_policy, queued ahead of the day's opening launch: blockIdx.y = member (the member table read through the
// constant address space), POLICY_WGS workgroups a member.  Every wave sums the signal row of its member's counter block and
// replays the rule from the member's policy state -- the decision is a handful of scalar instructions, cheaper than telling
// the other waves about it; the first wave of the member's first workgroup writes the next state and the day's trace words.
// A member whose level stays and whose bank is not new returns there.  Otherwise the member's workgroups copy the used rows of
// the level's bank entry into the member's own Tables and the table parts of its parameter block, 16 bytes a lane.
//
// The state is double-buffered (a launch reads one copy and writes the other), so the waves that only read it cannot meet the
// one that writes.  The tables are read by the NEXT launch through the scalar / constant path: a kernel boundary lies between,
// as between k_group_tables and the day it precedes.
#include "../../include/reina_policy.h"

#define POLICY_THREADS 256
#define POLICY_WGS 8u

struct PolicyState {
    int32_t level;       // in force on the last day seen
    int32_t in_force;    // days it has governed
    int32_t first_day;   // first day of the unbroken sequence of days seen
    int32_t next_day;    // the day that would continue it (0 before the first: any first day starts a sequence ...)
    int32_t seen;        // ... unless nothing was seen yet
    int32_t pad_[3];
    int32_t ring[REINA_POLICY_RING];   // x_now of day d at [d & 31]
};
static_assert(sizeof(PolicyState) == 160, "forty words");
typedef reina_engine::Stage PolicyEntry;   // a bank entry: what an upload stages -- the parameter block (its table parts are used) and the Tables image
static_assert(sizeof(DevParams) % 16 == 0 && offsetof(PolicyEntry, t) % 16 == 0 && sizeof(PolicyEntry) % 16 == 0, "entries and members' blocks agree in 16-byte alignment");

// words [w0, w1) of a block, source and destination at the same offsets of 16-byte aligned bases: 16 bytes a lane between the
// ragged ends
__device__ __forceinline__ void policy_copy(GAS uint32_t *dst, const GAS uint32_t *src, uint32_t w0, uint32_t w1, uint32_t first, uint32_t stride) {
    const uint32_t a0 = (w0 + 3u) & ~3u, a1 = w1 & ~3u;
    if (a0 >= a1) {
        for (uint32_t k = w0 + first; k < w1; k += stride) dst[k] = src[k];
        return;
    }
    for (uint32_t k = w0 + first; k < a0; k += stride) dst[k] = src[k];
    GAS v4u_ *d4 = reinterpret_cast<GAS v4u_ *>(dst);
    const GAS v4u_ *s4 = reinterpret_cast<const GAS v4u_ *>(src);
    for (uint32_t k = a0 / 4u + first; k < a1 / 4u; k += stride) d4[k] = s4[k];
    for (uint32_t k = a1 + first; k < w1; k += stride) dst[k] = src[k];
}

// (GROUP = false: one engine, its member by value in the kernel arguments like the day's own kernels -- one dependent load less
// ahead of the signal)
template <bool GROUP>
__global__ __launch_bounds__(POLICY_THREADS) void k_policy(const MemberRef *M_, const MemberRef one_, const reina_policy_rule_t rule,
                                                           const PolicyEntry *bank, const PolicyState *st_in, PolicyState *st_out,
                                                           int32_t *trace, uint32_t day, uint32_t new_bank) {
    const uint32_t m = GROUP ? blockIdx.y : 0u, lane = threadIdx.x & 63u;
    MEMBER_OF_LAUNCH;
    const MemberRef &ref = mref_;
    // the signal: 128 words of the counter block, two a lane, summed over the wave
    const GAS int32_t *row = (const GAS int32_t *)ref.B.counters + rule.signal * REINA_MAX_AGES;
    int32_t x_now = row[lane] + row[lane + 64u];
#pragma unroll
    for (int o = 32; o; o >>= 1) x_now += __shfl_xor(x_now, o);
    x_now = __builtin_amdgcn_readfirstlane(x_now);
    // (the state was written by the previous day's launch: a constant to this one)
    const CAS PolicyState *S = (const CAS PolicyState *)(st_in + m);
    const int32_t d = (int32_t)day;
    const int32_t first = (S->seen && S->next_day == d) ? S->first_day : d;
    int32_t x = x_now;
    if (rule.kind == REINA_POLICY_INCREMENT) {
        const int32_t back = d - (int32_t)rule.n_days > first ? d - (int32_t)rule.n_days : first;
        x = x_now - (back == d ? x_now : S->ring[back & (REINA_POLICY_RING - 1)]);
    }
    const int32_t L = (int32_t)rule.n_levels;
    int32_t level = S->level, in_force = S->in_force;
    if (level < 0 || level >= L) level = 0;   // (never: the state is this kernel's own)
    const int32_t before = level;
    if (day >= rule.start_day && (day - rule.start_day) % rule.review_every == 0u) {
        int32_t to = level;
        for (int32_t j = L - 1; j > level; j--)
            if (x >= rule.up[j - 1]) {
                to = j;
                break;
            }
        if (to == level && level > 0 && x < rule.down[level - 1] && in_force >= (int32_t)rule.min_days) to = level - 1;
        if (to != level) {
            level = to;
            in_force = 0;
        }
    }
    if (blockIdx.x == 0u && threadIdx.x < 64u) {
        PolicyState *O = st_out + m;
        if (lane < REINA_POLICY_RING) O->ring[lane] = lane == (day & (REINA_POLICY_RING - 1u)) ? x_now : S->ring[lane];
        if (lane == 32u) O->level = level;
        if (lane == 33u) O->in_force = in_force + 1;
        if (lane == 34u) O->first_day = first;
        if (lane == 35u) O->next_day = d + 1;
        if (lane == 36u) O->seen = 1;
        int32_t *tr = trace + ((size_t)m * REINA_MAX_DAYS + day) * REINA_POLICY_TRACE_WORDS;
        if (lane == 37u) tr[0] = level;
        if (lane == 38u) tr[1] = x;
    }
    if (level == before && !new_bank) return;
    // the switch: the used rows of the level's entry (reina_hip.hip: stage_upload's segments), then the table parts of the parameter block
    const PolicyEntry *E = bank + level;
    const CAS Tables *ET = (const CAS Tables *)&E->t;
    const uint32_t nr = ET->n_rows ? ET->n_rows : 1u, nc = ET->n_crows ? ET->n_crows : 1u;
    const uint32_t stride = gridDim.x * POLICY_THREADS, t0 = blockIdx.x * POLICY_THREADS + threadIdx.x;
    {
        const GAS uint32_t *src = (const GAS uint32_t *)&E->t;
        GAS uint32_t *dst = (GAS uint32_t *)const_cast<Tables *>(ref.T);
        policy_copy(dst, src, offsetof(Tables, thr) / 4u, offsetof(Tables, thr) / 4u + REINA_MAX_ENTRIES * nr, t0, stride);
        policy_copy(dst, src, offsetof(Tables, meta) / 4u, offsetof(Tables, meta) / 4u + REINA_MAX_ENTRIES * nr, t0, stride);
        policy_copy(dst, src, offsetof(Tables, guide) / 4u, offsetof(Tables, guide) / 4u + 64u * nr, t0, stride);
        policy_copy(dst, src, offsetof(Tables, grp) / 4u, offsetof(Tables, grp) / 4u + 8u * nr, t0, stride);
        policy_copy(dst, src, offsetof(Tables, rcount) / 4u, offsetof(Tables, cthr) / 4u, t0, stride);
        policy_copy(dst, src, offsetof(Tables, cthr) / 4u, offsetof(Tables, cthr) / 4u + REINA_COUNT_WORDS * nc, t0, stride);
        policy_copy(dst, src, offsetof(Tables, cguide) / 4u, offsetof(Tables, cguide) / 4u + 64u * nc, t0, stride);
        policy_copy(dst, src, offsetof(Tables, crow_of_age) / 4u, sizeof(Tables) / 4u, t0, stride);
    }
    {
        const GAS uint32_t *src = (const GAS uint32_t *)&E->p;
        GAS uint32_t *dst = (GAS uint32_t *)const_cast<DevParams *>(ref.P);
        policy_copy(dst, src, DP_TAB0_BEGIN / 4u, DP_TAB0_END / 4u, t0, stride);
        policy_copy(dst, src, DP_TAB1_BEGIN / 4u, sizeof(DevParams) / 4u, t0, stride);
    }
}

struct reina_policy : attachment {           // (last_day: the last day run)
    reina_policy_rule_t rule;
    PolicyEntry *d_bank = nullptr;           // [n_levels]
    std::vector<PolicyEntry> h_bank;         // the entries as derived on the host (LDS sizing; the members' mirrors after a run)
    bool uploaded[REINA_POLICY_MAX_LEVELS] = {false};
    bool new_bank = false;                   // a level was uploaded since the last day ran: every member takes its entry
    PolicyState *d_state[2] = {nullptr, nullptr};
    uint32_t parity = 0;                     // which copy of the state the next launch reads
    int32_t *d_trace = nullptr;              // [members][REINA_MAX_DAYS][REINA_POLICY_TRACE_WORDS]
};

static void free_policy(reina_policy *p) {
    if (p->d_bank) (void)hipFree(p->d_bank);
    if (p->d_state[0]) (void)hipFree(p->d_state[0]);
    if (p->d_state[1]) (void)hipFree(p->d_state[1]);
    if (p->d_trace) (void)hipFree(p->d_trace);
    delete p;
}

static int policy_check_rule(const reina_policy_rule_t *r) {
    if (r->n_levels < 2u || r->n_levels > REINA_POLICY_MAX_LEVELS) return refuse("policy: n_levels must be in [2, REINA_POLICY_MAX_LEVELS]");
    if (r->signal >= REINA_C_NR) return refuse("policy: signal is not a per-age counter row (REINA_C_*)");
    if (r->kind != REINA_POLICY_LEVEL && r->kind != REINA_POLICY_INCREMENT) return refuse("policy: kind must be REINA_POLICY_LEVEL or REINA_POLICY_INCREMENT");
    if (r->kind == REINA_POLICY_INCREMENT && (r->n_days < 1u || r->n_days > 28u)) return refuse("policy: an increment is taken over 1..28 days");
    if (r->review_every < 1u) return refuse("policy: review_every must be at least 1");
    if (r->start_day >= REINA_MAX_DAYS) return refuse("policy: start_day >= REINA_MAX_DAYS");
    for (uint32_t j = 0; j + 1u < r->n_levels; j++)
        if ((j > 0 && r->up[j] < r->up[j - 1]) || r->down[j] > r->up[j])
            return refuse("policy: inconsistent thresholds (up[] must be non-decreasing and down[j] <= up[j])");
    return REINA_OK;
}

static int policy_create(const std::vector<reina_engine_t *> &members, reina_group *g, const MemberRef *d_refs,
                         const reina_policy_rule_t *rule, reina_policy_t **out) {
    if (!rule || !out) return REINA_E_INVALID;
    if (int rc = attachment_check_members(members, "policy", "the signal would need the shards' all-reduce")) return rc;
    if (int rc = policy_check_rule(rule)) return rc;
    reina_policy *p = new reina_policy();
    p->e0 = members[0], p->g = g, p->members = members, p->d_refs = d_refs;
    p->rule = *rule;
    const size_t K = members.size(), L = rule->n_levels;
    p->h_bank.resize(L);
    std::memset(static_cast<void *>(p->h_bank.data()), 0, sizeof(PolicyEntry) * L);
    HIP_CHECK_OR(hipMalloc(&p->d_bank, sizeof(PolicyEntry) * L), free_policy(p));
    HIP_CHECK_OR(hipMemset(p->d_bank, 0, sizeof(PolicyEntry) * L), free_policy(p));
    for (int k = 0; k < 2; k++) {
        HIP_CHECK_OR(hipMalloc(&p->d_state[k], sizeof(PolicyState) * K), free_policy(p));
        HIP_CHECK_OR(hipMemset(p->d_state[k], 0, sizeof(PolicyState) * K), free_policy(p));
    }
    const size_t trace_bytes = sizeof(int32_t) * K * REINA_MAX_DAYS * REINA_POLICY_TRACE_WORDS;
    HIP_CHECK_OR(hipMalloc(&p->d_trace, trace_bytes), free_policy(p));
    HIP_CHECK_OR(hipMemset(p->d_trace, 0, trace_bytes), free_policy(p));
    *out = p;
    return REINA_OK;
}

extern "C" {

// ahead of a day's opening launch
static int policy_launch_day(attachment *a, const reina_day_t &dp, hipStream_t s) {
    reina_policy *p = static_cast<reina_policy *>(a);
    if (int rc = attachment_check_day(dp.day)) return rc;
    const uint32_t K = (uint32_t)p->members.size();
    launch_members(k_policy, K > 1, POLICY_WGS, K, POLICY_THREADS, s, p->d_refs, p->e0->h_ref, p->rule, p->d_bank, p->d_state[p->parity],
                   p->d_state[p->parity ^ 1u], p->d_trace, dp.day, p->new_bank ? 1u : 0u);
    p->parity ^= 1u;
    p->new_bank = false;
    p->last_day = dp.day;
    return REINA_OK;
}

// before a run: every level uploaded; k_day's LDS carved for the most rows of any level (the host does not know a member's level)
static int policy_begin_run(reina_policy *p) {
    uint32_t rows = 0, crows = 0;
    for (uint32_t l = 0; l < p->rule.n_levels; l++) {
        if (!p->uploaded[l]) return refuse("policy: bank level " + std::to_string(l) + " was never uploaded");
        if (p->h_bank[l].t.n_rows > rows) rows = p->h_bank[l].t.n_rows;
        if (p->h_bank[l].t.n_crows > crows) crows = p->h_bank[l].t.n_crows;
    }
    p->e0->policy_lds_rows = rows;
    p->e0->policy_lds_crows = crows;
    return REINA_OK;
}
// before a run: every day has its trace words (refused as a whole, before any of its days is queued)
static int policy_check_days(const reina_day_t *days, uint32_t n_days) {
    for (uint32_t k = 0; k < n_days; k++)
        if (days[k].day >= REINA_MAX_DAYS) return refuse("policy: day >= REINA_MAX_DAYS (4096): the trace has no words for it");
    return REINA_OK;
}
static void policy_end_run(reina_policy *p) { p->e0->policy_lds_rows = p->e0->policy_lds_crows = 0; }

int reina_policy_version(void) { return REINA_POLICY_VERSION; }

int reina_policy_create(reina_engine_t *e, const reina_policy_rule_t *rule, reina_policy_t **out) {
    if (!e) return REINA_E_INVALID;
    if (!e->bound) return REINA_E_NOT_BOUND;
    return policy_create(std::vector<reina_engine_t *>(1, e), nullptr, e->d_ref, rule, out);
}

int reina_group_policy_create(reina_group_t *g, const reina_policy_rule_t *rule, reina_policy_t **out) {
    if (!g || g->members.empty()) return REINA_E_INVALID;
    return policy_create(g->members, g, g->d_refs, rule, out);
}

int reina_policy_destroy(reina_policy_t *p) {
    if (!p) return REINA_E_INVALID;
    free_policy(p);
    return REINA_OK;
}

int reina_policy_upload_level(reina_policy_t *p, uint32_t level, const reina_contact_tables_t *t, void *stream) {
    if (!p || !t) return REINA_E_INVALID;
    if (level >= p->rule.n_levels) return refuse("policy: level out of range");
    PolicyEntry &E = p->h_bank[level];
    if (int rc = derive_contact_tables(p->e0, t, E.p, E.t)) return rc;
    if (int rc = stage_upload(p->e0, E.p, E.t, &p->d_bank[level].p, &p->d_bank[level].t, (hipStream_t)stream)) return rc;
    p->uploaded[level] = true;
    p->new_bank = true;
    return REINA_OK;
}

int reina_policy_run_days(reina_policy_t *p, const reina_day_t *days, uint32_t n_days, int32_t *history_base, void *stream) {
    if (!days) return REINA_E_INVALID;
    if (int rc = attachment_kind(p, false, "policy: reina_policy_run_days")) return rc;
    if (int rc = policy_check_days(days, n_days)) return rc;
    if (int rc = policy_begin_run(p)) return rc;
    const int rc = engine_run_days(p->e0, days, n_days, history_base, stream, day_hooks{p, policy_launch_day, nullptr});
    policy_end_run(p);
    return rc;
}

int reina_group_policy_run_days(reina_policy_t *p, const reina_day_t *days, uint32_t n_days, int32_t *const *history_bases, void *stream) {
    if (!days) return REINA_E_INVALID;
    if (int rc = attachment_kind(p, true, "policy: reina_group_policy_run_days")) return rc;
    if (int rc = policy_check_days(days, n_days)) return rc;
    if (int rc = policy_begin_run(p)) return rc;
    const int rc = group_run_days(p->g, days, n_days, history_bases, stream, day_hooks{p, policy_launch_day, nullptr});
    policy_end_run(p);
    return rc;
}

int reina_policy_read_trace(reina_policy_t *p, uint32_t first_day, uint32_t n_days, int32_t *out_host, void *stream) {
    if (!p) return REINA_E_INVALID;
    if (n_days && !out_host) return refuse("policy: read_trace without an output buffer (out_host is null)");
    if ((uint64_t)first_day + n_days > REINA_MAX_DAYS) return refuse("policy: trace range beyond REINA_MAX_DAYS");
    hipStream_t s = (hipStream_t)stream;
    const size_t K = p->members.size(), day_bytes = sizeof(int32_t) * REINA_POLICY_TRACE_WORDS;
    if (n_days)
        HIP_CHECK(hipMemcpy2DAsync(out_host, day_bytes * n_days, p->d_trace + (size_t)first_day * REINA_POLICY_TRACE_WORDS, day_bytes * REINA_MAX_DAYS,
                                   day_bytes * n_days, K, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (n_days && (int64_t)first_day + n_days - 1 == p->last_day) {
        // the members' tables are their final levels' entries of the bank as it stands: the host mirrors follow
        for (size_t m = 0; m < K; m++) {
            const int32_t level = out_host[(m * n_days + (n_days - 1u)) * REINA_POLICY_TRACE_WORDS];
            if (level < 0 || level >= (int32_t)p->rule.n_levels) continue;
            const PolicyEntry &E = p->h_bank[level];
            reina_engine_t *e = p->members[m];
            std::memcpy(reinterpret_cast<char *>(&e->h_params) + DP_TAB0_BEGIN, reinterpret_cast<const char *>(&E.p) + DP_TAB0_BEGIN, DP_TAB0_END - DP_TAB0_BEGIN);
            std::memcpy(reinterpret_cast<char *>(&e->h_params) + DP_TAB1_BEGIN, reinterpret_cast<const char *>(&E.p) + DP_TAB1_BEGIN, sizeof(DevParams) - DP_TAB1_BEGIN);
            std::memcpy(&e->h_tables, &E.t, sizeof(Tables));
        }
    }
    return REINA_OK;
}

}  // extern "C"
