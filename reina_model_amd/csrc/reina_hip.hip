// reina_hip.hip -- MI355X (gfx950 / CDNA4) agent engine behind the C ABI of include/reina_hip.h.
//
// One simulated day (the reference's Context.iterate, cythonsim/main.pyx:2011-2018) is a short
// sequence of kernels over SoA agent state resident in HBM:
//
//   k_open          first launch: roles by arrival ticket -- history snapshot, new beds, imports (claim rounds),
//                   daily zeroing | weekly imports | test queue -> detect, contact tracing (main.pyx:1652-1699,495-558)
//   k_vaccinate     days with a programme: oldest-first cursor scan                            (:560-583)
//   k_day           every agent's 4-byte hot word streamed once: R bookkeeping, state machine (:1968-1992,395-438),
//                   and in the same waves the contact sampling of the infectious agents found: LDS-staged
//                   contact tables, target gather, Bernoulli transmission, atomicMin winner claim
//                   (:1290-1304,1525-1573,908-934)
//   k_hosp_install  workgroup 0: bed / ICU admission in priority order (:321-367,617-651) beside workgroups 1..:
//                   winners become INCUBATION (severity + incubation draw, :209-235), symptom onsets, bookkeeping
//
// The path is HBM-bound integer / RNG work: no MFMA.  Wave64 ballots compact rare events,
// per-lane Philox keys every decision by (agent, day, purpose) so results do not depend on launch
// geometry.  Integer results are bit-identical to oracle/reina_par.c by construction (same
// primitives header, FP contraction off).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

// gfx950 (MI355X / CDNA4) only: k_day's hand-written ISA (global_load_dwordx4 into hand-reserved VGPRs, global_load_lds_dword through
// M0, manual vmcnt accounting) and reina_prims.h's v_bitop3 Philox are written for this target and checked on it alone
// (tests/test_abi.py disassembles the code object); another --offload-arch must not build silently
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libreina_hip is written for gfx950 (MI355X) only: build with --offload-arch=gfx950"
#endif

#include <climits>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/reina_hip.h"
#include "reina_prims.h"
#include "reina_sample.h"
#include "reina_contacts.h"

#define CNT_IDX(c, age) ((c) * REINA_MAX_AGES + (age))
#define SC_IDX(s) (REINA_C_NR * REINA_MAX_AGES + (s))

enum { EV_HOSPITALIZE = 0, EV_TO_ICU = 1, EV_RELEASE_WARD = 2, EV_RELEASE_ICU = 3 };

// The kernels, in the order of a day (each part is included exactly once, here):
#include "k_common.inc"
#include "k_open.inc"
#include "k_testing.inc"
#include "k_scan.inc"
#include "k_hospital.inc"
#include "k_initial.inc"
#include "k_contacts.inc"
#include "k_remote.inc"
#include "k_install.inc"
#include "k_small.inc"
#define SMALL_MAX_DAYS 64u   // days of one k_small_days launch (the records' device buffer)

// ---------------------------------------------------------------------------------------------
// host side

// HIP-event timing of the day's kernels (reina_profile_enable): start/stop timestamps ride on the kernel's
// own dispatch packet (hipExtLaunchKernelGGL), no extra stream commands.  On a profiled day ONE kind of kernel
// is timed (the kinds take turns), so the cost of timestamped dispatches is spread thinly over the run.
// (the events only carry timestamps, read after a synchronisation: a DEVICE-scope release where they are recorded -- the default, a
// system-scope release, writes the caches back behind every timestamped kernel)
#define REINA_TIMING_EVENT_FLAGS (hipEventReleaseToDevice)
static bool take_event_pair(reina_engine *e, size_t *a, size_t *b) {
    while (e->ev_used + 2 > e->ev_pool.size()) {
        if (e->ev_pool.size() >= reina_engine::MAX_EVENTS) return false;   // pool exhausted: this launch goes untimed
        hipEvent_t ev = nullptr;
        if (hipEventCreateWithFlags(&ev, REINA_TIMING_EVENT_FLAGS) != hipSuccess || !ev) return false;
        e->ev_pool.push_back(ev);
    }
    *a = e->ev_used++;
    *b = e->ev_used++;
    return true;
}

// which kind of kernel carries timestamps on `day` (-1: none)
static int profiled_kind(const reina_engine *e, uint32_t day) {
    if (!e->profile) return -1;
    const uint32_t stride = e->profile_stride;
    if (stride <= 1) return REINA_PK_NR;        // every kernel, every day
    const uint32_t ph = day % stride;
    // the four kernels of every day at evenly spaced phases; the occasional ones ride with k_open's phase
    if (ph == 0) return REINA_PK_DAY;
    if (e->profile_day_only) return -1;   // (enable < 0: only the dominant kernel carries timestamps -- a third of the instrument's cost)
    if (ph == stride / 4) return REINA_PK_OPEN;
    if (ph == stride / 2) return REINA_PK_HOSPITAL;
    if (ph == stride / 2 + stride / 4) return REINA_PK_INSTALL;
    return -1;
}
static bool kind_timed(int today, int kind) {
    if (today < 0) return false;
    if (today == REINA_PK_NR || today == kind) return true;
    // the one launch of a small population's day (k_small_day) is timed on k_day's days and on the event walk's: twice per stride
    if (kind == REINA_PK_SMALL_DAY) return today == REINA_PK_DAY || today == REINA_PK_HOSPITAL;
    // kernels that do not run every day are timed on k_open's days
    if (today == REINA_PK_HOSPITAL && (kind == REINA_PK_REMOTE || kind == REINA_PK_HOSP_SORT || kind == REINA_PK_HOSP_WALK || kind == REINA_PK_XCHG || kind == REINA_PK_COLLECTIVE)) return true;
    return today == REINA_PK_OPEN && (kind == REINA_PK_TRACE1 || kind == REINA_PK_VACCINATE);
}

#define LAUNCH_TIMED(e, today, kind, kernel, grid, block, lds, stream, ...)                                              \
    do {                                                                                                                 \
        size_t ev_a_, ev_b_;                                                                                             \
        if (kind_timed(today, kind) && take_event_pair(e, &ev_a_, &ev_b_)) {                                             \
            hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, (e)->ev_pool[ev_a_], (e)->ev_pool[ev_b_], 0, __VA_ARGS__); \
            (e)->kpairs[kind].emplace_back(ev_a_, ev_b_);                                                                \
        } else {                                                                                                         \
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                           \
        }                                                                                                                \
    } while (0)

// THE list of the day kernels' instantiations <GROUP, EXACT>: a single engine, a group's members (found in `refs`), a shard under
// exact attribution (k_common.inc: DAY_KERNEL) -- k_day's each in the dense and the sparse form of the stream.  `f` is called
// once per entry; what launches, sizes or checks the day kernels is written over these two.
template <bool G, bool X, bool SP = false> struct DayForm { static constexpr bool group = G, exact = X, sparse = SP; };
template <class F> static void each_day_form(F &&f) { f(DayForm<false, false>()); f(DayForm<true, false>()); f(DayForm<false, true>()); }
template <class F> static void each_k_day_form(F &&f) {
    each_day_form([&](auto m) { using M = decltype(m); f(DayForm<M::group, M::exact, false>()); f(DayForm<M::group, M::exact, true>()); });
}
// a kernel of the day: the instantiation of the launch's form -- K members, or the single engine's MemberRef by value
#define LAUNCH_DAY(e, today, kind, kernel, grid, block, lds, stream, ...)                                                \
    each_day_form([&](auto m_) {                                                                                         \
        using M_ = decltype(m_);                                                                                         \
        if (M_::group == (K > 1) && M_::exact == (K == 1 && (e)->exact))                                                 \
            LAUNCH_TIMED(e, today, kind, (kernel<M_::group, M_::exact>), grid, block, lds, stream, refs, (e)->h_ref, __VA_ARGS__); \
    })

static void resolve_profile(reina_engine *e) {
    for (int k = 0; k < REINA_PK_NR; k++) {
        size_t idx = 0;
        for (auto &p : e->kpairs[k]) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, e->ev_pool[p.first], e->ev_pool[p.second]) == hipSuccess) {
                e->k_ms[k] += ms;
                // (a k_small_days launch runs a stretch of days: the kind counts DAYS, so that ms / count is a day's time like the others')
                e->k_launches[k] += k == REINA_PK_SMALL_DAY && idx < e->small_pair_days.size() ? e->small_pair_days[idx] : 1u;
            }
            idx++;
        }
        if (k == REINA_PK_SMALL_DAY) e->small_pair_days.clear();
        e->kpairs[k].clear();
    }
    e->ev_used = 0;
}

// frees what reina_create / reina_group_create had acquired when a later step fails
static void free_engine(reina_engine *e) {
    for (auto ev : e->ev_pool) (void)hipEventDestroy(ev);
    e->stage.free();
    e->days_stage.free();
    if (e->d_params) (void)hipFree(e->d_params);
    if (e->d_tables) (void)hipFree(e->d_tables);
    if (e->d_ref) (void)hipFree(e->d_ref);
    if (e->d_bar) (void)hipFree(e->d_bar);
    if (e->d_days) (void)hipFree(e->d_days);
    if (e->d_snap) (void)hipFree(e->d_snap);
    if (e->counted_live) g_live_engines--;
    delete e;
}

// One row of contact-count thresholds + its guide table (reina_contacts.h: 105 erfc + log in double, 4 us a row, 80 us for the
// 20 distinct rows of a table -- host time that a short run cannot hide behind the GPU: the 20-day window of the round
// driver's bench contains one table change, and it cost 5 us per step).  A row depends on one float only, and the same
// values come back all the time -- a table change that closes schools leaves the other ages' rows as they were; every seed
// of an ensemble, every scenario run of a serving process rebuilds the same tables on the same dates -- so rows are kept,
// process-wide, keyed by the float's bits (at most 4096 rows, 1.5 MB; beyond that rows are computed and not kept).
struct CountRow { uint32_t thr[REINA_COUNT_WORDS]; uint8_t guide[256]; };
static void count_row_for(float nr_contacts, uint32_t *thr, uint8_t *guide) {
    static std::mutex mu;
    static std::unordered_map<uint32_t, CountRow> rows;
    uint32_t key;
    std::memcpy(&key, &nr_contacts, 4);
    // (REINA_COUNT_ROW_CACHE=0: every row computed afresh -- what a table change costs a process that has not seen the
    // scenario's mobility values before; bench.py reports that figure beside the warm one)
    const char *cache_env = std::getenv("REINA_COUNT_ROW_CACHE");
    const bool use_cache = !(cache_env && cache_env[0] == '0');
    if (use_cache) {
        std::lock_guard<std::mutex> g(mu);
        auto it = rows.find(key);
        if (it != rows.end()) {
            std::memcpy(thr, it->second.thr, sizeof(it->second.thr));
            std::memcpy(guide, it->second.guide, 256);
            return;
        }
    }
    CountRow row;
    rc_count_thresholds(nr_contacts, row.thr);
    int idx = 0;
    for (uint32_t b = 0; b < 256; b++) {
        while (idx < REINA_COUNT_FULL && row.thr[idx] <= (b << 24)) idx++;   // thresholds are non-decreasing
        row.guide[b] = (uint8_t)idx;
    }
    std::memcpy(thr, row.thr, sizeof(row.thr));
    std::memcpy(guide, row.guide, 256);
    if (!use_cache) return;
    std::lock_guard<std::mutex> g(mu);
    if (rows.size() < 4096) rows.emplace(key, row);
}

// the environment's switches (read in reina_create): a flag, or a number that counts only within [lo, hi]
static void env_flag(const char *name, bool *v) {
    if (const char *w = std::getenv(name)) *v = std::atoi(w) != 0;
}
static void env_uint(const char *name, int lo, int hi, uint32_t *v) {
    const char *w = std::getenv(name);
    if (w && std::atoi(w) >= lo && std::atoi(w) <= hi) *v = (uint32_t)std::atoi(w);
}
// reina_create's way out of a configuration it refuses
static int refuse_create(reina_engine *e, const std::string &text, int code = REINA_E_INVALID) {
    free_engine(e);
    return refuse(text, code);
}

extern "C" {

int reina_abi_version(void) { return 7; }

int reina_build_contact_tables(const double *base, const int32_t *row_page, const int32_t *row_place, uint32_t n_rows,
                               const double *mobility, uint32_t n_mobility, const int32_t *rows_mat,
                               const int32_t *sorted_mat, uint32_t n_ages, uint32_t n_entries, double *totals_out,
                               double *cum_out, float *nrc_out, uint32_t *thr_out, uint32_t thr_stride) {
    const int rc = reina_build_contact_tables_impl(base, row_page, row_place, n_rows, mobility, n_mobility, rows_mat, sorted_mat,
                                                   n_ages, n_entries, totals_out, cum_out, nrc_out, thr_out, thr_stride);
    return rc == 0 ? REINA_OK : REINA_E_INVALID;
}

// test hook: one primitive of reina_prims.h evaluated on the device, one lane per record
__global__ __launch_bounds__(256) void k_test_prims(int what, const uint32_t *in, uint32_t n, uint32_t n_in, uint32_t n_out, uint32_t *out) {
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        uint32_t a[8] = {0, 0, 0, 0, 0, 0, 0, 0}, o[4] = {0, 0, 0, 0};
        for (uint32_t j = 0; j < n_in; j++) a[j] = in[(size_t)k * n_in + j];
        rp_test_prim(what, a, o);
        for (uint32_t j = 0; j < n_out; j++) out[(size_t)k * n_out + j] = o[j];
    }
}

int reina_test_prims(int what, const uint32_t *in_host, uint32_t n, uint32_t *out_host) {
    uint32_t n_in = 0, n_out = 0;
    rp_test_prim_words(what, &n_in, &n_out);
    if (!n_in || !in_host || !out_host) return REINA_E_INVALID;
    if (n == 0) return REINA_OK;
    uint32_t *d_in = nullptr, *d_out = nullptr;
    HIP_CHECK(hipMalloc(&d_in, (size_t)n * n_in * 4));
    HIP_CHECK_OR(hipMalloc(&d_out, (size_t)n * n_out * 4), (void)hipFree(d_in));
#define TP_CLEAN { (void)hipFree(d_in); (void)hipFree(d_out); }
    HIP_CHECK_OR(hipMemcpy(d_in, in_host, (size_t)n * n_in * 4, hipMemcpyHostToDevice), TP_CLEAN);
    hipLaunchKernelGGL(k_test_prims, dim3(grid_for(n, 256, 4096)), dim3(256), 0, nullptr, what, d_in, n, n_in, n_out, d_out);
    HIP_CHECK_OR(hipGetLastError(), TP_CLEAN);
    HIP_CHECK_OR(hipMemcpy(out_host, d_out, (size_t)n * n_out * 4, hipMemcpyDeviceToHost), TP_CLEAN);
    TP_CLEAN;
#undef TP_CLEAN
    return REINA_OK;
}

int reina_sample(const reina_disease_t *disease, uint64_t seed, int what, int age, int severity,
                 float nr_contacts_of_age, int n, int32_t *out) {
    return reina_sample_impl(disease, seed, what, age, severity, nr_contacts_of_age, n, out);
}
const char *reina_last_error(void) { return g_last_error.c_str(); }

int reina_create(const reina_config_t *cfg, const reina_disease_t *disease, reina_engine_t **out) {
    if (!cfg || !disease || !out) return REINA_E_INVALID;
    if (cfg->nr_ages == 0 || cfg->nr_ages > REINA_MAX_AGES || cfg->nr_variants == 0 ||
        cfg->nr_variants > REINA_MAX_VARIANTS)
        return refuse("nr_ages / nr_variants out of range");
    int ndev = 0;
    HIP_CHECK(hipGetDeviceCount(&ndev));
    if (ndev == 0) return refuse("no HIP device", REINA_E_HIP);
    for (uint32_t a = 0; a < cfg->nr_ages; a++)
        if (cfg->age_start[a] < 0 || cfg->age_start[a] > cfg->age_start[a + 1] || (uint32_t)cfg->age_start[a + 1] > cfg->n_agents)
            return refuse("age_start must be non-decreasing and end at n_agents");
    reina_engine *e = new reina_engine();
    e->cfg = *cfg;
    {   // compute units of the current device: grids of one-workgroup-per-CU kernels are sized to it
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 1)
            e->n_cus = (uint32_t)cus;
        env_flag("REINA_VACC_ONE_WG", &e->vacc_one_wg);   // (the single-workgroup vaccination pass at every size: the tests compare)
        env_flag("REINA_NO_PLACE_GROUPS", &e->no_place_groups);
        env_uint("REINA_LDS_ROWS_CAP", 1, INT_MAX, &e->lds_rows_cap);
        env_uint("REINA_WALK_DIV", 16, 1024, &e->walk_div);
        env_uint("REINA_IMPORT_WGS", 1, 16, &e->import_wgs);
        // k_day streams the ACTIVE bit plane instead of the hot words when the population is large enough for that form to pay
        // (reina_launch.h: plan_day).  REINA_DAY_MODE = dense | sparse forces one form whatever the size (the tests run every scenario in
        // both), alternate switches between them day by day; REINA_DAY_FLAGS are k_day's measurement switches
        if (const char *w = std::getenv("REINA_DAY_MODE")) {
            if (!std::strcmp(w, "dense")) e->day_mode = 1;
            else if (!std::strcmp(w, "sparse")) e->day_mode = 2;
            else if (!std::strcmp(w, "alternate")) e->day_mode = 3;
        }
        if (const char *w = std::getenv("REINA_DAY_FLAGS")) e->day_flags |= (uint32_t)std::atoi(w);
        if (const char *w = std::getenv("REINA_EXPORT")) e->export_by_copies = !std::strcmp(w, "memcpy");
        env_flag("REINA_OPEN_TICKETS", &e->open_tickets);   // (the tests' handle on the ticket path of a single engine)
        env_flag("REINA_IMPORTS_IN_OPEN", &e->imports_in_open);   // (the round-3 placement, for comparison)
        // stretches of days of a small unsharded population as ONE launch (k_small.inc): REINA_FUSED_DAY=1 switches it on (off by
        // default: measured slower than the three launches a day; the tests run scenario families both ways), REINA_FUSED_WGS its
        // workgroups (measurement handle; 8..64)
        env_flag("REINA_FUSED_DAY", &e->fused_day);
        env_uint("REINA_FUSED_WGS", 8, 64, &e->small_wgs);
    }
    std::memset(&e->h_params, 0, sizeof(DevParams));
    std::memset(&e->h_tables, 0, sizeof(Tables));
    e->h_params.dis = *disease;
    std::memcpy(e->h_params.age_start, cfg->age_start, sizeof(cfg->age_start));
    e->h_params.n_agents = cfg->n_agents;
    e->h_params.nr_ages = cfg->nr_ages;
    e->h_params.nr_variants = cfg->nr_variants;
    e->cfg.n_shards = cfg->n_shards ? cfg->n_shards : 1;
    if (e->cfg.n_shards > REINA_MAX_SHARDS || e->cfg.shard_rank >= e->cfg.n_shards)
        return refuse_create(e, "n_shards / shard_rank out of range");
#ifdef DIAG_ANY   // (a diagnostic build, reina_diag.h: its stamps and rows go to buffers.mirror, a sharded engine's mirror tables)
    if (e->cfg.n_shards > 1 || cfg->exact_attribution) {
        char sw[160];
        diag_switches(sw, sizeof sw);
        return refuse_create(e, std::string("this library was built with") + sw + ": a diagnostic build runs unsharded engines only "
                                "(buffers.mirror is its scratch, and a sharded engine keeps the mirror tables there)");
    }
#endif
    const uint64_t shard_seed = rp_shard_seed(cfg->seed, e->cfg.shard_rank);
    e->h_params.k0 = (uint32_t)shard_seed;
    e->h_params.k1 = (uint32_t)(shard_seed >> 32);
    for (uint32_t v = 0; v < REINA_MAX_VARIANTS; v++) {
        uint32_t m = 0;
        for (int k = 0; k < REINA_IOT_LEN; k++)
            if (disease->infectiousness_over_time[v][k] != 0.0f) m |= 1u << k;
        e->h_params.iot_mask[v] = m;
    }
    e->h_params.n_shards = e->cfg.n_shards;
    e->h_params.shard_rank = e->cfg.shard_rank;
    e->h_params.mirror_slots = cfg->mirror_slots ? cfg->mirror_slots : 64;
    if (e->h_params.mirror_slots & (e->h_params.mirror_slots - 1))
        return refuse_create(e, "mirror_slots must be a power of two");
    for (uint32_t v = 0; v < cfg->nr_variants; v++) {
        float m = 0.0f;
        for (uint32_t a = 0; a < cfg->nr_ages; a++)
            if (disease->p_susceptibility[v][a] > m) m = disease->p_susceptibility[v][a];
        e->h_params.psus_max[v] = m;
    }
    // exact cross-shard attribution (include/reina_hip.h): global ids in the link fields, records exchanged between the shards
    e->exact = cfg->exact_attribution != 0 && e->cfg.n_shards > 1;
    e->h_params.gid_mask = 0xFFFFFFFFu;
    if (e->exact) {
        if (!cfg->shard_age_start || cfg->xchg_cap == 0 || cfg->pool_cap == 0 || cfg->n_agents > RP_GID_INDEX_MASK)
            return refuse_create(e, "exact attribution needs shard_age_start, xchg_cap > 0, pool_cap > 0 and fewer than 2^27 agents per shard");
        e->h_params.exact = 1u;
        e->h_params.gid_base = e->cfg.shard_rank << RP_GID_SHIFT;
        e->h_params.gid_mask = RP_GID_INDEX_MASK;
        e->h_params.xchg_cap = cfg->xchg_cap;
        e->h_params.pool_cap = cfg->pool_cap;
        std::memcpy(e->h_params.shard_age_start, cfg->shard_age_start, sizeof(int32_t) * (size_t)e->cfg.n_shards * (REINA_MAX_AGES + 1));
        for (uint32_t sh = 0; sh < e->cfg.n_shards; sh++) {
            const uint64_t ss = rp_shard_seed(cfg->seed, sh);
            e->h_params.shard_k0[sh] = (uint32_t)ss;
            e->h_params.shard_k1[sh] = (uint32_t)(ss >> 32);
        }
    }
    e->cfg.shard_age_start = nullptr;   // (the caller's array is not kept)
    e->h_params.max_work_items = cfg->max_work_items;
    e->h_params.max_candidates = cfg->max_candidates;
    {   // the space above the per-wave regions: half (at most 2^20 records) for records that overflow a wave's
        // region, the rest for the cross-shard candidates of k_remote
        const uint32_t extra = cfg->max_candidates > cfg->max_work_items ? cfg->max_candidates - cfg->max_work_items : 0u;
        uint32_t ovf = extra / 2;
        if (ovf > (1u << 20)) ovf = 1u << 20;
        e->h_params.cand_ovf_cap = ovf;
        e->h_params.cand_ovf_base = cfg->max_candidates - ovf;
    }
    e->h_params.max_queue = cfg->max_queue;
    e->h_params.max_hosp_events = cfg->max_hosp_events > REINA_MAX_HOSP_EVENTS ? cfg->max_hosp_events : REINA_MAX_HOSP_EVENTS;
    e->h_params.hosp_ranges = cfg->hosp_ranges ? cfg->hosp_ranges : REINA_HOSP_RANGES(cfg->n_agents);
    e->h_params.xchg_stride = (uint32_t)REINA_XCHG_SEG_WORDS(e->h_params.xchg_cap, e->h_params.hosp_ranges);   // (exact attribution: a segment = count + records + trailer)
    if (e->h_params.hosp_ranges < 16 || e->h_params.hosp_ranges > REINA_HOSP_MAX_RANGES || (e->h_params.hosp_ranges & (e->h_params.hosp_ranges - 1)))
        return refuse_create(e, "hosp_ranges must be a power of two in [16, REINA_HOSP_MAX_RANGES]");
    e->h_params.hosp_range_bits = 0;
    while ((1u << e->h_params.hosp_range_bits) < e->h_params.hosp_ranges) e->h_params.hosp_range_bits++;
    e->h_params.hosp_bucket_cap = REINA_HOSP_BUCKET_CAP_R(e->h_params.hosp_ranges, cfg->max_hosp_events);
    // (a sharded population always takes the bucket-per-wave walk: its shards exchange per-bucket maps)
    e->h_params.hosp_parallel = (cfg->n_agents > REINA_HOSP_SMALL_AGENTS || e->cfg.n_shards > 1) ? 1u : 0u;
    e->exchange_words = (uint32_t)REINA_EXCHANGE_WORDS(e->cfg.n_shards, e->h_params.hosp_ranges);
    if (e->h_params.hosp_parallel && e->h_params.hosp_bucket_cap > REINA_HOSP_MAX_BUCKET_KEYS)
        return refuse_create(e, "max_hosp_events too large for this population: a bucket of the event walk holds at most 4096 keys "
                      "(pass at most REINA_HOSP_MAX_EVENTS_FOR(n_agents), include/reina_hip.h)");
    HIP_CHECK_OR(hipMalloc(&e->d_params, sizeof(DevParams)), free_engine(e));
    HIP_CHECK_OR(hipMalloc(&e->d_tables, sizeof(Tables)), free_engine(e));
    HIP_CHECK_OR(hipMalloc(&e->d_ref, sizeof(MemberRef)), free_engine(e));
    HIP_CHECK_OR(hipMemcpy(e->d_params, &e->h_params, sizeof(DevParams), hipMemcpyHostToDevice), free_engine(e));
    HIP_CHECK_OR(hipMemcpy(e->d_tables, &e->h_tables, sizeof(Tables), hipMemcpyHostToDevice), free_engine(e));
    // (every instantiation of every day kernel that takes dynamic LDS -- single engine, group member, shard under exact attribution --,
    // sized for the larger of its launch shapes)
    const size_t walk_lds = (size_t)HOSP_P_THREADS * HOSP_P_E * 8, small_lds = (size_t)REINA_MAX_HOSP_EVENTS * 8;
    const int day_lds = (int)day_shared_bytes(REINA_LDS_ROWS, REINA_LDS_CROWS, REINA_MAX_SHARDS), inst_lds = (int)(walk_lds > small_lds ? walk_lds : small_lds);
    hipError_t lds_err = hipSuccess;
    auto set_lds = [&](const void *kernel, int bytes) {
        if (lds_err == hipSuccess) lds_err = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    };
    // k_day addresses v104..v127 by hand (k_contacts.inc): the code object must allocate all 128 registers to every instantiation.
    // tests/test_abi.py checks that in the disassembly of the build it runs on; this is the check a box without the tests makes
    // (round-5 verdict: a compiler that stopped honouring the clobber list would hand the kernel fewer registers than it names)
    hipFuncAttributes bad;
    bad.numRegs = 128, bad.localSizeBytes = 0;
    each_k_day_form([&](auto m) {
        using M = decltype(m);
        const void *kernel = reinterpret_cast<const void *>(k_day<M::group, M::exact, M::sparse>);
        set_lds(kernel, day_lds);
        hipFuncAttributes fa;
        if (lds_err == hipSuccess) lds_err = hipFuncGetAttributes(&fa, kernel);
        if (lds_err == hipSuccess && (fa.numRegs != 128 || fa.localSizeBytes != 0)) bad = fa;
    });
    each_day_form([&](auto m) {
        using M = decltype(m);
        set_lds(reinterpret_cast<const void *>(k_hosp_presort<M::group, M::exact>), (int)walk_lds);
        set_lds(reinterpret_cast<const void *>(k_hosp_install<M::group, M::exact>), inst_lds);
    });
    HIP_CHECK_OR(lds_err, free_engine(e));
    if (bad.numRegs != 128 || bad.localSizeBytes != 0)
        return refuse_create(e, "k_day was built with " + std::to_string(bad.numRegs) + " VGPRs / " + std::to_string(bad.localSizeBytes) +
                                    " bytes of scratch: it names v104..v127 by hand and needs 128 / 0 (rebuild with the ROCm release the sources were written for)",
                             REINA_E_HIP);
    {
        // the fused day of a small population: its LDS block (the stream's image or the hospital role's keys + maps, whichever is
        // larger) beside the static LDS of the three phases' functions must fit one compute unit; its barrier counter
        hipFuncAttributes fa;
        HIP_CHECK_OR(hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_small_days)), free_engine(e));
        e->small_static_lds = fa.sharedSizeBytes;
        const size_t most = 160u * 1024u > fa.sharedSizeBytes ? 160u * 1024u - fa.sharedSizeBytes : 0u;
        HIP_CHECK_OR(hipFuncSetAttribute(reinterpret_cast<const void *>(k_small_days), hipFuncAttributeMaxDynamicSharedMemorySize, (int)most), free_engine(e));
        HIP_CHECK_OR(hipMalloc(&e->d_bar, 256), free_engine(e));
        HIP_CHECK_OR(hipMemset(e->d_bar, 0, 256), free_engine(e));
        HIP_CHECK_OR(hipMalloc(&e->d_days, sizeof(SmallDayRec) * SMALL_MAX_DAYS), free_engine(e));
    }
    e->counted_live = true;
    g_live_engines++;
    *out = e;
    return REINA_OK;
}

int reina_destroy(reina_engine_t *e) {
    if (!e) return REINA_E_INVALID;
    free_engine(e);   // teardown: nothing useful can be done about a failing free
    return REINA_OK;
}

int reina_bind_buffers(reina_engine_t *e, const reina_buffers_t *b) {
    if (!e || !b) return REINA_E_INVALID;
    const void *const *p = reinterpret_cast<const void *const *>(b);
    for (size_t k = 0; k < sizeof(reina_buffers_t) / sizeof(void *); k++)
        if (!p[k]) return refuse("null buffer pointer");
    e->buf = *b;
    e->bound = true;
    MemberRef r;
    r.P = e->d_params;
    r.T = e->d_tables;
    r.B = e->buf;
    r.history_base = nullptr;

    HIP_CHECK(hipMemcpy(e->d_ref, &r, sizeof(MemberRef), hipMemcpyHostToDevice));
    e->h_ref = r;
    return REINA_OK;
}

int reina_init_state(reina_engine_t *e, int32_t beds, int32_t icu, void *stream) {
    if (!e || !e->bound) return REINA_E_NOT_BOUND;
    hipStream_t s = (hipStream_t)stream;
    e->init_beds = beds;
    hipLaunchKernelGGL(k_init, dim3(grid_for(e->cfg.n_agents, 256, 4096), 1), dim3(256), 0, s, e->d_ref, beds, icu);
    HIP_CHECK(hipGetLastError());
    return REINA_OK;
}

int reina_set_initial_state(reina_engine_t *e, const reina_initial_state_t *ic, void *stream) {
    if (!e || !ic) return REINA_E_INVALID;
    if (!e->bound) return REINA_E_NOT_BOUND;
    // slot j of the walk over [0, were_incubating) is bound for ICU iff it lies behind the incubating / recovered / ill / dead
    // slots: a walk that stops short of them (fewer recovered than incubating people, main.pyx:1456-1463) constructs
    const uint64_t first_icu_slot = (uint64_t)ic->incubating + ic->recovered_without_illness + ic->ill + ic->dead;
    if (e->cfg.n_shards <= 1 && ic->in_icu > 0 && (uint64_t)ic->were_incubating > first_icu_slot && e->init_beds == 0) {
        // (the reference raises AssertionError out of Context.__init__: an agent bound for ICU is refused a bed and
        // Population.transfer_to_icu asserts state == HOSPITALIZED, main.pyx:1495 -> :350 -> :1603; a shard cannot tell --
        // its own share of the beds may be 0 while the population has some -- and leaves the check to its caller)
        return refuse("initial population condition: people in ICU but a hospital without beds (the reference refuses it)");
    }
    hipLaunchKernelGGL(k_initial_state, dim3(1, 1), dim3(PRO_THREADS), 0, (hipStream_t)stream, e->d_ref, *ic);
    HIP_CHECK(hipGetLastError());
    return REINA_OK;
}

// What an upload derives from the caller's tables: the table-dependent parts of the parameter block `hp` and the Tables image
// `ht` (distinct rows, guides, place groups, count rows, age blocks, uniform_meta).  reina_upload_contact_tables derives into
// the engine's own mirrors, a policy's bank (k_policy.inc) into its entries'.
static int derive_contact_tables(const reina_engine_t *e, const reina_contact_tables_t *t, DevParams &hp, Tables &ht) {
    const uint32_t A = e->cfg.nr_ages;
    if (t->n_ranges > REINA_MAX_RANGES) return refuse("more than REINA_MAX_RANGES contact ranges");
    for (uint32_t a = 0; a < A; a++)
        if (t->count[a] < 0 || t->count[a] > REINA_MAX_ENTRIES) return refuse("contact entries per age must be in [0, REINA_MAX_ENTRIES]");
    for (uint32_t a = 0; a < A; a++)
        if (t->count[a] == 0 && t->nr_contacts_by_age[a] > 0.0f) {   // (k_day would read entry 0 of an empty row)
            return refuse("age " + std::to_string(a) + " has contacts (nr_contacts_by_age > 0) but no contact entries (count == 0)");
        }
    if (e->cfg.n_shards > 1 && t->n_ranges >= REINA_MAX_RANGES)
        return refuse("a sharded engine takes at most REINA_MAX_RANGES - 1 contact ranges (the last range's pressure words carry free capacity)");
    std::memcpy(hp.nrc, t->nr_contacts_by_age, sizeof(float) * A);
    std::memcpy(hp.tcount, t->count, sizeof(int32_t) * A);
    std::memcpy(hp.mask_p, t->mask_p, sizeof(float) * A * 8);
    hp.n_ranges = t->n_ranges;
    std::memcpy(hp.range_min, t->range_min, sizeof(t->range_min));
    std::memcpy(hp.range_max, t->range_max, sizeof(t->range_max));
    {   // distinct contact rows (entry count, thresholds, meta words): ages of one class of the matrix share a row
        Tables &T = ht;
        uint32_t n_rows = 0;
        T.grouped = 1;
        for (uint32_t a = 0; a < A; a++) {
            const uint32_t *thr_a = t->threshold + (size_t)a * REINA_MAX_ENTRIES, *meta_a = t->meta + (size_t)a * REINA_MAX_ENTRIES;
            const size_t used = sizeof(uint32_t) * (size_t)t->count[a];
            uint32_t r = 0;
            for (; r < n_rows; r++)
                if (T.rcount[r] == t->count[a] && std::memcmp(T.thr[r], thr_a, used) == 0 && std::memcmp(T.meta[r], meta_a, used) == 0) break;
            if (r == n_rows) {
                std::memcpy(T.thr[r], thr_a, sizeof(uint32_t) * REINA_MAX_ENTRIES);
                std::memcpy(T.meta[r], meta_a, sizeof(uint32_t) * REINA_MAX_ENTRIES);
                T.rcount[r] = t->count[a];
                const int cnt = t->count[a];
                int idx = 0;
                for (uint32_t b = 0; b < 256; b++) {
                    const uint32_t floor_ = b << 24;
                    while (idx < cnt - 1 && T.thr[r][idx] <= floor_) idx++;   // thresholds are non-decreasing
                    T.guide[r][b] = (uint8_t)(cnt > 0 ? idx : 0);
                }
                // place groups (k_common.inc: Tables::grp)
                uint32_t *G = T.grp[r];
                for (int q = 0; q < 5; q++) G[q] = 0xFFFFFFFFu;
                G[5] = G[6] = G[7] = 0;
                uint32_t groups = 0, last_place = 0;
                for (int en = 0; en < cnt; en++) {
                    const uint32_t place = T.meta[r][en] & 0xFFu;
                    if (en == 0 || place != last_place) {
                        if (en > 0 && groups <= 5) G[groups - 1] = T.thr[r][en - 1];
                        if (groups < 6) G[5] |= (place * 5u) << (5u * groups);
                        groups++;
                        last_place = place;
                    }
                    if (place >= REINA_NR_PLACES) groups = 99;   // (cannot be packed; never with the places of the model)
                }
                for (uint32_t q = groups; q < 6 && groups > 0; q++) G[5] |= (last_place * 5u) << (5u * q);
                G[6] = groups;
                if (groups > 6) T.grouped = 0;
                n_rows++;
            }
            T.row_of_age[a] = (uint8_t)r;
        }
        T.n_rows = n_rows;
        if (e->no_place_groups) T.grouped = 0;
        // contact-count thresholds: one row per distinct nr_contacts_by_age value
        uint32_t n_crows = 0;
        float crow_value[REINA_MAX_AGES];
        for (uint32_t a = 0; a < A; a++) {
            uint32_t r = 0;
            for (; r < n_crows; r++)
                if (std::memcmp(&crow_value[r], &t->nr_contacts_by_age[a], sizeof(float)) == 0) break;
            if (r == n_crows) {
                crow_value[r] = t->nr_contacts_by_age[a];
                count_row_for(crow_value[r], T.cthr[r], T.cguide[r]);
                n_crows++;
            }
            T.crow_of_age[a] = (uint8_t)r;
        }
        T.n_crows = n_crows;
        // coarse index -> age map (the age of a sampled target: one table read + 0-1 steps instead of a search)
        uint32_t shift = 0;
        while (((uint64_t)e->cfg.n_agents >> shift) >= REINA_AGE_BLOCKS) shift++;
        T.age_shift = shift;
        uint32_t a = 0;
        for (uint32_t b = 0; b < REINA_AGE_BLOCKS; b++) {
            const uint64_t i = (uint64_t)b << shift;
            while (a + 1 < A && (uint64_t)e->cfg.age_start[a + 1] <= i) a++;
            T.age_block[b] = (uint8_t)a;
        }
    }
    ht.uniform_meta = 1;
    for (uint32_t r = 1; r < ht.n_rows && ht.uniform_meta; r++)
        if (ht.rcount[r] != ht.rcount[0] ||
            std::memcmp(ht.meta[r], ht.meta[0], sizeof(uint32_t) * (size_t)ht.rcount[0]) != 0)
            ht.uniform_meta = 0;
    return REINA_OK;
}

// the pinned-staging, kernel-reads-host route of an upload: `hp` whole and the used rows of `ht` into d_params / d_tables
static int stage_upload(reina_engine_t *e, const DevParams &hp, const Tables &ht, DevParams *d_params, Tables *d_tables, hipStream_t s) {
    void *block = nullptr, *dsrc = nullptr;
    if (int rc = e->stage.acquire(sizeof(reina_engine::Stage), reina_engine::MAX_STAGES, &block, &dsrc)) return rc;
    reina_engine::Stage *st = static_cast<reina_engine::Stage *>(block);
    std::memcpy(&st->p, &hp, sizeof(DevParams));
    UploadSegs segs;
    {
        const Tables &T = ht;
        const uint32_t nr = T.n_rows ? T.n_rows : 1u, nc = T.n_crows ? T.n_crows : 1u;
        const size_t seg[8][2] = {
            {offsetof(Tables, thr), sizeof(T.thr[0]) * nr},
            {offsetof(Tables, meta), sizeof(T.meta[0]) * nr},
            {offsetof(Tables, guide), sizeof(T.guide[0]) * nr},
            {offsetof(Tables, grp), sizeof(T.grp[0]) * nr},
            {offsetof(Tables, rcount), offsetof(Tables, cthr) - offsetof(Tables, rcount)},   // rcount, row_of_age, n_rows, uniform_meta, grouped
            {offsetof(Tables, cthr), sizeof(T.cthr[0]) * nc},
            {offsetof(Tables, cguide), sizeof(T.cguide[0]) * nc},
            {offsetof(Tables, crow_of_age), sizeof(Tables) - offsetof(Tables, crow_of_age)},   // crow_of_age, n_crows, age_shift, age_block
        };
        segs.n = 8;
        for (int q = 0; q < 8; q++) {
            std::memcpy(reinterpret_cast<char *>(&st->t) + seg[q][0], reinterpret_cast<const char *>(&T) + seg[q][0], seg[q][1]);
            segs.off[q] = (uint32_t)(seg[q][0] / 4);
            segs.words[q] = (uint32_t)(seg[q][1] / 4);
        }
    }
    // The transfer is a KERNEL that reads the pinned host slot directly (zero-copy): an ordinary
    // dispatch in the day stream.  hipMemcpyAsync of the 98 KB table was measured to block the host
    // for 7-8 ms once per run when >1000 dispatches were queued ahead of it (ROCm 7.2).
    static_assert(sizeof(DevParams) % 4 == 0 && sizeof(Tables) % 4 == 0 && offsetof(reina_engine::Stage, t) % 4 == 0 &&
                  offsetof(Tables, meta) % 4 == 0 && offsetof(Tables, guide) % 4 == 0 && offsetof(Tables, grp) % 4 == 0 && offsetof(Tables, rcount) % 4 == 0 &&
                  offsetof(Tables, cthr) % 4 == 0 && offsetof(Tables, cguide) % 4 == 0 && offsetof(Tables, crow_of_age) % 4 == 0, "word copies");
    const uint32_t *src_w = reinterpret_cast<const uint32_t *>(dsrc);
    hipLaunchKernelGGL(k_upload, dim3(64), dim3(256), 0, s, reinterpret_cast<uint32_t *>(d_params), src_w,
                       (uint32_t)(sizeof(DevParams) / 4), reinterpret_cast<uint32_t *>(d_tables),
                       src_w + offsetof(reina_engine::Stage, t) / 4, segs);
    return e->stage.release_behind(s);
}

int reina_upload_contact_tables(reina_engine_t *e, const reina_contact_tables_t *t, void *stream) {
    if (!e || !t) return REINA_E_INVALID;
    if (int rc = derive_contact_tables(e, t, e->h_params, e->h_tables)) return rc;
    return stage_upload(e, e->h_params, e->h_tables, e->d_params, e->d_tables, (hipStream_t)stream);
}

// One day's launches for K engine instances at once (K = 1: a single engine; K > 1: a group of identically configured
// engines, one launch per phase for all of them, member = blockIdx.y), `e` the representative engine.  What is launched, and
// how large, is the day's PLAN (reina_launch.h: plan_day, a pure function): planned once a day by reina_step_day and
// group_run_days, on every call by the stateless entry points; the launchers below only launch.
// The day comes in the PHASES of include/reina_hip.h (reina_step_phase): between them a sharded population exchanges.
static LaunchShape launch_shape(const reina_engine_t *e) {
    return LaunchShape{e->cfg.n_agents, e->n_cus, e->cfg.n_shards, e->exact, e->h_params.hosp_ranges, e->h_params.hosp_parallel,
                       e->h_params.cand_ovf_cap, e->cfg.max_work_items, e->cfg.xchg_cap, e->import_wgs, e->walk_div, e->vacc_one_wg,
                       e->open_tickets, e->imports_in_open, (uint32_t)e->day_mode, e->lds_rows_cap, e->small_wgs};
}
// THE step that notes that a population has ever tested (k_open's test-queue roles run from then on): the caller's, before it plans
static void note_testing(reina_engine_t *e, const reina_day_t &dp) {
    if (dp.testing_mode != RT_NO_TESTING) e->testing_ever = true;
}
static int plan_engine_day(const reina_engine_t *e, uint32_t K, const reina_day_t &dp, DayPlan *plan) {
    uint32_t rows = K > 1 ? e->group_lds_rows : e->h_tables.n_rows, crows = K > 1 ? e->group_lds_crows : e->h_tables.n_crows;   // (a member stages min(its own rows, lds_rows))
    if (e->policy_lds_rows) rows = e->policy_lds_rows;   // (a policy run: the most rows of any level of its bank, k_policy.inc)
    if (e->policy_lds_crows) crows = e->policy_lds_crows;
    switch (plan_day(launch_shape(e), K, e->testing_ever, rows, crows, dp, plan)) {
    case PLAN_E_DAY: return refuse("day >= REINA_MAX_DAYS (4096): the winner-selection keys carry the day in 12 bits");
    case PLAN_E_COUNTS: return refuse("n_import_batches / n_vaccinations out of range");
    }
    return REINA_OK;
}

// REINA_PH_OPEN: the day's opening -- roles (0 opens the day, 1 weekly imports, 2.. the test queue) by arrival ticket
static void launch_day_open(reina_engine_t *e, const MemberRef *refs, uint32_t K, const reina_day_t &dp, const DayPlan &p, uint32_t hist_slot, hipStream_t s) {
    const int today = profiled_kind(e, dp.day);
    LAUNCH_DAY(e, today, REINA_PK_OPEN, k_open, dim3(p.open_grid, K), dim3(PRO_THREADS), 0, s, dp, hist_slot, p.weekly_own, (int)p.open_mode, (int)p.open_tickets);
    if (p.trace1_in_open) LAUNCH_DAY(e, today, REINA_PK_TRACE1, k_test_trace1, dim3(p.trace1_grid, K), dim3(256), 0, s, dp);
}
// REINA_PH_TRACE (exact attribution, contact-tracing days): the level-0 requests of the other shards, then level 1
static void launch_day_trace(reina_engine_t *e, const MemberRef *refs, uint32_t K, const reina_day_t &dp, const DayPlan &p, hipStream_t s) {
    if (!p.xtrace) return;
    const int today = profiled_kind(e, dp.day);
    LAUNCH_DAY(e, today, REINA_PK_XCHG, k_xtrace, dim3(p.xchg_grid, K), dim3(256), 0, s, dp, 0);
    LAUNCH_DAY(e, today, REINA_PK_TRACE1, k_test_trace1, dim3(p.trace1_grid, K), dim3(256), 0, s, dp);
}
// REINA_PH_MAIN: (the level-1 requests of the other shards,) vaccination -- its pass over the agents comes after the test queue and
// before the stream (HealthcareSystem.iterate, main.pyx:514-558) --, the stream with the contact sampling, and a sharded
// population's event maps for the all-reduce
static void launch_day_main(reina_engine_t *e, const MemberRef *refs, uint32_t K, const reina_day_t &dp, const DayPlan &p, hipStream_t s) {
    const int today = profiled_kind(e, dp.day);
    if (p.xtrace) LAUNCH_DAY(e, today, REINA_PK_XCHG, k_xtrace, dim3(p.xchg_grid, K), dim3(256), 0, s, dp, 1);
    if (p.vacc_grid) {
        // The tag is drawn from ONE process-wide counter (round-5 advisor): the tagged words live in each member's own buffers and
        // are never cleared, so a per-engine counter could come back to a value those buffers already hold -- a member stepped in
        // a group (tag = the representative's count) and later alone or under another representative.  A process-wide value is
        // never reused on any buffers (2^32 - 1 vaccination launches per process before it wraps).
        static std::atomic<uint32_t> vacc_seq_next{0};
        do e->vacc_seq = ++vacc_seq_next; while (e->vacc_seq == 0u);
        LAUNCH_DAY(e, today, REINA_PK_VACCINATE, k_vaccinate, dim3(p.vacc_grid, K), dim3(PRO_THREADS), 0, s, dp, e->vacc_seq, p.vacc);
    }
    const dim3 grid(p.day_blocks + p.stream_imports, K);
    const size_t lds = day_shared_bytes(p.lds_rows, p.lds_crows, e->cfg.n_shards);
    each_k_day_form([&](auto m) {
        using M = decltype(m);
        if (M::group == (K > 1) && M::exact == (K == 1 && e->exact) && M::sparse == (p.sparse != 0u))
            LAUNCH_TIMED(e, today, REINA_PK_DAY, (k_day<M::group, M::exact, M::sparse>), grid, dim3(DAY_THREADS), lds, s, refs, e->h_ref, dp, p.lds_rows,
                         p.lds_crows, e->day_flags, p.stream_imports);
    });
    if (p.presort_grid)   // a sharded population: its event buckets sorted and their maps written to the exchange block BEFORE the all-reduce
        LAUNCH_DAY(e, today, REINA_PK_HOSP_SORT, k_hosp_presort, dim3(p.presort_grid, K), dim3(HOSP_THREADS), (size_t)HOSP_P_THREADS * HOSP_P_E * 8, s, dp);
}
// REINA_PH_FEEDBACK (exact attribution): the sources of the day's cross-shard infections take their infectees
static void launch_day_feedback(reina_engine_t *e, const MemberRef *refs, uint32_t K, const reina_day_t &dp, const DayPlan &p, hipStream_t s) {
    if (!e->exact) return;
    const int today = profiled_kind(e, dp.day);
    LAUNCH_DAY(e, today, REINA_PK_XCHG, k_feedback, dim3(p.xchg_grid, K), dim3(256), 0, s, dp);
}
// REINA_PH_END: (k_remote, which also takes this shard's share of the pooled free beds / ICU units: the walk starts from it,) the installs
static void launch_day_end(reina_engine_t *e, const MemberRef *refs, uint32_t K, const reina_day_t &dp, const DayPlan &p, hipStream_t s) {
    const int today = profiled_kind(e, dp.day);
    if (p.remote_grid) LAUNCH_DAY(e, today, REINA_PK_REMOTE, k_remote, dim3(p.remote_grid, K), dim3(256), 0, s, dp);
    const size_t lds = p.install_walk_lds ? (size_t)HOSP_P_THREADS * HOSP_P_E * 8 : (size_t)REINA_MAX_HOSP_EVENTS * 8;
    LAUNCH_DAY(e, today, REINA_PK_INSTALL, k_hosp_install, dim3(p.install_grid, K), dim3(HOSP_THREADS), lds, s, dp, p.scan_waves, p.scan_tiles,
               (int)p.install_flags, p.n_walk);
}

// A stretch of days of a small unsharded population as ONE launch (k_small.inc).  Every workgroup of it must be resident at once
// (they meet at three barriers a day): at most one per compute unit by their LDS, `small_wgs` of them, and only while the process
// holds so few engines that all of theirs fit the chip together (other engines' launches may run beside this one on streams of
// their own).  A day qualifies when nothing in it needs another launch shape: no vaccination programme, at most one workgroup's
// worth of weekly imports, import helpers and one test-queue role within the launch's workgroups.
static bool small_days_engine_ok(const reina_engine_t *e) {
    if (!e->fused_day || e->cfg.n_shards != 1 || e->exact || e->coll_fn || e->h_params.hosp_parallel != 0u) return false;
    if (e->cfg.n_agents > REINA_HOSP_SMALL_AGENTS) return false;
    if (e->day_mode != 0 || e->open_tickets || e->imports_in_open) return false;      // (the tests' handles on the three-launch forms)
    if ((uint32_t)g_live_engines.load() * e->small_wgs > e->n_cus) return false;
    return SMALL_TAIL_BYTES + e->small_static_lds <= 160u * 1024u;
}
// the record of one day from its plan, or false: the day takes the three launches
static bool small_day_record(reina_engine_t *e, const reina_day_t &dp, SmallDayRec *rec) {
    if (dp.n_vaccinations != 0u) return false;
    DayPlan p;
    note_testing(e, dp);
    if (plan_engine_day(e, 1, dp, &p) != REINA_OK || !plan_fits_small(launch_shape(e), p)) return false;
    std::memset(rec, 0, sizeof(*rec));
    rec->dp = dp;
    rec->weekly_own = p.weekly_own;
    rec->mode = (int32_t)p.open_mode;
    rec->stream_imports = p.stream_imports;
    return true;
}
static int launch_small_days(reina_engine_t *e, const SmallDayRec *recs, uint32_t n, hipStream_t s) {
    // the records travel like the tables: a pinned slot the host fills, a copy kernel in the day stream (reina_upload_contact_tables)
    void *block = nullptr, *dsrc = nullptr;
    if (int rc = e->days_stage.acquire(sizeof(SmallDayRec) * SMALL_MAX_DAYS, reina_engine::MAX_STAGES, &block, &dsrc)) return rc;
    std::memcpy(block, recs, sizeof(SmallDayRec) * n);
    UploadSegs none;
    std::memset(&none, 0, sizeof(none));
    const uint32_t words = (uint32_t)(sizeof(SmallDayRec) * n / 4);
    hipLaunchKernelGGL(k_upload, dim3(words / 256u + 1u < 64u ? words / 256u + 1u : 64u), dim3(256), 0, s, reinterpret_cast<uint32_t *>(e->d_days),
                       reinterpret_cast<const uint32_t *>(dsrc), words, (uint32_t *)nullptr, (const uint32_t *)nullptr, none);
    if (int rc = e->days_stage.release_behind(s)) return rc;
    const uint32_t W = e->small_wgs;
    const LaunchShape sh = launch_shape(e);
    SmallGeom g;
    std::memset(&g, 0, sizeof(g));
    g.n_days = n;
    g.lds_rows = lds_rows_for(sh, e->h_tables.n_rows, REINA_LDS_ROWS);
    g.lds_crows = lds_rows_for(sh, e->h_tables.n_crows, REINA_LDS_CROWS);
    g.day_flags = e->day_flags;
    g.scan_tiles = scan_tiles_for(sh.n_agents);
    g.bar_base = e->bar_epoch;
    g.bar = e->d_bar;
    g.days = e->d_days;
    e->bar_epoch += SMALL_BARRIERS_PER_DAY * n;
    // (timed as a whole on the stretches that begin on one of the two profiled phases; the kind's "launches" count DAYS: its mean is per day)
    const int today = profiled_kind(e, recs[0].dp.day);
    const size_t timed_before = e->kpairs[REINA_PK_SMALL_DAY].size();
    LAUNCH_TIMED(e, today, REINA_PK_SMALL_DAY, k_small_days, dim3(W), dim3(HOSP_THREADS), SMALL_TAIL_BYTES, s, e->h_ref, g);
    if (e->kpairs[REINA_PK_SMALL_DAY].size() > timed_before) e->small_pair_days.push_back(n);
    HIP_CHECK(hipGetLastError());
    return REINA_OK;
}
// days[0 .. n): stretches of qualifying days (at least two: a single day is faster as three launches) as one launch each, the rest day by day
static int run_days_small(reina_engine_t *e, const reina_day_t *days, uint32_t n_days, int32_t *history_base, hipStream_t s) {
    std::vector<SmallDayRec> recs;
    recs.reserve(SMALL_MAX_DAYS);
    auto day_at = [&](uint32_t k) {
        reina_day_t d = days[k];
        if (history_base) d.history_row = history_base + (size_t)k * REINA_COUNTER_WORDS;
        return d;
    };
    uint32_t k = 0;
    while (k < n_days) {
        recs.clear();
        uint32_t m = 0;
        while (k + m < n_days && m < SMALL_MAX_DAYS) {
            SmallDayRec r;
            if (!small_day_record(e, day_at(k + m), &r)) break;
            recs.push_back(r);
            m++;
        }
        if (m >= 2u) {
            if (int rc = launch_small_days(e, recs.data(), m, s)) return rc;
            k += m;
            continue;
        }
        // (one qualifying day between two that do not, or none: the launches)
        const uint32_t take = m ? m : 1u;
        for (uint32_t q = 0; q < take; q++) {
            const reina_day_t d = day_at(k + q);
            if (int rc = reina_step_day(e, &d, s)) return rc;
        }
        k += take;
    }
    return REINA_OK;
}

// one phase of a planned day; > 0: the collectives that must follow it
static int step_phase_planned(reina_engine_t *e, const reina_day_t &day, const DayPlan &p, int phase, hipStream_t s) {
    int need = 0;
    switch (phase) {
    case REINA_PH_OPEN: launch_day_open(e, e->d_ref, 1, day, p, 0, s), need = p.xtrace ? REINA_X_ALLTOALL : 0; break;
    case REINA_PH_TRACE: launch_day_trace(e, e->d_ref, 1, day, p, s), need = p.xtrace ? REINA_X_ALLTOALL : 0; break;
    case REINA_PH_MAIN:
        // (a single shard with a collective set exchanges too: the one-GPU box exercises the call)
        // exact attribution (round 6, ABI 7): what the all-reduce carries -- the shards' capacity words and event maps -- rides in the
        // trailers of the contact records' segments: ONE collective here, not two
        launch_day_main(e, e->d_ref, 1, day, p, s);
        need = e->exact ? REINA_X_ALLTOALL : (e->cfg.n_shards > 1 || e->coll_fn) ? REINA_X_ALLREDUCE : 0;
        break;
    case REINA_PH_END: launch_day_end(e, e->d_ref, 1, day, p, s), need = e->exact ? REINA_X_ALLTOALL : 0; break;
    default: launch_day_feedback(e, e->d_ref, 1, day, p, s);
    }
    HIP_CHECK(hipGetLastError());
    return need;
}
// what every stateless entry point of a single engine begins with: the arguments, then the day's plan
static int begin_step(reina_engine_t *e, const reina_day_t *day, DayPlan *p) {
    if (!e || !day) return REINA_E_INVALID;
    if (!e->bound) return REINA_E_NOT_BOUND;
    note_testing(e, *day);
    return plan_engine_day(e, 1, *day, p);
}

int reina_step_phase(reina_engine_t *e, const reina_day_t *day, int phase, void *stream) {
    DayPlan p;
    if (e && day && e->bound && (phase < 0 || phase >= REINA_PH_NR)) return refuse("phase out of range");
    if (int rc = begin_step(e, day, &p)) return rc;
    return step_phase_planned(e, *day, p, phase, (hipStream_t)stream);
}

// the two halves of a day around its one all-reduce (a population without exact attribution)
static const char *const EXACT_HALVES = "exact attribution: a day has more than one exchange -- step it by reina_step_phase (or reina_step_day with reina_set_alltoall)";
int reina_step_day_begin(reina_engine_t *e, const reina_day_t *day, void *stream) {
    DayPlan p;
    if (e && day && e->bound && e->exact) return refuse(EXACT_HALVES);
    if (int rc = begin_step(e, day, &p)) return rc;
    for (int ph = REINA_PH_OPEN; ph <= REINA_PH_MAIN; ph++) {
        const int need = step_phase_planned(e, *day, p, ph, (hipStream_t)stream);
        if (need < 0) return need;
    }
    return REINA_OK;
}

int reina_step_day_end(reina_engine_t *e, const reina_day_t *day, void *stream) {
    DayPlan p;
    if (e && day && e->bound && e->exact) return refuse(EXACT_HALVES);
    if (int rc = begin_step(e, day, &p)) return rc;
    const int need = step_phase_planned(e, *day, p, REINA_PH_END, (hipStream_t)stream);
    return need < 0 ? need : REINA_OK;
}

int reina_set_collective(reina_engine_t *e, reina_allreduce_fn allreduce, void *comm) {
    if (!e) return REINA_E_INVALID;
    e->coll_fn = allreduce;
    e->coll_comm = comm;
    return REINA_OK;
}

int reina_set_alltoall(reina_engine_t *e, reina_alltoall_fn alltoall, void *comm) {
    if (!e) return REINA_E_INVALID;
    e->a2a_fn = alltoall;
    e->a2a_comm = comm;
    return REINA_OK;
}

int reina_step_day(reina_engine_t *e, const reina_day_t *day, void *stream) {
    DayPlan p;
    if (int rc = begin_step(e, day, &p)) return rc;
    for (int ph = 0; ph < REINA_PH_NR; ph++) {
        const int need = step_phase_planned(e, *day, p, ph, (hipStream_t)stream);
        if (need < 0) return need;
        // the exchanges of a sharded population, queued on the day stream itself (on the profiled days of the event-walk kind an
        // event pair is recorded around them: `collective` of reina_profile_read_kernels -- what RCCL costs a day, apart from the kernels)
        size_t ev_a = 0, ev_b = 0;
        const bool timed = need > 0 && (e->coll_fn || e->a2a_fn) && kind_timed(profiled_kind(e, day->day), REINA_PK_COLLECTIVE) &&
                           take_event_pair(e, &ev_a, &ev_b) && hipEventRecord(e->ev_pool[ev_a], (hipStream_t)stream) == hipSuccess;
        if ((need & REINA_X_ALLREDUCE) && e->coll_fn) {
            const int r = e->coll_fn(e->buf.pressure, e->buf.pressure, e->exchange_words, 2 /* ncclInt32 */, 0 /* ncclSum */, e->coll_comm, stream);
            if (r != 0) return refuse("collective failed with code " + std::to_string(r), REINA_E_HIP);
        }
        if (need & REINA_X_ALLTOALL) {
            if (!e->a2a_fn)
                return refuse("exact attribution: no all-to-all set (reina_set_alltoall) -- step the day by reina_step_phase and exchange buffers.xsend / xrecv yourself", REINA_E_NOT_BOUND);
            const int r = e->a2a_fn(e->buf.xsend, e->buf.xrecv, (size_t)e->h_params.xchg_stride, 4 /* ncclInt64 */, e->a2a_comm, stream);
            if (r != 0) return refuse("all-to-all failed with code " + std::to_string(r), REINA_E_HIP);
        }
        if (timed && hipEventRecord(e->ev_pool[ev_b], (hipStream_t)stream) == hipSuccess) e->kpairs[REINA_PK_COLLECTIVE].emplace_back(ev_a, ev_b);
    }
    return REINA_OK;
}

// `rows`: the history rows laid out from history_base (none if null); otherwise every day keeps its own history_row
static int run_days(reina_engine_t *e, const reina_day_t *days, uint32_t n_days, bool rows, int32_t *history_base, void *stream) {
    if (e && days && e->bound && n_days >= 2u && small_days_engine_ok(e)) return run_days_small(e, days, n_days, history_base, (hipStream_t)stream);
    for (uint32_t k = 0; k < n_days; k++) {
        reina_day_t d;
        if (rows) {
            d = days[k];
            d.history_row = history_base ? history_base + (size_t)k * REINA_COUNTER_WORDS : nullptr;
        }
        if (int rc = reina_step_day(e, rows ? &d : &days[k], stream)) return rc;
    }
    return REINA_OK;
}
int reina_run_days(reina_engine_t *e, const reina_day_t *days, uint32_t n_days, void *stream) { return run_days(e, days, n_days, false, nullptr, stream); }
int reina_run_days_hist(reina_engine_t *e, const reina_day_t *days, uint32_t n_days, int32_t *history_base, void *stream) {
    return run_days(e, days, n_days, true, history_base, stream);
}

struct reina_group {
    std::vector<reina_engine_t *> members;
    MemberRef *d_refs = nullptr;
    std::vector<MemberRef> h_refs;
};

int reina_group_create(reina_engine_t **engines, uint32_t n, reina_group_t **out) {
    if (!engines || !out || n == 0 || n > 65535) return REINA_E_INVALID;
    for (uint32_t k = 0; k < n; k++) {
        reina_engine_t *m = engines[k];
        if (!m || !m->bound) return REINA_E_NOT_BOUND;
        if (m->cfg.n_agents != engines[0]->cfg.n_agents || m->cfg.nr_ages != engines[0]->cfg.nr_ages ||
            m->cfg.nr_variants != engines[0]->cfg.nr_variants || m->cfg.n_shards != 1 ||
            std::memcmp(m->cfg.age_start, engines[0]->cfg.age_start, sizeof(m->cfg.age_start)) != 0)
            return refuse("group members must be unsharded engines of the same population");
    }
    reina_group *g = new reina_group();
    g->members.assign(engines, engines + n);
    g->h_refs.resize(n);
    for (uint32_t k = 0; k < n; k++) {
        g->h_refs[k].P = engines[k]->d_params;
        g->h_refs[k].T = engines[k]->d_tables;
        g->h_refs[k].B = engines[k]->buf;
        g->h_refs[k].history_base = nullptr;

    }
    HIP_CHECK_OR(hipMalloc(&g->d_refs, sizeof(MemberRef) * n), delete g);
    HIP_CHECK_OR(hipMemcpy(g->d_refs, g->h_refs.data(), sizeof(MemberRef) * n, hipMemcpyHostToDevice),   // (table broadcasts may precede the first run)
                 { (void)hipFree(g->d_refs); delete g; });
    *out = g;
    return REINA_OK;
}

int reina_group_destroy(reina_group_t *g) {
    if (!g) return REINA_E_INVALID;
    (void)hipFree(g->d_refs);
    delete g;
    return REINA_OK;
}

// the table-dependent parts of DevParams: [nrc, iot_mask) and [n_ranges, end)
#define DP_TAB0_BEGIN offsetof(DevParams, nrc)
#define DP_TAB0_END offsetof(DevParams, iot_mask)
#define DP_TAB1_BEGIN offsetof(DevParams, n_ranges)
static_assert(DP_TAB0_BEGIN % 4 == 0 && DP_TAB0_END % 4 == 0 && DP_TAB1_BEGIN % 4 == 0, "word copies");

// member 0's freshly uploaded tables, device to device, into every other member of the group
__global__ __launch_bounds__(256) void k_group_tables(const MemberRef *refs) {
    const MemberRef &src = refs[0], &dst = refs[blockIdx.y + 1];
    const uint32_t stride = gridDim.x * blockDim.x, first = blockIdx.x * blockDim.x + threadIdx.x;
    {
        const uint32_t *s_ = reinterpret_cast<const uint32_t *>(src.T);
        uint32_t *d_ = reinterpret_cast<uint32_t *>(const_cast<Tables *>(dst.T));
        for (uint32_t k = first; k < sizeof(Tables) / 4; k += stride) d_[k] = s_[k];
    }
    const uint32_t *sp = reinterpret_cast<const uint32_t *>(src.P);
    uint32_t *dp_ = reinterpret_cast<uint32_t *>(const_cast<DevParams *>(dst.P));
    for (uint32_t k = DP_TAB0_BEGIN / 4 + first; k < DP_TAB0_END / 4; k += stride) dp_[k] = sp[k];
    for (uint32_t k = DP_TAB1_BEGIN / 4 + first; k < sizeof(DevParams) / 4; k += stride) dp_[k] = sp[k];
}

int reina_group_upload_contact_tables(reina_group_t *g, const reina_contact_tables_t *t, void *stream) {
    if (!g) return REINA_E_INVALID;
    // the members sample from identical tables: one transfer from the host (member 0), one device-to-device
    // broadcast to the others -- two launches whatever the size of the group
    reina_engine_t *e0 = g->members[0];
    int rc = reina_upload_contact_tables(e0, t, stream);
    if (rc) return rc;
    const uint32_t K = (uint32_t)g->members.size();
    if (K == 1) return REINA_OK;
    for (uint32_t k = 1; k < K; k++) {   // host mirrors follow
        reina_engine_t *m = g->members[k];
        std::memcpy(reinterpret_cast<char *>(&m->h_params) + DP_TAB0_BEGIN, reinterpret_cast<const char *>(&e0->h_params) + DP_TAB0_BEGIN,
                    DP_TAB0_END - DP_TAB0_BEGIN);
        std::memcpy(reinterpret_cast<char *>(&m->h_params) + DP_TAB1_BEGIN, reinterpret_cast<const char *>(&e0->h_params) + DP_TAB1_BEGIN,
                    sizeof(DevParams) - DP_TAB1_BEGIN);
        std::memcpy(&m->h_tables, &e0->h_tables, sizeof(Tables));
    }
    hipLaunchKernelGGL(k_group_tables, dim3(32, K - 1), dim3(256), 0, (hipStream_t)stream, g->d_refs);
    HIP_CHECK(hipGetLastError());
    return REINA_OK;
}

// what an attachment (k_addons.inc) queues around every day of a run: `before` ahead of the day's opening launch (a policy),
// `after` behind its last one (a transmission log)
struct attachment;
struct day_hooks {
    attachment *a = nullptr;
    int (*before)(attachment *a, const reina_day_t &d, hipStream_t s) = nullptr;
    int (*after)(attachment *a, const reina_day_t &d, hipStream_t s) = nullptr;
};

static int group_run_days(reina_group_t *g, const reina_day_t *days, uint32_t n_days, int32_t *const *history_bases,
                          void *stream, const day_hooks &hooks = day_hooks()) {
    if (!g || !days) return REINA_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t K = (uint32_t)g->members.size();
    for (uint32_t k = 0; k < K; k++) g->h_refs[k].history_base = history_bases ? history_bases[k] : nullptr;
    HIP_CHECK(hipMemcpyAsync(g->d_refs, g->h_refs.data(), sizeof(MemberRef) * K, hipMemcpyHostToDevice, s));
    reina_engine_t *e0 = g->members[0];
    bool tested = false;  // the test-queue kernels run for all members once any member ever tested
    e0->group_lds_rows = e0->group_lds_crows = 0;
    for (auto m : g->members) {
        if (m->h_tables.n_rows > e0->group_lds_rows) e0->group_lds_rows = m->h_tables.n_rows;
        if (m->h_tables.n_crows > e0->group_lds_crows) e0->group_lds_crows = m->h_tables.n_crows;
    }
    for (auto m : g->members) tested = tested || m->testing_ever;
    for (uint32_t d = 0; d < n_days; d++) tested = tested || days[d].testing_mode != RT_NO_TESTING;
    e0->testing_ever = e0->testing_ever || (tested && n_days == 0);
    // (a group of ONE member launches the single-engine kernels, which take the member by value: its history base for this run)
    const MemberRef own_ref = e0->h_ref;
    if (K == 1) e0->h_ref.history_base = g->h_refs[0].history_base;
    for (uint32_t d = 0; d < n_days; d++) {
        reina_day_t dp = days[d];
        dp.history_row = nullptr;
        DayPlan p;
        int rc = hooks.before ? hooks.before(hooks.a, dp, s) : REINA_OK;
        if (rc == REINA_OK) note_testing(e0, dp), rc = plan_engine_day(e0, K, dp, &p);
        if (rc == REINA_OK) {
            launch_day_open(e0, g->d_refs, K, dp, p, d, s);
            launch_day_trace(e0, g->d_refs, K, dp, p, s);
            launch_day_main(e0, g->d_refs, K, dp, p, s);
            launch_day_end(e0, g->d_refs, K, dp, p, s);
            HIP_CHECK_OR(hipGetLastError(), e0->h_ref = own_ref);
        }
        if (rc == REINA_OK && hooks.after) rc = hooks.after(hooks.a, dp, s);
        if (rc) {
            e0->h_ref = own_ref;
            return rc;
        }
    }
    e0->h_ref = own_ref;
    for (auto m : g->members) m->testing_ever = m->testing_ever || e0->testing_ever;
    return REINA_OK;
}

int reina_group_run_days(reina_group_t *g, const reina_day_t *days, uint32_t n_days, int32_t *const *history_bases,
                         void *stream) {
    return group_run_days(g, days, n_days, history_bases, stream);
}

int reina_read_counters(reina_engine_t *e, int32_t *out_host, void *stream) {
    if (!e || !out_host) return REINA_E_INVALID;
    if (!e->bound) return REINA_E_NOT_BOUND;
    hipStream_t s = (hipStream_t)stream;
    HIP_CHECK(hipMemcpyAsync(out_host, e->buf.counters, sizeof(int32_t) * REINA_COUNTER_WORDS, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    return REINA_OK;
}

int reina_read_history(reina_engine_t *e, const int32_t *history_dev, uint32_t n_rows, int32_t *out_host, void *stream) {
    if (!e || !out_host || (n_rows && !history_dev)) return REINA_E_INVALID;
    if (!e->bound) return REINA_E_NOT_BOUND;
    hipStream_t s = (hipStream_t)stream;
    const size_t row = sizeof(int32_t) * REINA_COUNTER_WORDS;
    static_assert(sizeof(int32_t) * REINA_COUNTER_WORDS % 16 == 0, "rows are copied 16 bytes at a time");
    // a page-locked destination (what engine.py passes) is written by a kernel, over the link: one launch instead of the copy
    // engine's two set-ups (REINA_EXPORT=memcpy: the copies, for comparison)
    void *export_dev = nullptr;
    {
        hipPointerAttribute_t at;
        std::memset(&at, 0, sizeof(at));
        if (!e->export_by_copies && hipPointerGetAttributes(&at, out_host) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer &&
            (reinterpret_cast<uintptr_t>(at.devicePointer) & 15u) == 0u)
            export_dev = at.devicePointer;
        else
            (void)hipGetLastError();   // (pageable memory is not an error here: it takes the copies below)
    }
    // (k_export reads 16 bytes a lane: the history rows AND the counter block -- a C-ABI caller may have bound either at any
    // 4-byte offset into a block of its own; anything not 16-byte aligned takes the copies below)
    if (export_dev && (n_rows == 0 || (reinterpret_cast<uintptr_t>(history_dev) & 15u) == 0u) &&
        (reinterpret_cast<uintptr_t>(e->buf.counters) & 15u) == 0u) {
        const uint32_t n_hist4 = (uint32_t)(row * n_rows / 16), n_cnt4 = (uint32_t)(row / 16);
        const uint32_t blocks = (n_hist4 + n_cnt4 + 255u) / 256u;
        hipLaunchKernelGGL(k_export, dim3(blocks < 64u ? blocks : 64u), dim3(256), 0, s, reinterpret_cast<const uint4 *>(history_dev), n_hist4,
                           reinterpret_cast<const uint4 *>(e->buf.counters), n_cnt4, reinterpret_cast<uint4 *>(export_dev));
        HIP_CHECK(hipGetLastError());
    } else {
        if (n_rows) HIP_CHECK(hipMemcpyAsync(out_host, history_dev, row * n_rows, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipMemcpyAsync(out_host + (size_t)n_rows * REINA_COUNTER_WORDS, e->buf.counters, row, hipMemcpyDeviceToHost, s));
    }
    HIP_CHECK(hipStreamSynchronize(s));
    return REINA_OK;
}

int reina_profile_enable(reina_engine_t *e, int enable) {
    if (!e) return REINA_E_INVALID;
    e->profile = enable != 0;
    e->profile_day_only = enable < 0;      // -k: stride k, and only k_day (the stream + contact sampling) is timed
    if (enable < 0) enable = -enable;
    e->profile_stride = enable > 1 ? (uint32_t)(enable < 4 ? 4 : enable) : 1u;   // (four kinds take turns: stride >= 4)
    // create timing events up front: hipEventCreate inside a timed region costs microseconds each
    while (e->profile && e->ev_pool.size() < 1024) {
        hipEvent_t ev;
        HIP_CHECK(hipEventCreateWithFlags(&ev, REINA_TIMING_EVENT_FLAGS));
        e->ev_pool.push_back(ev);
    }
    return REINA_OK;
}

int reina_profile_read_kernels(reina_engine_t *e, double *ms_total, uint64_t *launches) {
    if (!e) return REINA_E_INVALID;
    HIP_CHECK(hipDeviceSynchronize());
    resolve_profile(e);
    for (int k = 0; k < REINA_PK_NR; k++) {
        if (ms_total) ms_total[k] = e->k_ms[k];
        if (launches) launches[k] = e->k_launches[k];
        e->k_ms[k] = 0;
        e->k_launches[k] = 0;
    }
    return REINA_OK;
}

int reina_profile_read(reina_engine_t *e, double *scan_ms_total, uint64_t *scan_launches, double *all_ms_total) {
    double ms[REINA_PK_NR];
    uint64_t n[REINA_PK_NR];
    const int rc = reina_profile_read_kernels(e, ms, n);
    if (rc) return rc;
    if (scan_ms_total) *scan_ms_total = ms[REINA_PK_DAY];
    if (scan_launches) *scan_launches = n[REINA_PK_DAY];
    if (all_ms_total) {   // every timed launch of every kind
        *all_ms_total = 0;
        for (int k = 0; k < REINA_PK_NR; k++) *all_ms_total += ms[k];
    }
    return REINA_OK;
}

}  // extern "C"

// what the parts below share: wave helpers, link classification, launch geometry, the attachment base
#include "k_addons.inc"

// snapshots of an engine between days (include/reina_snapshot.h): kernels and entry points
#include "k_snapshot.inc"

// transmission-tree reports of an engine between days (include/reina_transmission.h): kernels and entry points
#include "k_transmission.inc"

// the particle filter's in-group clone (include/reina_filter.h): kernel and entry point
#include "k_filter.inc"

// triggered interventions (include/reina_policy.h): the deciding kernel and entry points
#include "k_policy.inc"

// the dated transmission log (include/reina_txlog.h): kernels and entry points
#include "k_txlog.inc"

// the clinical course log attached to a transmission log (include/reina_course.h): kernels and entry points
#include "k_course.inc"

// the detection report taken of a course log and its transmission log (include/reina_detection.h): kernel and entry point
#include "k_detection.inc"

// the vaccination report taken of a transmission log (include/reina_vaccination.h): kernel and entry point
#include "k_vaccination.inc"

// a policy and a log in one run, and the regime report taken of a transmission log (include/reina_regime.h): kernel and entry points
#include "k_regime.inc"

// the clone of a logged group: the particle filter carries both logs (include/reina_filter_log.h): kernel and entry point
#include "k_filter_log.inc"

// lineage reports: mixing by period and trees by seeding period (include/reina_lineage.h): kernels and entry points
#include "k_lineage.inc"

// ensemble summaries: bands, sums, peaks and exceedance of the members' histories (include/reina_summary.h): kernels and entry point
#include "k_summary.inc"

// per-member disease parameters of an engine group (include/reina_params.h): the expanding kernel and entry points
#include "k_params.inc"
