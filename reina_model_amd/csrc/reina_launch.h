// The plan of one day's launches: every grid, role count and LDS row count of the day's kernels as a PURE function of a few sizes
// and switches of the engine, the group size, whether anyone ever tested, the contact rows to stage and the day's descriptor.
// Host only, no GPU header, no engine struct: reina_hip.hip plans a day once and its launchers only launch; tests/test_launch_plan.py
// compiles this file alone -- results do not depend on launch geometry, so a wrong grid shows up nowhere else but in speed.
#ifndef REINA_LAUNCH_H
#define REINA_LAUNCH_H
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "../../include/reina_hip.h"
#include "reina_prims.h"   // RT_*: the testing modes

// block shapes and thresholds of the day's kernels (the kernel files read them from here)
#define PRO_THREADS 1024    // k_open, k_vaccinate
#define DAY_THREADS 1024    // k_day
#define DAY_WAVES (DAY_THREADS / 64)
#define HOSP_THREADS 1024   // k_hosp_presort, k_hosp_install
#define VACC_CHUNKS 16      // chunks of PRO_THREADS agents one step of a vaccinating workgroup scans
#define DAY_SPARSE_MIN_TILES 4u   // tiles per wave from which on a day is sparse (plan_day decides)
#define REINA_LDS_ROWS 28   // distinct contact rows a workgroup keeps in LDS; rows beyond are read through L2
#define REINA_LDS_CROWS 20  // distinct count rows a workgroup keeps in LDS; rows beyond are read through L2
#define OPEN_WEEKLY_IN_STREAM 0x40000000   // k_open's weekly_own: the weekly imports are placed beside the stream (k_testing.inc: open_role)
enum { HI_HOSP_WG = 1, HI_INSTALL = 2, HI_EVENTS = 4 };   // k_hosp_install's flags (k_install.inc)

// how the launch's workgroups are dealt to the day's programmes.  `parallel`: the programmes' windows are pairwise DISJOINT
// (age tiers side by side), so their order does not matter and every programme has workgroups of its own, g[k] of them
// behind those of programmes 0 .. k - 1, all at once; otherwise all workgroups take the programmes one after the other.
struct VaccGeom { uint32_t parallel; uint16_t g[REINA_MAX_VACCINATIONS]; };
struct LaunchShape {   // what the geometry reads from an engine, and nothing else: sizes, then the switches
    uint32_t n_agents, n_cus, n_shards, exact, hosp_ranges, hosp_parallel, cand_ovf_cap, max_work_items, xchg_cap;
    uint32_t import_wgs, walk_div, vacc_one_wg, open_tickets, imports_in_open, day_mode, lds_rows_cap, small_wgs;
};
struct DayPlan {
    // REINA_PH_OPEN: k_open's workgroups, its import roles (k_testing.inc: open_role), what it does about the test queue (0 nothing,
    // 1 detects, 2 detects + traces level 0, 3 both levels) and whether its roles go by arrival ticket
    uint32_t open_grid, open_mode, open_tickets;
    int32_t weekly_own;
    uint32_t trace1_in_open;   // k_test_trace1 behind k_open (mode 2 of an engine without exact attribution)
    uint32_t xtrace;           // exact attribution on a contact-tracing day: tracing level by level, an exchange behind each
    uint32_t trace1_grid, xchg_grid;   // k_test_trace1; a launch that takes in the records of an exchange (k_xtrace, k_feedback)
    // REINA_PH_MAIN
    uint32_t vacc_grid;        // k_vaccinate's workgroups; 0: no programme today
    VaccGeom vacc;
    uint32_t lds_rows, lds_crows;   // contact / count rows k_day stages (its LDS bytes follow from them: day_shared_bytes)
    uint32_t day_blocks;       // streaming workgroups of k_day
    uint32_t stream_imports;   // workgroups of k_day's launch that place the weekly imports beside the stream
    uint32_t sparse;           // the form of the stream (k_contacts.inc)
    uint32_t scan_waves, scan_tiles;   // the per-wave slices every later launch walks; tiles of 512 agents
    uint32_t presort_grid;     // k_hosp_presort (a sharded population: its event buckets sorted BEFORE the all-reduce); 0: none
    // REINA_PH_END
    uint32_t remote_grid;      // k_remote (a sharded population); 0: none
    uint32_t install_grid, install_flags, n_walk;   // k_hosp_install
    uint32_t install_walk_lds; // its dynamic LDS: 1 the walkers' sorting network, 0 workgroup 0's REINA_MAX_HOSP_EVENTS keys
};
enum { PLAN_OK = 0, PLAN_E_DAY = 1, PLAN_E_COUNTS = 2 };   // plan_day's refusals (the caller has the texts)

static inline int grid_for(uint32_t n_items, int threads, int max_blocks) {
    const long blocks = ((long)n_items + threads - 1) / threads;
    return (int)(blocks < 1 ? 1 : blocks > max_blocks ? max_blocks : blocks);
}
// a member's share of the chip's compute units: all of them for a single engine, never less than one
static inline uint32_t member_cap(uint32_t n_cus, uint32_t K) { return K > 1 ? (n_cus / K > 0 ? n_cus / K : 1u) : n_cus; }
static inline uint32_t scan_tiles_for(uint32_t n_agents) { return ((n_agents >> 2) + 127u) / 128u; }
// rows of a table staged in LDS: what the tables (or the group, or a policy's bank) hold, within the kernel's room and the tests' cap
static inline uint32_t lds_rows_for(const LaunchShape &sh, uint32_t rows, uint32_t room) {
    if (rows > room) rows = room;
    return sh.lds_rows_cap && rows > sh.lds_rows_cap ? sh.lds_rows_cap : rows;
}
// k_open's helper roles for the day's imports
static inline uint32_t open_helpers(int32_t weekly_own) {
    return weekly_own == OPEN_WEEKLY_IN_STREAM ? 0u : weekly_own > 0 ? (uint32_t)weekly_own : (uint32_t)-weekly_own;
}

// One day's launches for K engine instances at once (K = 1: a single engine; K > 1: a group of identically configured engines,
// one launch per phase for all of them, member = blockIdx.y).  0, or the refusal (checked in this order, nothing planned).
static inline int plan_day(const LaunchShape &sh, uint32_t K, bool testing_ever, uint32_t rows, uint32_t crows, const reina_day_t &dp, DayPlan *p) {
    memset(p, 0, sizeof(*p));
    // claim / mirror keys carry the day in 12 bits (rp_order_key) and claim[] is never cleared: from day 4096 on, stale claims would beat today's
    if (dp.day >= REINA_MAX_DAYS) return PLAN_E_DAY;
    if (dp.n_import_batches > REINA_MAX_IMPORT_BATCHES || dp.n_vaccinations > REINA_MAX_VACCINATIONS) return PLAN_E_COUNTS;
    const uint32_t N = sh.n_agents, cap = member_cap(sh.n_cus, K);
    const bool ct = dp.testing_mode == RT_ALL_WITH_SYMPTOMS_CT;
    p->xtrace = sh.exact && ct;
    p->scan_tiles = scan_tiles_for(N);
    uint32_t n_pre = 0, n_post = 0;
    for (uint32_t b = 0; b < dp.n_import_batches; b++)
        (dp.import_batches[b].pre_init ? n_pre : n_post) += dp.import_batches[b].count;
    // weekly imports on a day without intervention imports (which would share their claim keys) have workgroups of their
    // own: one per wave of imports, at most 16 (k_open.inc, imports_any); members of a group take one each (they wait on each
    // other, and a group's launch is not resident as a whole)
    // (> 0: so many workgroups for the weekly imports; <= 0: the opening workgroup places the day's imports, with -weekly_own
    // helpers: open_role, k_testing.inc)
    int32_t weekly_own = n_pre == 0 && n_post > 0;
    if (K == 1) {
        const uint32_t most = n_pre > n_post ? n_pre : n_post;
        int32_t w = (int32_t)((most + 511u) / 512u);
        if (w > (int32_t)sh.import_wgs) w = (int32_t)sh.import_wgs;
        if (weekly_own) weekly_own = w;
        else if (n_pre > 0 && w > 1) weekly_own = -(w - 1);
    }
    // k_day's workgroups for one engine instance: one 512-agent tile per wave (small populations) up to one workgroup of 16
    // waves per CU, whose waves then walk several tiles; members of a group share the chip.  Every later kernel takes the
    // resulting wave count as a parameter (the per-wave slices of the lists).
    const uint32_t most_blocks = cap < REINA_MAX_SCAN_WAVES / DAY_WAVES ? cap : REINA_MAX_SCAN_WAVES / DAY_WAVES;
    uint32_t day_blocks = (p->scan_tiles + DAY_WAVES - 1) / DAY_WAVES;
    day_blocks = day_blocks < 1 ? 1 : day_blocks > most_blocks ? most_blocks : day_blocks;
    // weekly imports on a day without intervention imports are placed in k_day's launch, beside the stream, by workgroups
    // of their own behind the streaming ones (k_open.inc: deferred placement); all of them fit the chip together.
    // (Their records go to the shared candidate overflow list: only when the day's imports fit it with room to spare for real
    // overflow records -- a caller of the C ABI may have sized max_candidates tightly -- else the opening launch places them)
    if (weekly_own > 0 && dp.day + 1u < REINA_MAX_DAYS && !sh.imports_in_open && (uint64_t)n_post * 2u <= sh.cand_ovf_cap) {
        p->stream_imports = K == 1 ? (uint32_t)weekly_own : 1u;
        if (day_blocks + p->stream_imports > cap && cap > p->stream_imports) day_blocks = cap - p->stream_imports;
        weekly_own = OPEN_WEEKLY_IN_STREAM;
    }
    p->weekly_own = weekly_own;
    p->day_blocks = day_blocks;
    p->scan_waves = day_blocks * DAY_WAVES;
    {   // the opening: roles (0 opens the day, 1 weekly imports, 2.. the test queue)
        // (groups: the members share the chip, so each gets proportionally fewer workgroups per phase; a single engine's test-queue
        // roles are NOT held to member_cap -- up to 64 even on a smaller chip --, hence the K > 1)
        uint32_t tg = (uint32_t)grid_for(N / 64 + 1, PRO_THREADS, 64);
        if (K > 1 && tg > cap) tg = cap;
        const uint32_t helpers = open_helpers(weekly_own), g0 = 1 + (helpers > 1 ? helpers : 1), g = g0 + tg;
        // roles by arrival ticket unless the launch is resident as a whole -- and, measured, for small populations too
        // (HUS year: k_open 10.4 us a day with tickets, 11.2 by block number; 10^8 agents: 14.6 against 14.1)
        p->open_tickets = (K > 1 || g > sh.n_cus || sh.open_tickets || N <= 8000000u) ? 1 : 0;
        // detects + traces: both levels in the opening of a population up to 8 000 000; beyond, and under exact attribution
        // (behind the exchange of the level-0 requests), level 1 by a launch of its own
        p->open_mode = !testing_ever ? 0u : !ct ? 1u : (N <= 8000000u && !p->xtrace) ? 3u : 2u;
        p->open_grid = p->open_mode == 0u ? g0 : g;
        p->trace1_in_open = p->open_mode == 2u && !p->xtrace;
        p->trace1_grid = (uint32_t)grid_for(N / 64 + 1, 256, 256);
        p->xchg_grid = sh.exact ? (uint32_t)grid_for(sh.xchg_cap * (sh.n_shards - 1u) / 4u + 1u, 256, 128) : 0u;
    }
    if (dp.n_vaccinations) {
        // a day on which some programme's number exceeds a step of 16 x 1024 agents: a chain of workgroups, one step each, with room
        // for a third more agents than the largest number (k_open.inc: pro_vaccinate_chain; the programmes one after the other, the
        // launch agreeing on each one's end); otherwise one workgroup.  (the numbers as the kernel clips them: a programme whose window
        // holds fewer agents never needs the chain.)  Members of a group chain too while the whole launch stays resident.
        uint32_t most = 0, need[REINA_MAX_VACCINATIONS], sum_need = 0;
        bool disjoint = dp.n_vaccinations > 1;
        for (uint32_t k = 0; k < dp.n_vaccinations; k++) {
            const reina_vaccination_t &vk = dp.vaccinations[k];
            const uint32_t window = vk.idx_end > vk.idx_start ? vk.idx_end - vk.idx_start : 0u;
            const uint32_t nrk = vk.nr < window ? vk.nr : window;
            if (nrk > most) most = nrk;
            need[k] = (nrk + nrk / 3u) / (VACC_CHUNKS * PRO_THREADS) + 1u;
            sum_need += need[k];
            for (uint32_t j = 0; j < k; j++)
                if (vk.idx_start < dp.vaccinations[j].idx_end && dp.vaccinations[j].idx_start < vk.idx_end) disjoint = false;
        }
        p->vacc_grid = 1;
        // (the published words live in the head of buffers.scan_lists: 16 programmes x 512 + 16 arrival words, 64 bits each)
        if (most > VACC_CHUNKS * PRO_THREADS && sh.max_work_items >= 8192 + 16 && !sh.vacc_one_wg) {
            const uint32_t vcap = cap < 256u ? cap : 256u;   // (member_cap's floor of one: the launch's one workgroup at the least, whatever K)
            if (disjoint && sum_need <= vcap) {
                // age tiers side by side (windows pairwise disjoint: the order of the programmes does not matter): every
                // programme on workgroups of its own, all at once
                p->vacc.parallel = 1u;
                for (uint32_t k = 0; k < dp.n_vaccinations; k++) p->vacc.g[k] = (uint16_t)need[k];
                p->vacc_grid = sum_need;
            } else {
                const uint32_t vg = (most + most / 3u) / (VACC_CHUNKS * PRO_THREADS) + 1u;
                p->vacc_grid = vg > vcap ? vcap : vg;
            }
        }
    }
    p->lds_rows = lds_rows_for(sh, rows, REINA_LDS_ROWS);
    p->lds_crows = lds_rows_for(sh, crows, REINA_LDS_CROWS);
    // the form of the stream (k_contacts.inc): sparse from DAY_SPARSE_MIN_TILES tiles per wave on -- every day of such a population:
    // a threshold on yesterday's active agents (rounds 4-5, decided in the kernel) never chose the dense form where the sparse
    // one was possible
    p->sparse = sh.day_mode == 2 || (sh.day_mode == 0 && p->scan_tiles >= DAY_SPARSE_MIN_TILES * p->scan_waves);
    if (sh.day_mode == 3) p->sparse = (dp.day & 1u) == 0u;
    if (sh.n_shards > 1) {
        p->presort_grid = (sh.hosp_ranges + 15u) / 16u;
        p->remote_grid = (uint32_t)grid_for(N / 256 + 1, 256, 256);
    }
    // installing workgroups: one wave per unit of a quiet day (3 lists of scan_waves / 8 units + the event buckets), so
    // that no wave walks two dependent chains one after the other; at most one workgroup per CU
    int ig = grid_for(N / 64 + 1, HOSP_THREADS, 128) * 2;
    const uint32_t units = 3u * ((p->scan_waves + 7u) / 8u) + (sh.hosp_ranges + 7u) / 8u;
    const int want = (int)((units + HOSP_THREADS / 64 - 1) / (HOSP_THREADS / 64));
    if (want > ig) ig = want;
    if (ig > (int)sh.n_cus) ig = (int)sh.n_cus;
    // (groups: 128 workgroups for all members together -- every workgroup pays its prologue and its histogram flush)
    // (a group of 128 HUS members, measured in round 4: ONE installing workgroup per member beside the one for the events --
    // 256 workgroups, one per CU, all resident together -- 67 us a launch against 72.5 with two, 70 with three)
    if (K > 1 && ig > (int)(128 / K)) ig = (int)(128 / K) >= 2 ? ((int)(128 / K) & ~1) : 1;
    if (sh.hosp_parallel) {
        // a large population: the launch's first workgroups are the walkers of a day on which the events' order matters
        // (one wave per priority bucket: R / 16 workgroups; on any other day they install too), the others install.
        // One workgroup of 1024 threads per CU: all of them resident together, so the walk runs beside the installs.
        // (the walkers come out of the member's share; what is left, however little, is held to two installing workgroups)
        p->n_walk = (sh.hosp_ranges + sh.walk_div - 1u) / sh.walk_div;
        int rest = (int)cap - (int)p->n_walk;
        if (rest > ig) rest = ig;
        p->install_grid = p->n_walk + (uint32_t)(rest < 2 ? 2 : rest);
        p->install_flags = HI_INSTALL | HI_EVENTS;
        p->install_walk_lds = 1;
    } else {
        // workgroup 0 walks the bed / ICU events of a day on which order matters, beside the installs
        if (ig < 2 && K == 1) ig = 2;
        p->install_grid = (uint32_t)ig + 1u;
        p->install_flags = HI_HOSP_WG | HI_INSTALL | HI_EVENTS;
    }
    return PLAN_OK;
}

// a day of the one-launch form (k_small.inc) needs its helper roles and one test-queue role within the launch's workgroups,
// and at most one workgroup's worth of weekly imports beside the stream
static inline bool plan_fits_small(const LaunchShape &sh, const DayPlan &p) {
    const uint32_t helpers = open_helpers(p.weekly_own);
    return sh.small_wgs >= 1u + (helpers > 1u ? helpers : 1u) + 1u && p.stream_imports <= 1u;
}
#endif  // REINA_LAUNCH_H
