// reina_hip.hip part: k_small_days -- a run of days of a SMALL unsharded population in ONE launch (round 6).
// Included by reina_hip.hip only (one translation unit); not a standalone header.
// ---------------------------------------------------------------------------------------------
// One iterate() of the reference is one pass (main.pyx:1994-2018).  Here a day is three dependent phases -- the opening (imports,
// test queue, tracing), the stream with the contact sampling, the installs beside the bed / ICU walk -- and for a HUS-sized
// population each of them is a chain of a few dependent round trips: as three launches the day is (3 x the dispatch floor) +
// (the chains), 37 us of which 12 are launch boundaries (a dependent launch boundary: 3.9-4.1 us; tools/ubench_xcd.hip).  A
// barrier among a few dozen co-resident workgroups -- agent-scope release, a counter, agent-scope acquire -- costs 1.7 us
// (same measurement, 32 workgroups), so a population whose phases fit a few dozen workgroups runs a whole STRETCH of days --
// the days reina_run_days was handed at once, between two changes of the contact tables -- as ONE launch: the three phases of
// a day are the very device functions the three kernels call (open_role, day_block, hospital_block / install_block) with the
// launch's workgroup number in the place of blockIdx.x, separated by launch-wide barriers, three a day.  The stream's form is
// FEED_PLAIN (k_contacts.inc): a wave holds a handful of tiles, nothing is named by hand, all phases have the whole register file.
// Measured first as one launch PER DAY (two barriers): no gain -- 37.4 us a HUS day against 36.3 as three launches; the phases ran
// 5.5 us longer on 32 workgroups than on their own grids of 66 / 206 / 79, which is what the two saved boundaries were worth,
// and a launch of 1024-thread workgroups with 150 KB of LDS each takes longer to come up and to drain than the in-kernel stamps
// see (profiles/r06_evidence/small_days.txt).  The launch that STAYS -- this kernel: one ramp and one drain per stretch, the tables
// staged into LDS once per stretch instead of once per day and workgroup -- was built next and is bit-exact against oracle B on every
// scenario family, and it is SLOWER still: 41.3 us a HUS day in the round driver's window (34 us in the kernel by HIP events) against
// 36.3 as three launches a day.  In-kernel stamps, days 5-25: the three phases with their barriers take 10.5 + 14.1 + 12.6 us a day
// -- the chains between the barriers run 9 us longer than on the three kernels' own grids (a control workgroup that opens, a
// stream of 31 workgroups instead of 206, 31 installing ones instead of 78, the day's record read through the scalar cache instead
// of kernel arguments, a loop body whose invariants the compiler carries in 100 spilled registers) and the slowest workgroup of a phase
// holds the other 31 at its barrier.  The day of a small population is a chain of ~15 dependent round trips of 1.6 us; launch
// boundaries are 12 us of it and a barrier is cheaper than a boundary, but not by more than the phases lose on a fraction of the
// chip.  OFF by default (REINA_FUSED_DAY=1 switches it on); kept with its tests as the measured answer to round 5's verdict item 2.
// Roles: workgroup 0 is the CONTROL workgroup -- it opens the day (prologue_block), places the weekly imports beside the stream,
// walks or applies the bed / ICU events; it never streams and keeps no tables.  Workgroups 1.. take the opening's other roles
// (import helpers, the test queue), stream, and install; their LDS image of the tables stays from day to day -- the opening's
// and the installs' LDS blocks lie over the stream's QUEUES, which are empty between two streams.
// Who takes this path: reina_hip.hip, small_days_run (an unsharded single engine of at most REINA_HOSP_SMALL_AGENTS agents, days
// without a vaccination programme and with at most one workgroup's worth of weekly imports, a process with few live engines:
// every workgroup of the launch must be resident).
//
// The barrier: every workgroup adds 1 to a counter that only grows -- the k-th barrier of the engine's life is through when the
// counter has reached k x W (the host numbers the barriers: `bar_base`) --, polls with relaxed loads and a bounded poll count (a
// launch that is not resident as a whole flags the day, REINA_PROBLEM_SYNC_TIMEOUT, instead of hanging the box).  The release
// before and the acquire behind it are agent-scope fences by ONE thread between two workgroup barriers: they write back / invalidate
// the compute unit's view, which is what the whole workgroup reads through (tools/ubench_xcd.hip checked exactly this shape for
// stale reads across the eight XCDs: none; without the fences: every read).
// (a barrier that gave up leaves word 32 of the counter block set: every later barrier of the process's launches on this engine returns
// at once -- the run has failed, it must not also sit through three timeouts a day)
__device__ __forceinline__ void small_day_barrier(GAS uint32_t *counter, uint32_t target, GAS int32_t *counters) {
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        uint32_t polls = 0;
        // (the counter wraps after 2^32 arrivals -- 45 million days at 32 workgroups --: compared as a signed distance)
        while ((int32_t)(__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - target) < 0) {
            __builtin_amdgcn_s_sleep(1);
            if ((++polls & 1023u) == 0u && __hip_atomic_load(counter + 32, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) break;
            if (polls > (1u << 24)) {
                set_problem(counters, REINA_PROBLEM_SYNC_TIMEOUT);
                __hip_atomic_store(counter + 32, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                break;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
}

// one day of the stretch: its descriptor and what the host decided about its launch shape (reina_launch.h: plan_day)
struct SmallDayRec {
    reina_day_t dp;
    int32_t weekly_own, mode;      // k_open's roles (k_testing.inc: open_role)
    uint32_t stream_imports;       // 1: the control workgroup places the day's weekly imports beside the stream
    uint32_t pad_;
};
static_assert(sizeof(SmallDayRec) % 8 == 0, "records are copied as words");
struct SmallGeom {
    uint32_t n_days;
    uint32_t lds_rows, lds_crows, day_flags;   // k_day's launch parameters
    uint32_t scan_tiles;       // tiles of 512 agents
    uint32_t bar_base;         // barriers this engine's launches have passed before this one
    uint32_t *bar;             // the engine's barrier counter
    const SmallDayRec *days;   // the stretch's records (device memory, written before the launch, constant to it)
};
#define SMALL_BARRIERS_PER_DAY 3u
// the control workgroup's LDS: the hospital role's REINA_MAX_HOSP_EVENTS keys, behind them the ordered walk's maps, then the events'
// per-age histogram (every workgroup's histogram lives there: beyond the largest image of the stream)
#define SMALL_SF_OFF ((size_t)REINA_MAX_HOSP_EVENTS * 8)
#define SMALL_HL_OFF (SMALL_SF_OFF + sizeof(SatFn) * 2 * HOSP_THREADS)
#define SMALL_TAIL_BYTES (SMALL_HL_OFF + sizeof(int32_t) * HL_NR * REINA_MAX_AGES)
// a streaming workgroup's opening / install blocks lie over the stream's queues (DayShared::needy .. grp)
#define SMALL_OVL_OFF ((offsetof(DayShared, needy) + 15u) & ~(size_t)15u)
static_assert(offsetof(DayShared, grp) - SMALL_OVL_OFF >= sizeof(OpenLds) && offsetof(DayShared, grp) - SMALL_OVL_OFF >= sizeof(OnsetStage),
              "the opening's block and the installs' stage fit the queues of the stream");
static_assert(SMALL_OVL_OFF % 16 == 0, "aligned like the launch's LDS");
static_assert(sizeof(DayShared) + (size_t)REINA_LDS_ROWS * DAY_ROW_BYTES + (size_t)REINA_LDS_CROWS * DAY_CROW_BYTES <= SMALL_HL_OFF,
              "the events' histogram lies beyond the largest image of the stream");
static_assert(sizeof(OpenLds) <= SMALL_SF_OFF, "the control workgroup's opening block lies in front of the maps");
static_assert(DAY_THREADS == HOSP_THREADS && PRO_THREADS == HOSP_THREADS, "one block shape for the three phases");
static size_t small_day_lds_bytes(uint32_t lds_rows, uint32_t lds_crows) {
    (void)lds_rows; (void)lds_crows;
    return SMALL_TAIL_BYTES;   // (the stream's image is smaller whatever the rows: the assertion above)
}

__global__ __launch_bounds__(HOSP_THREADS) void k_small_days(MemberRef one_, SmallGeom g) {
    extern __shared__ __align__(16) unsigned char smem_sd[];
    const uint32_t W = gridDim.x, bx = blockIdx.x;
    GAS uint32_t *bar = (GAS uint32_t *)g.bar;
    GAS int32_t *counters = (GAS int32_t *)one_.B.counters;
    const CAS SmallDayRec *recs = (const CAS SmallDayRec *)g.days;
    unsigned char *ovl = bx == 0 ? smem_sd : smem_sd + SMALL_OVL_OFF;
    SatFn (*s_f)[HOSP_THREADS] = reinterpret_cast<SatFn (*)[HOSP_THREADS]>(smem_sd + SMALL_SF_OFF);
    int32_t (*s_hl)[REINA_MAX_AGES] = reinterpret_cast<int32_t (*)[REINA_MAX_AGES]>(smem_sd + SMALL_HL_OFF);
    const uint32_t scan_waves = (W - 1u) * DAY_WAVES;
    uint32_t nb = g.bar_base;
    DIAG_CLOCK(SMALL, ss_t);   // (-DREINA_SMALL_STAMPS: every workgroup's time in each phase of a day, summed and the longest)
    for (uint32_t d = 0; d < g.n_days; d++) {
        // (the parameter block and the tables are constants: left alone, the compiler reads everything the three phases will ever ask
        // of them in front of this loop and carries it through -- 118 registers in scratch.  A day's phases get their pointers
        // afresh, through a statement the compiler cannot see through, and read what they need where they need it.)
        MemberRef mref_ = one_;
        asm volatile("" : "+s"(mref_.P), "+s"(mref_.T));
        // (the record through the constant address space: uniform reads of it are scalar loads wherever they stand, as a single day's
        // kernel arguments are)
        const reina_day_t &dp = *(const reina_day_t *)&recs[d].dp;
        const int weekly_own = recs[d].weekly_own, mode = recs[d].mode;
        const uint32_t stream_imports = recs[d].stream_imports;
        // phase 1, the day's opening: role = workgroup number (the launch is resident as a whole: no tickets)
        open_role<false>(mref_, dp, 0u, weekly_own, mode, bx, W, ovl);
        DIAG_LAP(SMALL, DIAG_SMALL_OPENING, DIAG_BARRIER_THREAD0, ss_t, one_.B.mirror);
        small_day_barrier(bar, ++nb * W, counters);
        DIAG_LAP(SMALL, DIAG_SMALL_BARRIER1, DIAG_BARRIER_THREAD0, ss_t, one_.B.mirror);
        // phase 2, the stream + contact sampling on workgroups 1..; the control workgroup places the weekly imports beside it
        if (bx == 0) {
            if (stream_imports) day_imports_block(mref_, dp, smem_sd, 0u, 1u);
        } else {
            day_block<false, FEED_PLAIN>(mref_, dp, g.lds_rows, g.lds_crows, g.day_flags, 0u, bx - 1u, W - 1u, smem_sd, d != 0u);
        }
        DIAG_LAP(SMALL, DIAG_SMALL_STREAM, DIAG_BARRIER_THREAD0, ss_t, one_.B.mirror);
        small_day_barrier(bar, ++nb * W, counters);
        DIAG_LAP(SMALL, DIAG_SMALL_BARRIER2, DIAG_BARRIER_THREAD0, ss_t, one_.B.mirror);
        // phase 3, k_hosp_install's small shape: the control workgroup has the bed / ICU events (the ordered walk, or all granted),
        // the others install
        if (bx == 0) {
            if (hosp_day_is_ordered(global_buffers(mref_.B))) hospital_block(mref_, dp, s_hl, s_f);
            else install_block<false>(mref_, dp, scan_waves, g.scan_tiles, 0, 1, true, true, s_hl, nullptr);
        } else {
            install_block<false>(mref_, dp, scan_waves, g.scan_tiles, bx - 1u, W - 1u, false, false, s_hl, reinterpret_cast<OnsetStage *>(ovl));
        }
        DIAG_LAP(SMALL, DIAG_SMALL_INSTALLS, DIAG_BARRIER_THREAD0, ss_t, one_.B.mirror);
        // (the next day's opening reads what the installs wrote: tomorrow's test queue, the counters of the snapshot)
        small_day_barrier(bar, ++nb * W, counters);
        DIAG_LAP(SMALL, DIAG_SMALL_BARRIER3, DIAG_BARRIER_THREAD0, ss_t, one_.B.mirror);
    }
}
