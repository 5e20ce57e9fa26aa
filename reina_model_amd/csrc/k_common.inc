// reina_hip.hip part: device-side parameter blocks, engine-instance references, small device helpers, person_infect.
// Included by reina_hip.hip only (one translation unit); not a standalone header.
// ---------------------------------------------------------------------------------------------
// device-side parameter block (one per engine, lives in HBM, read through the scalar/L1 caches)
struct DevParams {
    reina_disease_t dis;
    int32_t age_start[REINA_MAX_AGES + 1];
    // (the scalars every launch reads at its head share ONE 64-byte line of the scalar cache -- sixteen words: a uniform read of
    // another line is a round trip to L2 on a launch's critical path)
    alignas(64) uint32_t n_agents;
    uint32_t nr_ages, nr_variants;
    uint32_t k0, k1;
    uint32_t max_work_items, max_candidates, max_queue;
    uint32_t max_hosp_events;   // bed / ICU events one day may hold (buffers.hosp_events is sized from it)
    // the day's events by priority range (k_hospital.inc): buckets, log2 of that, keys per bucket; hosp_parallel:
    // one workgroup per bucket walks them (k_hosp_sort / k_hosp_walk) instead of one workgroup for all
    uint32_t hosp_ranges, hosp_range_bits, hosp_bucket_cap, hosp_parallel;
    // candidate buffer = [one region per scanning wave: max_work_items][cross-shard region][overflow region]
    uint32_t cand_ovf_base, cand_ovf_cap;
    uint32_t exact;             // exact cross-shard attribution (include/reina_hip.h): what follows is read by its instantiations only
    // gid_base / gid_mask: reina_prims.h rp_gid_is_local; records per exchange segment, nodes of the infectee pool
    uint32_t gid_base, gid_mask, xchg_cap, pool_cap;
    uint32_t xchg_stride;       // 64-bit words of one exchange segment: REINA_XCHG_SEG_WORDS(xchg_cap, hosp_ranges) (count, records, trailer)
    uint32_t shard_k0[REINA_MAX_SHARDS], shard_k1[REINA_MAX_SHARDS];   // every shard's Philox key (a target recomputes its source's priority)
    int32_t shard_age_start[REINA_MAX_SHARDS][REINA_MAX_AGES + 1];     // every shard's age_start (a source works out its target's age)
    // contact tables
    float nrc[REINA_MAX_AGES];
    int32_t tcount[REINA_MAX_AGES];
    float mask_p[REINA_MAX_AGES][8];
    // sharding
    uint32_t iot_mask[REINA_MAX_VARIANTS];   // bit (day+10) set when infectiousness_over_time[v][day+10] != 0
    uint32_t n_shards, shard_rank, mirror_slots;
    float psus_max[REINA_MAX_VARIANTS];
    uint32_t n_ranges;
    int32_t range_min[REINA_MAX_RANGES], range_max[REINA_MAX_RANGES];
};

#define REINA_AGE_BLOCKS 2048
struct Tables {  // bigger tables staged into LDS by k_day
    // Contact rows are stored once per DISTINCT row: the thresholds of all participant ages of one class of
    // the contact matrix are identical (FI: 16 classes for 101 ages) unless a mobility window splits a
    // class, so a workgroup stages n_rows x (96 thresholds + 256 guide bytes) instead of nr_ages x.
    uint32_t thr[REINA_MAX_AGES][REINA_MAX_ENTRIES];    // [row]
    uint32_t meta[REINA_MAX_AGES][REINA_MAX_ENTRIES];   // [row]
    // search guide, derived from thr at upload: guide[row][b] = first entry of the row whose threshold
    // exceeds b << 24, so "first entry with r < threshold" starts there and walks 0-2 steps
    uint8_t guide[REINA_MAX_AGES][256];                 // [row]
    // place groups, derived from thr and meta at upload: a row's entries are sorted by place (main.pyx:1213-1235: sort_index on
    // (place_type, contact_age)), so the PLACE of a draw -- all that the 49 contacts in 50 which fail the thinning need of their
    // entry, for daily_contacts -- follows from at most five comparisons: grp[row][0..4] = threshold of the last entry of place
    // group 0..4 (0xFFFFFFFF: no such group), [5] = 5 x place of group g in bits [5g, 5g + 5) (the last group's repeated to
    // g = 5: half the bit offset of the place's 10-bit counter field), [6] = groups of the row.  `grouped` (below): every row has at most six groups, i.e. the table is usable.
    uint32_t grp[REINA_MAX_AGES][8];                    // [row]
    int32_t rcount[REINA_MAX_AGES];                     // [row] entries of the row
    uint8_t row_of_age[REINA_MAX_AGES];
    uint32_t n_rows;
    uint32_t uniform_meta;   // every row lists the same (place, contact range) sequence: meta[0] serves all
    uint32_t grouped;        // grp is usable (a caller of the C ABI may pass entries in any order: then the full search serves)
    // contact-COUNT thresholds (reina_contacts.h: rc_count_thresholds), one row per distinct nr_contacts_by_age value, and
    // the search guide of the full class: cguide[row][b] = thresholds of that class at or below b << 24
    uint32_t cthr[REINA_MAX_AGES][REINA_COUNT_WORDS];   // [count row]
    uint8_t cguide[REINA_MAX_AGES][256];                // [count row]
    uint8_t crow_of_age[REINA_MAX_AGES];
    uint32_t n_crows;
    // coarse index -> age map for the target's age: age_block[t >> age_shift] = age of agent (t >> age_shift) << age_shift
    uint32_t age_shift;
    uint8_t age_block[REINA_AGE_BLOCKS];
};
#include "reina_diag.h"     // the diagnostic builds: slot map of buffers.mirror, the stamp, PROF_* / ABLATED
#include "reina_launch.h"   // REINA_LDS_ROWS / _CROWS, the block shapes and thresholds of the day's kernels, VaccGeom, the HI_* flags

// Pointers that reach a kernel through MemberRef (an array in HBM) are generic to the compiler, and
// generic means flat_load / flat_store / flat_atomic: instructions that count against BOTH the vector-
// memory and the LDS counter (every wait for an LDS result also waits for the global loads in flight:
// the scan's prefetched tile, the contacts' gathers) and that take a 64-bit address in two VGPRs.
// GBuffers is reina_buffers_t with the pointers TYPED as global memory: a kernel converts its member's
// buffers once and every access through them is global_* (scalar base + 32-bit offset where it can).
#define GAS __attribute__((address_space(1)))
// The parameter block and the tables are written by uploads BETWEEN launches only (reina_hip.hip: k_upload, hipMemcpy): to a
// kernel they are constants.  Typed as constant address space their uniform reads become s_load (lgkmcnt) wherever they stand --
// typed as global, a read that follows any store of the kernel is a VECTOR load (the scalar cache is not coherent with the
// kernel's own stores, and the compiler cannot know that no store aliases them), and the wait for it, s_waitcnt vmcnt(0), drains
// every load the wave has in flight: k_day's Philox keys (P->k0, P->k1) cost one such drain per 64 contacts until round 4.
#define CAS __attribute__((address_space(4)))
struct GBuffers {
    GAS uint32_t *hot;
    GAS reina_cold_t *cold;
    GAS int32_t *infectees;
    GAS int32_t *counters;
    GAS int32_t *control;
    GAS uint32_t *work_items;
    GAS uint32_t *candidates;
    GAS uint32_t *queue0;
    GAS uint32_t *queue1;
    GAS uint32_t *level1;
    GAS uint64_t *hosp_events;
    GAS int32_t *pressure;
    GAS uint64_t *mirror;
    GAS uint32_t *mirror_meta;
    GAS uint32_t *work_counts;
    GAS uint32_t *scan_lists;
    GAS uint32_t *active_bits;
    GAS uint32_t *infected_bits;
    GAS uint64_t *xsend;
    GAS uint64_t *xrecv;
    GAS uint32_t *infectee_pool;
};
__device__ __forceinline__ GBuffers global_buffers(const reina_buffers_t &b) {
    GBuffers g;
    g.hot = (GAS uint32_t *)b.hot;
    g.cold = (GAS reina_cold_t *)b.cold;
    g.infectees = (GAS int32_t *)b.infectees;
    g.counters = (GAS int32_t *)b.counters;
    g.control = (GAS int32_t *)b.control;
    g.work_items = (GAS uint32_t *)b.work_items;
    g.candidates = (GAS uint32_t *)b.candidates;
    g.queue0 = (GAS uint32_t *)b.queue0;
    g.queue1 = (GAS uint32_t *)b.queue1;
    g.level1 = (GAS uint32_t *)b.level1;
    g.hosp_events = (GAS uint64_t *)b.hosp_events;
    g.pressure = (GAS int32_t *)b.pressure;
    g.mirror = (GAS uint64_t *)b.mirror;
    g.mirror_meta = (GAS uint32_t *)b.mirror_meta;
    g.work_counts = (GAS uint32_t *)b.work_counts;
    g.scan_lists = (GAS uint32_t *)b.scan_lists;
    g.active_bits = (GAS uint32_t *)b.active_bits;
    g.infected_bits = (GAS uint32_t *)b.infected_bits;
    g.xsend = (GAS uint64_t *)b.xsend;
    g.xrecv = (GAS uint64_t *)b.xrecv;
    g.infectee_pool = (GAS uint32_t *)b.infectee_pool;
    return g;
}
// the atomics the kernels use, on global-typed pointers (relaxed, device scope -- what HIP's atomicAdd & co do)
#define GATOMIC_(name, T, builtin) \
    __device__ __forceinline__ T name(GAS T *p, T v) { return builtin(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
GATOMIC_(atomicAdd, int, __hip_atomic_fetch_add)
GATOMIC_(atomicAdd, unsigned int, __hip_atomic_fetch_add)
GATOMIC_(atomicAdd, unsigned long long, __hip_atomic_fetch_add)
GATOMIC_(atomicMin, unsigned long long, __hip_atomic_fetch_min)
GATOMIC_(atomicMax, unsigned long long, __hip_atomic_fetch_max)
GATOMIC_(atomicMax, int, __hip_atomic_fetch_max)
GATOMIC_(atomicOr, unsigned int, __hip_atomic_fetch_or)
GATOMIC_(atomicAnd, unsigned int, __hip_atomic_fetch_and)
GATOMIC_(atomicExch, unsigned int, __hip_atomic_exchange)
GATOMIC_(atomicExch, int, __hip_atomic_exchange)
#undef GATOMIC_
__device__ __forceinline__ int atomicCAS(GAS int *p, int expect, int desired) {
    __hip_atomic_compare_exchange_strong(p, &expect, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expect;
}
// HIP's uint2 / uint4 are classes whose copy operations want generic references: records in global-typed
// memory are moved as plain vectors
typedef uint32_t v2u_ __attribute__((ext_vector_type(2)));
typedef uint32_t v4u_ __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint2 gld(const GAS uint2 *p) {
    const v2u_ v = *reinterpret_cast<const GAS v2u_ *>(p);
    return make_uint2(v.x, v.y);
}
__device__ __forceinline__ uint4 gld(const GAS uint4 *p) {
    const v4u_ v = *reinterpret_cast<const GAS v4u_ *>(p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void gst(GAS uint2 *p, uint2 v) {
    v2u_ w;
    w.x = v.x; w.y = v.y;
    *reinterpret_cast<GAS v2u_ *>(p) = w;
}
__device__ __forceinline__ void gst(GAS uint4 *p, uint4 v) {
    v4u_ w;
    w.x = v.x; w.y = v.y; w.z = v.z; w.w = v.w;
    *reinterpret_cast<GAS v4u_ *>(p) = w;
}
__device__ __forceinline__ unsigned int atomicCAS(GAS unsigned int *p, unsigned int expect, unsigned int desired) {
    __hip_atomic_compare_exchange_strong(p, &expect, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return expect;
}

// what a kernel needs to know about one engine instance.  Every kernel takes an array of these and
// works on element blockIdx.y: a single engine launches with grid.y = 1, a Monte-Carlo group of K
// engines with grid.y = K (one launch per phase for the whole ensemble).
struct MemberRef {
    const DevParams *P;
    const Tables *T;
    reina_buffers_t B;
    int32_t *history_base;  // group runs: row k of this member's history is history_base + k * COUNTER_WORDS
};

// The kernels of a day exist twice: GROUP = true finds its member in the array (an engine group: element blockIdx.y),
// GROUP = false takes the one member BY VALUE as a kernel argument -- pointers and the like then come straight from the
// kernel-argument segment instead of through two dependent loads from HBM (array -> MemberRef -> DevParams), about a
// microsecond at the head of every launch, which matters when a whole day of a HUS-sized population takes forty.
// ... and a third time for a shard under EXACT cross-shard attribution (EXACT = true; never a group): the global-id arithmetic,
// the record pushes and the pool walks are compiled into that instantiation alone -- an unsharded engine's kernels do not carry a
// single instruction of them (they cost a HUS day 0.6 us while they were runtime branches on cold code).  The kernels hand
// their parameter pointer on as ParamsX<EXACT>: the helpers that care are templates on its type, all others take the plain pointer.
#define DAY_KERNEL template <bool GROUP, bool EXACT = false> __global__
// (a group's member array is written when the group is made and never by a kernel: its element is read through the CONSTANT address
// space -- scalar loads the compiler may place where the values are used, like a single engine's kernel arguments, instead of global
// loads at the kernel's head whose results it must keep alive, and spill, to the end: round-5 verdict, k_hosp_install<GROUP>'s scratch)
// (generic in the element: the tree reports keep a table of their own, k_transmission.inc's TxMember)
template <class T>
__device__ __forceinline__ void member_from_constant(T *out, const T *m) {
    static_assert(sizeof(T) % 8 == 0, "copied as 64-bit words");
    const CAS uint64_t *s = (const CAS uint64_t *)m;
    uint64_t *d = reinterpret_cast<uint64_t *>(out);
#pragma unroll
    for (size_t k = 0; k < sizeof(T) / 8; k++) d[k] = s[k];
}
#define MEMBER_OF_LAUNCH                                       \
    MemberRef mref_g_;                                         \
    if (GROUP) member_from_constant(&mref_g_, M_ + blockIdx.y); \
    const MemberRef &mref_ = GROUP ? mref_g_ : one_

static_assert(sizeof(reina_cold_t) == 32, "one sector per agent");
static_assert(REINA_L_SORT_TICKET < REINA_L_VACC_CURSOR && REINA_L_VACC_CURSOR + REINA_MAX_VACCINATIONS <= REINA_L_DET_SIDE && REINA_L_DET_SIDE + REINA_MAX_AGES <= REINA_L_NR,
              "named control words, then the vaccination cursors");
static thread_local std::string g_last_error;
static std::atomic<int> g_live_engines{0};   // engines of this process (reina_create .. reina_destroy): who may take the one-launch day (reina_hip.hip)

// The texts these two build from the spelled-out expression (#x) are no part of the library's contract: they change whenever
// an expression moves.  A refusal with a text of its own goes through refuse, below.
#define HIP_CHECK(x)                                                                         \
    do {                                                                                     \
        hipError_t _e = (x);                                                                 \
        if (_e != hipSuccess) {                                                              \
            g_last_error = std::string(#x) + ": " + hipGetErrorString(_e);                   \
            return REINA_E_HIP;                                                              \
        }                                                                                    \
    } while (0)
#define HIP_CHECK_OR(x, cleanup)                                                             \
    do {                                                                                     \
        hipError_t _e = (x);                                                                 \
        if (_e != hipSuccess) {                                                              \
            g_last_error = std::string(#x) + ": " + hipGetErrorString(_e);                   \
            cleanup;                                                                         \
            return REINA_E_HIP;                                                              \
        }                                                                                    \
    } while (0)

// the one way an entry point refuses: the text reina_last_error() gives, and the code
static int refuse(const std::string &text, int code = REINA_E_INVALID) {
    g_last_error = text;
    return code;
}

// A ring of page-locked blocks of one size, each with the event recorded behind the copy kernel that reads it: what the host
// writes into a block travels as an ordinary dispatch of the stream, queued behind the work already issued without stalling
// the host (a pageable source would drain the stream first).  A block is taken again once its copy has left it; while the
// host runs far ahead of the GPU new blocks are added instead of waiting, up to the caller's cap, and from then on the host
// waits for block 0.  What is written into a block, and which kernel reads it, is the caller's.
struct StageRing {
    std::vector<void *> host;   // hipHostMalloc'd, one a slot
    std::vector<hipEvent_t> ev;
    size_t slot = 0;            // the slot acquire handed out last

    int acquire(size_t bytes_per_slot, size_t cap, void **host_ptr, void **device_ptr) {
        slot = host.size();
        for (size_t k = 0; k < host.size(); k++)
            if (hipEventQuery(ev[k]) == hipSuccess) {
                slot = k;
                break;
            }
        if (slot == host.size()) {
            if (host.size() < cap) {
                void *block = nullptr;
                hipEvent_t e;
                HIP_CHECK(hipHostMalloc(&block, bytes_per_slot, hipHostMallocDefault));
                HIP_CHECK_OR(hipEventCreateWithFlags(&e, hipEventDisableTiming), (void)hipHostFree(block));
                host.push_back(block);
                ev.push_back(e);
            } else {
                slot = 0;
                HIP_CHECK(hipEventSynchronize(ev[0]));
            }
        }
        *host_ptr = host[slot];
        HIP_CHECK(hipHostGetDevicePointer(device_ptr, host[slot], 0));
        return REINA_OK;
    }
    // behind the launch that reads the slot
    int release_behind(hipStream_t s) {
        HIP_CHECK(hipEventRecord(ev[slot], s));
        return REINA_OK;
    }
    // teardown: every copy has left its block before the block goes
    void free() {
        for (size_t k = 0; k < host.size(); k++) {
            (void)hipEventSynchronize(ev[k]);
            (void)hipEventDestroy(ev[k]);
            (void)hipHostFree(host[k]);
        }
        host.clear();
        ev.clear();
    }
};

struct reina_engine {
    int32_t init_beds = -1;   // hospital beds passed to reina_init_state (reina_set_initial_state's precondition)
    reina_config_t cfg;
    reina_buffers_t buf;
    bool bound = false;
    DevParams *d_params = nullptr;
    Tables *d_tables = nullptr;
    MemberRef *d_ref = nullptr;   // {d_params, d_tables, buf, no history base}: k_init / k_initial_state find the engine through it
    MemberRef h_ref;              // the same on the host: a single engine's day kernels take it by value
    DevParams h_params;
    Tables h_tables;
    struct Stage { DevParams p; Tables t; };
    static constexpr size_t MAX_STAGES = 32;
    StageRing stage;                        // table uploads (stage_upload): blocks of one Stage
    reina_allreduce_fn coll_fn = nullptr;   // in-stream pressure all-reduce (reina_set_collective)
    void *coll_comm = nullptr;
    reina_alltoall_fn a2a_fn = nullptr;     // in-stream record exchange of exact attribution (reina_set_alltoall)
    void *a2a_comm = nullptr;
    bool exact = false;                     // exact cross-shard attribution (cfg.exact_attribution of a sharded population)
    uint32_t n_cus = 256;                   // compute units of the device (MI355X: 256)
    bool vacc_one_wg = false;               // REINA_VACC_ONE_WG: k_vaccinate as one workgroup whatever the day's number
    bool no_place_groups = false;           // REINA_NO_PLACE_GROUPS: the tables' place groups are declared unusable (the tests' handle on k_day's full entry search for every contact)
    uint32_t lds_rows_cap = 0;              // REINA_LDS_ROWS_CAP: at most that many contact / count rows staged in LDS (the tests' handle on the rows read through L2); 0: no cap
    uint32_t walk_div = 16;                 // buckets of the ordered bed / ICU walk per walking workgroup of the install launch (REINA_WALK_DIV: measurement handle)
    uint32_t import_wgs = 16;               // most workgroups a day's imports are shared by (REINA_IMPORT_WGS: the tests' handle on the chunked paths)
    bool testing_ever = false;
    uint32_t *d_snap = nullptr;             // snapshots (k_snapshot.inc): per-tile record counts, then their exclusive offsets, of both streams
    uint32_t snap_total[2] = {0, 0};        // ... records of both streams as the last reina_snap_measure found them
    uint32_t snap_qlen[3] = {0, 0, 0};      // ... and the lengths of queue0 / queue1 / level1
    bool fused_day = false;                 // stretches of days of a small unsharded population as ONE launch (k_small.inc; REINA_FUSED_DAY=1: measured SLOWER than the three launches a day, kept behind the switch with its tests)
    uint32_t small_wgs = 32;                // ... its workgroups (REINA_FUSED_WGS)
    uint32_t *d_bar = nullptr;              // ... its barrier counter, and the barriers passed so far
    uint32_t bar_epoch = 0;
    struct SmallDayRec *d_days = nullptr;   // ... the records of the stretch being run (device), their pinned staging ring
    StageRing days_stage;
    std::vector<uint32_t> small_pair_days;  // ... days of every timed k_small_days launch (beside kpairs[REINA_PK_SMALL_DAY])
    size_t small_static_lds = 0;            // ... the static LDS of k_small_day (its three phases' functions)
    bool counted_live = false;
    uint32_t vacc_seq = 0;                  // tag of the last k_vaccinate launch (drawn from a process-wide counter: reina_hip.hip), carried by the words its chained workgroups publish
    int day_mode = 0;                       // the form of k_day's stream: 0 by population size (sparse from DAY_SPARSE_MIN_TILES tiles per wave on), REINA_DAY_MODE: 1 dense, 2 sparse, 3 alternating by day
    bool open_tickets = false;              // k_open's roles by arrival ticket even for a single engine (REINA_OPEN_TICKETS: the tests)
    bool imports_in_open = false;           // weekly imports placed by the day's opening launch (rounds 1-3) instead of beside the stream
    uint32_t day_flags = 0;                 // k_day's measurement switches (REINA_DAY_FLAGS), 0 in production
    bool export_by_copies = false;          // REINA_EXPORT=memcpy: reina_read_history by two copies even into page-locked memory (measurement handle)
    uint32_t exchange_words = REINA_PRESSURE_WORDS;   // int32 words of buffers.pressure a sharded population all-reduces per day
    uint32_t group_lds_rows = 0, group_lds_crows = 0;   // representative of a group: the most distinct contact / count rows any member holds (LDS sizing)
    uint32_t policy_lds_rows = 0, policy_lds_crows = 0;   // during a policy run (k_policy.inc): the most rows of any level of the bank -- the host does not know a member's level; 0 otherwise
    // (running independent kernels of a day on a second stream was measured on MI355X / ROCm 7.2:
    // the cross-stream event waits cost more than the overlap wins back -- HUS 0.108 -> 0.127 ms/day,
    // 50 M agents 0.315 -> 0.311 -- so independent phases share ONE launch instead: k_hosp_contacts)
    // profiling (reina_profile_enable / reina_profile_read_kernels)
    bool profile = false;
    bool profile_day_only = false;   // reina_profile_enable(-k): only k_day is timed (every k-th day)
    uint32_t profile_stride = 1;  // stride > 1: on day % stride == 0, /4, /2, 3/4 one kind of kernel is timed
    static constexpr size_t MAX_EVENTS = 16384;   // pool cap: launches beyond it go untimed until the next read
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    std::vector<std::pair<size_t, size_t>> kpairs[REINA_PK_NR];
    double k_ms[REINA_PK_NR] = {0};
    uint64_t k_launches[REINA_PK_NR] = {0};
};

// ---------------------------------------------------------------------------------------------
// small device helpers

__device__ __forceinline__ int lane_id() { return (int)__lane_id(); }

// One slot per calling lane from a global counter, one atomic per wave (ballot + popcount).
__device__ __forceinline__ uint32_t wave_alloc(GAS int32_t *ctr) {
    uint64_t m = __ballot(1);
    uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull));
    uint32_t base = 0;
    if (rank == 0) base = (uint32_t)atomicAdd(ctr, (int)__popcll(m));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    return base + rank;
}

__device__ __forceinline__ void set_problem(GAS int32_t *counters, int p) {
    atomicCAS(&counters[SC_IDX(REINA_S_PROBLEM)], 0, p);
}

// age of sorted agent index i; `as` = age_start (LDS or global), search within [lo, hi]
__device__ __forceinline__ int age_of(const int32_t *as, uint32_t i, int lo, int hi) {
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if ((uint32_t)as[mid] <= i)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ int age_of(const CAS int32_t *as, uint32_t i, int lo, int hi) {
    while (lo < hi) {
        int mid = (lo + hi + 1) >> 1;
        if ((uint32_t)as[mid] <= i)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ uint32_t ld_hot(const GAS uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t ld_claim(const GAS uint64_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the per-agent bit planes (include/reina_hip.h: reina_buffers_t.active_bits / infected_bits)
__device__ __forceinline__ void agent_bit_set(GAS uint32_t *plane, uint32_t i) {
    __hip_atomic_fetch_or(&plane[i >> 5], 1u << (i & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void agent_bit_clear(GAS uint32_t *plane, uint32_t i) {
    __hip_atomic_fetch_and(&plane[i >> 5], ~(1u << (i & 31u)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ bool agent_bit(const GAS uint32_t *plane, uint32_t i) { return (plane[i >> 5] >> (i & 31u)) & 1u; }

// Disease.get_symptom_severity (main.pyx:1042-1091) in float32; both FATAL branches are
// DEATH_OUTSIDE_HOSPITAL (quirk Q2); variant-0 tables (quirk Q3)
__device__ int severity_of(const CAS reina_disease_t &d, int age, float val, float vmod, int *pod_outside) {
    float syc = d.p_symptomatic[age];
    *pod_outside = 0;
    if (val >= syc) return RV_ASYMPTOMATIC;
    syc *= vmod;
    float dohc = d.p_death_outside_hospital[age];
    if (dohc != 0.0f) {
        if (val < dohc * syc) {
            *pod_outside = 1;
            return RV_FATAL;
        }
        val = (val - dohc) / (1.0f - dohc);
    }
    float sc = d.p_severe_given_symptomatic[age];
    float cc = d.p_critical_given_severe[age];
    float fc = d.p_fatal_given_critical[age];
    if (val < fc * cc * sc * syc) {
        *pod_outside = 1;
        return RV_FATAL;
    }
    if (val < cc * sc * syc) return RV_CRITICAL;
    if (val < sc * syc) return RV_SEVERE;
    return RV_MILD;
}

__device__ __forceinline__ uint32_t clamp_days(GAS int32_t *counters, int d) {
    if (d < 0) d = 0;
    if (d > RH_MAX_DAYS) {
        set_problem(counters, REINA_PROBLEM_DAYS_OVERFLOW);
        d = RH_MAX_DAYS;
    }
    return (uint32_t)d;
}

// ---------------------------------------------------------------------------------------------
// exact cross-shard attribution: global ids and the exchange segments (include/reina_hip.h)
// the parameter pointer with the launch's attribution mode in its TYPE (DAY_KERNEL): a plain pointer means "no global ids"
template <bool X>
struct ParamsX {
    const CAS DevParams *p;
    __device__ __forceinline__ const CAS DevParams *operator->() const { return p; }
    __device__ __forceinline__ operator const CAS DevParams *() const { return p; }
};
__device__ __forceinline__ constexpr bool px_exact(const CAS DevParams *) { return false; }
template <bool X> __device__ __forceinline__ constexpr bool px_exact(ParamsX<X>) { return X; }
#define IS_EXACT(P) px_exact(P)
template <class PT> __device__ __forceinline__ int32_t gid_of(PT P, uint32_t i) { return IS_EXACT(P) ? (int32_t)(P->gid_base | i) : (int32_t)i; }
template <class PT> __device__ __forceinline__ bool gid_local(PT P, int32_t g) { return IS_EXACT(P) ? rp_gid_is_local((uint32_t)g, P->gid_base, P->gid_mask) != 0u : true; }
template <class PT> __device__ __forceinline__ uint32_t gid_index(PT P, int32_t g) { return IS_EXACT(P) ? (uint32_t)g & P->gid_mask : (uint32_t)g; }
__device__ __forceinline__ GAS uint64_t *xseg(const CAS DevParams *P, GAS uint64_t *buf, uint32_t shard) {
    return buf + (size_t)shard * (size_t)P->xchg_stride;
}
// the trailer of a segment: what rides behind the records of the mid-day exchange (include/reina_hip.h: REINA_XCHG_TRAILER_WORDS)
__device__ __forceinline__ GAS uint64_t *xtrailer(const CAS DevParams *P, GAS uint64_t *buf, uint32_t shard) {
    return xseg(P, buf, shard) + 1u + P->xchg_cap;
}
// one record for shard `dest`, from any subset of a wave's lanes at once: the lanes bound for the same shard take their slots
// with ONE returning atomic on that segment's count word (a returning atomic per lane was tried first: the records of a peak day
// at 2 x 5 x 10^7 agents, all on one count word, serialised in L2 to 1 ms of k_day and 0.8 ms of k_hosp_install -- an atomic
// holds its line for some 12 ns, tools/ubench_atomics.hip); the groups are found with ballots alone, their atomics go out
// together: one round trip whatever the number of shards.  The run fails loudly when a segment is full.
__device__ __forceinline__ void xsend_push(const CAS DevParams *P, const GBuffers &B, uint32_t dest, uint64_t rec) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t lt = (1ull << lane) - 1ull;
    uint64_t rest = __ballot(1);   // the lanes that push together (the same value in all of them: they loop as one)
    uint32_t my_leader = lane, my_rank = 0, my_cnt = 1;
    while (rest) {
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)rest) - 1);
        const uint32_t d = (uint32_t)__builtin_amdgcn_readlane((int)dest, leader);
        const uint64_t same = __ballot(dest == d) & rest;
        if (dest == d) {
            my_leader = (uint32_t)leader;
            my_rank = (uint32_t)__popcll(same & lt);
            my_cnt = (uint32_t)__popcll(same);
        }
        rest &= ~same;
    }
    GAS uint64_t *seg = xseg(P, B.xsend, dest);
    uint32_t base = 0;
    if (lane == my_leader) base = (uint32_t)atomicAdd((GAS unsigned long long *)seg, (unsigned long long)my_cnt);
    base = (uint32_t)__shfl((int)base, (int)my_leader);
    const uint32_t pos = base + my_rank;
    if (pos < P->xchg_cap) seg[1u + pos] = rec;
    else set_problem(B.counters, REINA_PROBLEM_EXCHANGE_OVERFLOW);
}
__device__ __forceinline__ uint32_t xrecv_count(const CAS DevParams *P, const GBuffers &B, uint32_t shard) {
    const uint64_t n = xseg(P, B.xrecv, shard)[0];
    return n > P->xchg_cap ? P->xchg_cap : (uint32_t)n;
}
// the records all other shards sent in the last exchange, as ONE index space [0, total): prefix of the segments' counts
// in LDS (`pre`: REINA_MAX_SHARDS + 1 words, filled by thread 0; the caller puts a barrier behind it)
__device__ __forceinline__ void xrecv_prefix(const CAS DevParams *P, const GBuffers &B, uint32_t *pre) {
    if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (uint32_t sh = 0; sh < P->n_shards; sh++) {
            pre[sh] = acc;
            if (sh != P->shard_rank) acc += xrecv_count(P, B, sh);
        }
        pre[P->n_shards] = acc;
    }
}
__device__ __forceinline__ uint64_t xrecv_record(const CAS DevParams *P, const GBuffers &B, const uint32_t *pre, uint32_t idx, uint32_t *from) {
    uint32_t sh = 0;
    while (sh + 1u < P->n_shards && pre[sh + 1u] <= idx) sh++;
    *from = sh;
    return xseg(P, B.xrecv, sh)[1u + (idx - pre[sh])];
}
// the launch that has taken in an exchange's records empties the segments for the next one (stream order: the exchange
// that read xsend is complete, the next producer is a later launch)
__device__ __forceinline__ void xsend_reset(const CAS DevParams *P, const GBuffers &B) {
    if (blockIdx.x == 0 && threadIdx.x < P->n_shards) {
        GAS uint64_t *seg = xseg(P, B.xsend, threadIdx.x);
        const uint64_t n = seg[0];   // (how full the segment was: the run's peak says how close it came to the capacity)
        if (n) atomicMax(&B.control[REINA_L_XCHG_PEAK], (int)(n > 0x7FFFFFFFull ? 0x7FFFFFFF : n));
        seg[0] = 0ull;
    }
}

// the source's half of person_infect (main.pyx:219-233): other_people_infected++, and the infectee appended to its list.
// The source's infection count is also this infectee's RANK among them; while the source keeps an infectee list, ranks below
// REINA_INLINE_INFECTEES are slots of its inline block (one sector: contact tracing reads them in one access), the others go to
// the linked list -- threaded through the infectees' own records, or, when infectees may live on another shard (exact
// attribution), through nodes of the pool; a 65th infectee fails the whole simulation (TOO_MANY_INFECTEES).
// (a source that keeps no list -- every source while contact tracing is off, the epidemic's first wave in the default
// scenario -- is counted by an atomic that returns nothing: no round trip on the install's chain)
template <class PT>
__device__ __forceinline__ void source_gains_infectee(PT P, const GBuffers &B, uint32_t s, int32_t infectee, uint32_t src_has_list) {
    if (!src_has_list) {
        atomicAdd(&B.cold[s].n_infected, 1);
        return;
    }
    const int old = atomicAdd(&B.cold[s].n_infected, 1);
    if (old < REINA_INLINE_INFECTEES) {
        B.infectees[(size_t)s * REINA_INLINE_INFECTEES + (uint32_t)old] = infectee;
    } else if (old >= 64) {
        set_problem(B.counters, 1 /* TOO_MANY_INFECTEES */);
    } else if (IS_EXACT(P)) {
        const uint32_t node = (uint32_t)atomicAdd(&B.control[REINA_L_POOL], 1);
        if (node >= P->pool_cap) {
            set_problem(B.counters, REINA_PROBLEM_INFECTEE_POOL_OVERFLOW);
            return;
        }
        B.infectee_pool[2u * node] = (uint32_t)infectee;
        B.infectee_pool[2u * node + 1u] = (uint32_t)atomicExch(&B.cold[s].first_infectee, (int32_t)node);
    } else {
        B.cold[infectee].next_sibling = atomicExch(&B.cold[s].first_infectee, infectee);
    }
}

// person_infect (main.pyx:209-235) + Population.infect (:1576-1582).  `expect` is the susceptible
// word the caller saw; the CAS makes duplicate winner records install once.
// `src_has_list`: the source keeps an infectee list (it was infected while contact tracing was on and had not
// been removed when it made the contact: its start-of-day word, carried in the candidate record).
// `vacc_day`: the target's day of vaccination (its cold record; the caller requests it beside the claim it checks -- same
// sector -- so that no round trip of its own is spent on it).  `exclusive`: the caller OWNS the target (an import that
// holds its claim): the word is stored, not compare-and-swapped.
template <class PT>
__device__ bool install_infection(PT P, const GBuffers &B, const int32_t *age_start, uint32_t t, uint32_t expect,
                                  uint32_t day, uint32_t variant, int32_t src, int fresh,
                                  uint32_t testing_mode, int32_t *new_by_age, int32_t *new_by_variant,
                                  uint32_t src_has_list, int32_t vacc_day, bool exclusive = false, bool by_bit = false) {
    int age = age_of(age_start, t, 0, (int)P->nr_ages - 1);
    rp_u4 r = rp_philox(P->k0, P->k1, t, day, RP_P_INFECT, 0);
    float val = rp_uniform24(r.v[0]);
    float vmod = 1.0f;
    if ((expect & RH_VACCINATED) && ((int)day - vacc_day > 14)) vmod = 0.1f;
    int pod = 0;
    int sev = severity_of(P->dis, age, val, vmod, &pod);
    float g = rp_gamma_mu_cv(P->dis.mean_incubation_duration[0], 0.86f, P->k0, P->k1, t, day, RP_P_INFECT, 1);
    uint32_t dl = clamp_days(B.counters, rp_round_to_int(g));
    uint32_t nw = RS_INCUBATION | ((uint32_t)sev << 3) | (variant << 8) | (pod ? RH_POD_OUTSIDE : 0u) |
                  (expect & (RH_VACCINATED | RH_DETECTED)) |   // (was_detected outlives a re-infection: set_initial_state only)
                  (testing_mode == RT_ALL_WITH_SYMPTOMS_CT ? RH_HASLIST : 0u) | RH_ACTIVE |
                  // (a FRESH agent of the initial condition sits out the scan of day 0 first)
                  RH_DAYS_FIELD(dl, (fresh && day == RP_INIT_DAY) ? day + 1u : day) |
                  RH_INFECTED_ON((fresh && day == RP_INIT_DAY) ? day + 1u : day);
    // the two bit planes beside the hot words (include/reina_hip.h: active_bits, infected_bits): the agent has something to
    // do in the daily stream from now on, and is no longer a target (fire-and-forget atomics: nobody reads the planes in
    // the launches that install infections)
    if (by_bit) {
        // `by_bit` (round 5: a contact's winner, whose target was never infected before): the agent's bit of the infected plane IS
        // the claim -- the atomic that sets it returns whether somebody (a duplicate record of the same winner) set it before --
        // and the word is stored plainly: one atomic and one fetched line less per infection than compare-and-swap + bit
        const uint32_t bit = 1u << (t & 31u);
        if (__hip_atomic_fetch_or(&B.infected_bits[t >> 5], bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) return false;
        B.hot[t] = nw;
    } else {
        if (exclusive) B.hot[t] = nw;
        else if (atomicCAS(&B.hot[t], expect, nw) != expect) return false;
        agent_bit_set(B.infected_bits, t);
    }
    agent_bit_set(B.active_bits, t);
    if (src >= 0) {
        // `src` is a global id when the population keeps them (exact attribution): the source's own shard counts the
        // infection and keeps the infectee list -- this one at once, another one when the day's feedback records arrive
        B.cold[t].infector = src;
        if (gid_local(P, src))
            source_gains_infectee(P, B, gid_index(P, src), gid_of(P, t), src_has_list);
        else if (IS_EXACT(P))
            xsend_push(P, B, rp_gid_shard((uint32_t)src), rp_xrec(gid_index(P, src), src_has_list << 2, (uint32_t)gid_of(P, t)));
    }
    atomicAdd(&new_by_age[age], 1);          // workgroup-local (LDS) histograms,
    atomicAdd(&new_by_variant[variant], 1);  // flushed once per workgroup by flush_new_infections
    return true;
}

// Population.infect counters (main.pyx:1576-1582) for a workgroup's worth of new infections
// (`with_infected` false: the caller adds the new infections to REINA_C_INFECTED itself, with its other changes of that row)
__device__ void flush_new_infections(const GBuffers &B, int32_t *new_by_age, int32_t *new_by_variant,
                                     int nthreads, bool with_infected = true) {
    __syncthreads();
    for (int k = threadIdx.x; k < REINA_MAX_AGES; k += nthreads) {
        int32_t v = new_by_age[k];
        if (v) {
            atomicAdd(&B.counters[CNT_IDX(REINA_C_SUSCEPTIBLE, k)], -v);
            if (with_infected) atomicAdd(&B.counters[CNT_IDX(REINA_C_INFECTED, k)], v);
            atomicAdd(&B.counters[CNT_IDX(REINA_C_ALL_INFECTED, k)], v);
            atomicAdd(&B.counters[CNT_IDX(REINA_C_NEW_INFECTIONS, k)], v);
            new_by_age[k] = 0;
        }
    }
    if (threadIdx.x < REINA_MAX_VARIANTS) {
        int32_t v = new_by_variant[threadIdx.x];
        if (v) atomicAdd(&B.counters[SC_IDX(REINA_S_INFECTED_BY_VARIANT + threadIdx.x)], v);
        new_by_variant[threadIdx.x] = 0;
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------------------------
// The day's events live in BUCKETS by priority range (buffers.hosp_events): the stream (k_day) gives every event
// its key [priority:20][agent:32][type:2] -- priority = Philox(agent, day): the order in which a scarce bed or ICU
// unit is handed out, the reference's rotated scan order over shuffled agents (main.pyx:1982-1992) -- and appends
// it to the bucket of the key's top bits.  Buckets are therefore in priority order among themselves; sorting each
// one sorts the day.  Layout (64-bit words): [R/2: the R bucket counts, uint32][2R: the first R = each bucket's composed
// saturating maps as published by its walker (k_hospital.inc: sat_pack), the rest unused][R * C: keys].  R and C depend on the population size only (DevParams).
#define HOSP_AGG_OFF(R) ((R) / 2)
#define HOSP_KEYS_OFF(R) ((R) / 2 + 2 * (R))
__device__ __forceinline__ GAS uint32_t *hosp_counts(const GBuffers &B) { return reinterpret_cast<GAS uint32_t *>(B.hosp_events); }
__device__ __forceinline__ GAS uint64_t *hosp_bucket(const CAS DevParams *P, const GBuffers &B, uint32_t r) {
    return B.hosp_events + HOSP_KEYS_OFF(P->hosp_ranges) + (size_t)r * P->hosp_bucket_cap;
}

// k_day: one event of agent i (person_hospitalize / transfer_to_icu / release, main.pyx:321-367) goes to its bucket
// A wave-uniform value the compiler takes as it is: not re-derived from memory where it is used (a scalar load and a wait in the
// middle of a loop), and nothing computed from it hoisted out of the loops around it (Philox round keys that end up spilled).
__device__ __forceinline__ uint32_t opaque_s(uint32_t x) {
    asm volatile("" : "+s"(x));
    return x;
}
// Loads the compiler keeps no books on, waited for at once: the rare reads through L2 inside k_day's loops (contact rows beyond the
// LDS image, per-age meta words, the variants' mask parameters).  As ordinary loads they cost the COMMON path: wherever a path with
// such a load meets one without, the compiler waits for "the load" with s_waitcnt vmcnt(0) -- i.e. for every vector-memory operation
// the wave has in flight, the stream's fetch and the targets' gather among them (measured: the head of every batch and of every
// resolve step).
__device__ __forceinline__ uint32_t ld_u32_now(uint64_t addr) {
    uint32_t v;
    asm volatile("global_load_dword %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
__device__ __forceinline__ uint32_t ld_u8_now(uint64_t addr) {
    uint32_t v;
    asm volatile("global_load_ubyte %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
#define LD_U32_NOW(lvalue) ld_u32_now((uint64_t)&(lvalue))
#define LD_U8_NOW(lvalue) ld_u8_now((uint64_t)&(lvalue))
#define LD_F32_NOW(lvalue) rp_u2f(ld_u32_now((uint64_t)&(lvalue)))
__device__ __forceinline__ uint64_t hosp_event_key(const CAS DevParams *P, uint32_t i, uint32_t kind, uint32_t day) {
    const uint32_t prio = rp_priority20(opaque_s(P->k0), opaque_s(P->k1), i, day);
    return ((uint64_t)prio << 34) | ((uint64_t)i << 2) | (uint64_t)(kind & 3u);
}
__device__ __forceinline__ void hosp_push_key(const CAS DevParams *P, const GBuffers &B, uint64_t key) {
    const uint32_t r = (uint32_t)(key >> 34) >> (20u - P->hosp_range_bits);
    const uint32_t pos = atomicAdd(&hosp_counts(B)[r], 1u);
    if (pos < P->hosp_bucket_cap)
        hosp_bucket(P, B, r)[pos] = key;
    else
        set_problem(B.counters, REINA_PROBLEM_HOSPITAL_OVERFLOW);
}
// ... by way of the workgroup's stage in LDS (`stage_n`, `stage_key`: DAY_EV_STAGE entries, flushed when k_day's stream is
// through): one LDS atomic per wave step instead of a returning global atomic per event in the middle of the step; an
// event that finds the stage full goes to its bucket at once.  All lanes of the wave call together.
__device__ __forceinline__ void hosp_stage_event(const CAS DevParams *P, const GBuffers &B, bool pred, uint32_t i, uint32_t kind, uint32_t day,
                                                 uint32_t *stage_n, unsigned long long *stage_key, uint32_t stage_cap) {
    const uint64_t m = __ballot(pred);
    if (!m) return;
    uint32_t base = 0;
    if (stage_cap) {
        if ((uint32_t)lane_id() == (uint32_t)__ffsll((unsigned long long)m) - 1u) base = atomicAdd(stage_n, (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, __ffsll((unsigned long long)m) - 1);
    }
    if (pred) {
        const uint64_t key = hosp_event_key(P, i, kind, day);
        const uint32_t pos = base + (uint32_t)__popcll(m & ((1ull << lane_id()) - 1ull));
        if (pos < stage_cap) stage_key[pos] = key;
        else hosp_push_key(P, B, key);
    }
}

// The test-queue and weekly-import workgroups share the launch of the day's opening workgroup
// (k_open): before they add to the counters they wait here until it has taken the history snapshot
// and zeroed the daily counters.  Roles are handed out by an arrival TICKET (k_open), so the opening
// workgroup is by construction one that is already running when any other workgroup starts to wait:
// no assumption about the order in which the dispatcher starts workgroups (HIP promises none).
// The wait is bounded by a POLL COUNT (about 4 s of polling; not wall time, which keeps running
// while a process's waves are switched out): a workgroup that gives up flags the day failed
// (REINA_PROBLEM_SYNC_TIMEOUT) and returns false -- its caller then leaves the counters alone.
__device__ __forceinline__ bool wait_day_open(const GBuffers &B, uint32_t day) {
    __shared__ int s_open_ok;
    if (threadIdx.x == 0) {
        // poll with relaxed loads (an acquire per poll would invalidate this CU's caches every time);
        // one acquire fence once the value is there
        int ok = 1;
        uint32_t polls = 0;
        while (__hip_atomic_load(&B.control[REINA_L_DAY_OPEN], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != (int32_t)day + 1) {
            __builtin_amdgcn_s_sleep(8);
            if (++polls > (1u << 22)) {
                set_problem(B.counters, REINA_PROBLEM_SYNC_TIMEOUT);
                ok = 0;
                break;
            }
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        s_open_ok = ok;
    }
    __syncthreads();
    return s_open_ok != 0;
}
