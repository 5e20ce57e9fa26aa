// The diagnostic builds of the day kernels in one place: where their in-kernel stamps and profile rows go (the slot map), the one
// stamp that writes them, the names of REINA_DAY_PROF's parts and of REINA_ABLATE's bits.  Included by k_common.inc; tools/diag.py
// builds the variants and reads them back through reina_diag_describe -- no word offset is written anywhere else.
//
// The switches (hipcc -D..., reina_model_amd/build.py: build_variant; none of them in the production library):
//   REINA_OPEN_STAMPS / _HOSP_STAMPS / _INSTALL_STAMPS / _DAY_STAMPS / _SMALL_STAMPS   wall-clock stamps (100 MHz ticks) of a kernel's phases
//   REINA_DAY_PROF=<part>   every wave of k_day times ONE part of its loop beside the whole loop (shader-clock cycles)
//   REINA_ABLATE            parts of k_day switched off at run time (reina_debug_ablate), for timing only
// All of them write buffers.mirror, which is scratch only in an unsharded engine (a sharded one keeps the mirror tables there):
// reina_create refuses a sharded engine in a library built with any of them.
//
// The map part (down to "device part") is plain C++: tests/test_diag_map.py compiles it alone with every switch defined.
// A NEW STAMP IS A LINE IN THE MAP: a DIAG_PHASES line, its region's length in DIAG_REGIONS, and the call where the phase ends.
#ifndef REINA_DIAG_H
#define REINA_DIAG_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

// buffers.mirror of an unsharded engine, 64-bit words (reina_model_amd/engine.py: DIAG_MIRROR_WORDS)
#define DIAG_MIRROR_WORDS (64 + 4 * 8192)
#define DIAG_ROW_WORDS 4
// what a word holds: ticks summed over the stampers / the longest ever / how many stamped; a ROWS region is one row of
// DIAG_ROW_WORDS plain stores per wave of k_day, its phases are the row's words
enum { DIAG_SUM = 1, DIAG_MAX = 2, DIAG_COUNT = 4, DIAG_ROWS = 8 };

#ifdef REINA_OPEN_STAMPS
#define DIAG_ON_OPEN 1
#else
#define DIAG_ON_OPEN 0
#endif
#define DIAG_ON_TRACE DIAG_ON_OPEN
#define DIAG_ON_WAVES DIAG_ON_PROF
#define DIAG_ON_IMPORTS DIAG_ON_OPEN
#ifdef REINA_HOSP_STAMPS
#define DIAG_ON_HOSP 1
#else
#define DIAG_ON_HOSP 0
#endif
#ifdef REINA_INSTALL_STAMPS
#define DIAG_ON_INSTALL 1
#else
#define DIAG_ON_INSTALL 0
#endif
#ifdef REINA_DAY_STAMPS
#define DIAG_ON_DAY 1
#else
#define DIAG_ON_DAY 0
#endif
#ifdef REINA_SMALL_STAMPS
#define DIAG_ON_SMALL 1
#else
#define DIAG_ON_SMALL 0
#endif
#ifdef REINA_DAY_PROF
#define DIAG_ON_PROF 1
#define DIAG_PROF_PART (REINA_DAY_PROF)
#else
#define DIAG_ON_PROF 0
#define DIAG_PROF_PART (-1)
#endif
#ifdef REINA_ABLATE
#define DIAG_ON_ABLATE 1
#else
#define DIAG_ON_ABLATE 0
#endif
#if DIAG_ON_OPEN || DIAG_ON_HOSP || DIAG_ON_INSTALL || DIAG_ON_DAY || DIAG_ON_SMALL || DIAG_ON_PROF || DIAG_ON_ABLATE
#define DIAG_ANY 1
#endif

// ---- the slot map ------------------------------------------------------------------------------------------------------------
// R(region, the switch that writes it, first word, words): in ascending order, disjoint whatever the switches (asserted below)
#define DIAG_REGIONS(R)                                                                                                       \
    R(OPEN, REINA_OPEN_STAMPS, 0, 15)       /* k_open's roles: the opening workgroup, the weekly imports', the test queue's */   \
    R(TRACE, REINA_OPEN_STAMPS, 15, 8)      /* the tracing waves: the slowest wave's way through an entry of its list */         \
    R(IMPORTS, REINA_OPEN_STAMPS, 23, 9)    /* the import placement (pro_imports) of the weekly-import workgroup */              \
    R(HOSP, REINA_HOSP_STAMPS, 32, 7)       /* the small ordered event walk (hospital_block) */                                  \
    R(INSTALL, REINA_INSTALL_STAMPS, 39, 12) /* install_block: the installing workgroups, the events-only workgroup */           \
    R(DAY, REINA_DAY_STAMPS, 51, 5)         /* k_day's workgroups */                                                             \
    R(SMALL, REINA_SMALL_STAMPS, 56, 13)    /* k_small_days' phases of a day */                                                  \
    R(WAVES, REINA_DAY_PROF, 72, DIAG_ROW_WORDS * 8190)   /* REINA_DAY_PROF: a row per wave of k_day (the first 8190 of at most 8192) */
// P(region, phase, kinds): a phase takes one word per kind, SUM then MAX then COUNT, behind the words of the phases above it
#define DIAG_PHASES(P)                                                                                                        \
    P(OPEN, UNTIL_FLAG, DIAG_SUM)           /* opening workgroup, since its first instruction: the day-open flag is set */       \
    P(OPEN, TOTAL, DIAG_SUM)                /* ... its weekly imports are placed */                                              \
    P(OPEN, WEEKLY, DIAG_SUM)               /* the weekly-import workgroup (helper 0), from its set-up to its end */             \
    P(OPEN, LEVEL0, DIAG_SUM | DIAG_MAX | DIAG_COUNT)       /* a test-queue workgroup: its level-0 loop and list appends */      \
    P(OPEN, DETECTIONS, DIAG_SUM | DIAG_MAX | DIAG_COUNT)   /* ... the day's detections to the side block */                     \
    P(OPEN, ARRIVAL, DIAG_SUM | DIAG_MAX | DIAG_COUNT)      /* ... the fence and the arrival count in front of level 1 */        \
    P(OPEN, LEVEL1, DIAG_SUM | DIAG_MAX | DIAG_COUNT)       /* ... the level-1 loop */                                           \
    P(TRACE, L0_ENTRY, DIAG_MAX)            /* level 0, since the block's first instruction: the queue entry is read */          \
    P(TRACE, L0_RECORD, DIAG_MAX)           /* ... its record, inline slots and word are in */                                   \
    P(TRACE, L0_FLAGS, DIAG_MAX)            /* ... the candidates' flags are set */                                              \
    P(TRACE, L0_OVERFLOW, DIAG_MAX)         /* ... the overflow list is walked */                                                \
    P(TRACE, L1_ENTRY, DIAG_MAX)                                                                                              \
    P(TRACE, L1_RECORD, DIAG_MAX)                                                                                             \
    P(TRACE, L1_FLAGS, DIAG_MAX)                                                                                              \
    P(TRACE, L1_OVERFLOW, DIAG_MAX)                                                                                           \
    P(IMPORTS, SETUP, DIAG_SUM)                                                                                               \
    P(IMPORTS, PROPOSE, DIAG_SUM)                                                                                             \
    P(IMPORTS, ANY_PROPOSED, DIAG_SUM)      /* the workgroups' vote behind the proposals */                                      \
    P(IMPORTS, VERIFY, DIAG_SUM)                                                                                              \
    P(IMPORTS, LEFT_ROUNDS, DIAG_SUM)       /* the vote that ended the rounds */                                                 \
    P(IMPORTS, INFECT, DIAG_SUM)                                                                                              \
    P(IMPORTS, TAIL, DIAG_SUM)                                                                                                \
    P(IMPORTS, WAIT_OPEN, DIAG_SUM)         /* the wait for the opening workgroup's daily zeroing */                             \
    P(IMPORTS, FLUSH, DIAG_SUM)                                                                                               \
    P(HOSP, GATHER, DIAG_SUM)               /* bucket counts, prefix, the day's keys into LDS */                                 \
    P(HOSP, SORT, DIAG_SUM)                                                                                                   \
    P(HOSP, DECIDE, DIAG_SUM)               /* the scan of saturating maps */                                                    \
    P(HOSP, APPLY, DIAG_SUM)                                                                                                  \
    P(HOSP, FLUSH, DIAG_SUM)                                                                                                  \
    P(HOSP, BLOCK, DIAG_SUM | DIAG_COUNT)   /* the whole walk, and the ordered days that had one */                              \
    P(INSTALL, MAIN_SETUP, DIAG_SUM | DIAG_MAX)                                                                               \
    P(INSTALL, MAIN_WORK, DIAG_SUM | DIAG_MAX)                                                                                \
    P(INSTALL, MAIN_FLUSH, DIAG_SUM | DIAG_MAX)                                                                               \
    P(INSTALL, EVENTS_SETUP, DIAG_SUM | DIAG_MAX)                                                                             \
    P(INSTALL, EVENTS_WORK, DIAG_SUM | DIAG_MAX)                                                                              \
    P(INSTALL, EVENTS_FLUSH, DIAG_SUM | DIAG_MAX)                                                                             \
    P(DAY, STAGED, DIAG_SUM)                /* since the workgroup's first instruction: tables staged, the barrier passed */      \
    P(DAY, STREAM, DIAG_SUM)                /* ... thread 0's wave through its tiles and rounds */                               \
    P(DAY, RESOLVED, DIAG_SUM)              /* ... its last contacts resolved, its counts written */                             \
    P(DAY, BARRIER, DIAG_SUM | DIAG_COUNT)  /* ... the barrier before the counter flush; COUNT: workgroups */                    \
    P(SMALL, OPENING, DIAG_SUM | DIAG_MAX | DIAG_COUNT)   /* COUNT: workgroup-days */                                           \
    P(SMALL, BARRIER1, DIAG_SUM | DIAG_MAX)                                                                                   \
    P(SMALL, STREAM, DIAG_SUM | DIAG_MAX)                                                                                     \
    P(SMALL, BARRIER2, DIAG_SUM | DIAG_MAX)                                                                                   \
    P(SMALL, INSTALLS, DIAG_SUM | DIAG_MAX)                                                                                   \
    P(SMALL, BARRIER3, DIAG_SUM | DIAG_MAX)                                                                                   \
    P(WAVES, LOOP, DIAG_ROWS)                /* cycles of the wave's whole loop */                                                \
    P(WAVES, PART, DIAG_ROWS)                /* cycles of the timed part */                                                       \
    P(WAVES, PIECES, DIAG_ROWS)              /* how many times the part was entered */                                            \
    P(WAVES, WRITTEN, DIAG_ROWS)             /* 1: this wave wrote its row */
// the parts of k_day a -DREINA_DAY_PROF=<number> build times (PROF_BEGIN / PROF_END / PROF_IS in k_contacts.inc)
#define DIAG_PROF_PARTS(X)                                                                                                    \
    X(LOOP, 0)           /* the wave's whole loop: timed in every build */                                                      \
    X(FEED, 1)           /* finding the active agents (every form of the stream) */                                             \
    X(FETCH_WAIT, 2)     /* sparse: the wait for the fetched words */                                                           \
    X(BITS_WAIT, 3)      /* sparse: the wait for a chunk of bits */                                                             \
    X(ROUNDS, 4)         /* state-machine rounds */                                                                             \
    X(BATCHES, 5)        /* contact batches */                                                                                  \
    X(RESOLVE_TURNS, 6)  /* ... of which the resolve turns */                                                                   \
    X(TAIL, 7)           /* the last resolve behind the loop */                                                                 \
    X(BATCH_HEAD, 8)     /* a batch's head: counts, prefix, the sources' LDS rows */                                            \
    X(BATCH_STEPS, 9)    /* ... its steps of 64 contacts (pieces: steps) */                                                     \
    X(HEAD_DRAIN, 10)    /* the wave's memory operations in flight drained at the head of a batch */                            \
    X(HEAD_DRAINED, 11)  /* ... the head behind that drain */                                                                   \
    X(ROUND_DRAIN, 12)   /* what a state-machine round leaves in flight */                                                      \
    X(FEED_DRAIN, 13)    /* what the feeder left in flight */                                                                   \
    X(SPARSE_WORDS, 14)  /* sparse stage 1: fetched words -> queue */                                                           \
    X(SPARSE_BITS, 15)   /* sparse stage 2: bits -> agent numbers */                                                            \
    X(SPARSE_FETCH, 16)  /* sparse stage 3: the next fetch requested */                                                         \
    X(BIT_LANES, 17)     /* no cycles: iterations of the bit loop (pieces) and lanes that took a bit in them (part) */
// what reina_debug_ablate's bits switch off in k_day (the state that follows is meaningless)
#define DIAG_ABLATE_BITS(X)                                                                                                   \
    X(RESOLVE, 1)        /* no target resolution */                                                                             \
    X(COUNT_DRAW, 2)     /* no thresholds in the count draw */                                                                  \
    X(CONTACTS, 4)       /* no contact sampling at all */                                                                       \
    X(ACTIVE_CLEAR, 8)   /* no clearing of ACTIVE bits in the plane */                                                          \
    X(LIST_STORES, 16)   /* no list stores in the state-machine rounds */                                                       \
    X(HOT_STORE, 32)     /* no store of changed hot words */                                                                    \
    X(ONSET_STORE, 64)   /* no store of onset_days */                                                                           \
    X(EVENT_PUSH, 128)   /* no push of the staged bed / ICU events */

#define DIAG_R_ENUM(r, sw, first, words) DIAG_R_##r,
enum { DIAG_REGIONS(DIAG_R_ENUM) DIAG_N_REGIONS };
#define DIAG_P_ENUM(r, p, k) DIAG_##r##_##p,
enum { DIAG_PHASES(DIAG_P_ENUM) DIAG_N_PHASES };
#define DIAG_X_PROF(name, n) DIAG_PROF_##name = n,
enum { DIAG_PROF_PARTS(DIAG_X_PROF) };
#define DIAG_X_ABLATE(name, n) DIAG_ABLATE_##name = n##u,
enum : uint32_t { DIAG_ABLATE_BITS(DIAG_X_ABLATE) };

struct DiagRegion { const char *name, *sw; int first, words, on; };
struct DiagPhase { int region; const char *name; int kinds; };
struct DiagName { const char *name; int value; };
#define DIAG_R_ROW(r, sw, first, words) {#r, #sw, first, words, DIAG_ON_##r},
#define DIAG_P_ROW(r, p, k) {DIAG_R_##r, #p, k},
#define DIAG_X_ROW(name, n) {#name, n},
static constexpr DiagRegion DIAG_REGION_TABLE[] = {DIAG_REGIONS(DIAG_R_ROW)};
static constexpr DiagPhase DIAG_PHASE_TABLE[] = {DIAG_PHASES(DIAG_P_ROW)};
static constexpr DiagName DIAG_PROF_TABLE[] = {DIAG_PROF_PARTS(DIAG_X_ROW)};
static constexpr DiagName DIAG_ABLATE_TABLE[] = {DIAG_ABLATE_BITS(DIAG_X_ROW)};

constexpr int diag_kind_words(int kinds) { return (kinds & 1) + ((kinds >> 1) & 1) + ((kinds >> 2) & 1) + ((kinds >> 3) & 1); }
// the first word of a phase, and the word of one of its kinds
constexpr int diag_phase_word(int phase) {
    int w = DIAG_REGION_TABLE[DIAG_PHASE_TABLE[phase].region].first;
    for (int q = 0; q < phase; q++)
        if (DIAG_PHASE_TABLE[q].region == DIAG_PHASE_TABLE[phase].region) w += diag_kind_words(DIAG_PHASE_TABLE[q].kinds);
    return w;
}
constexpr int diag_phase_kinds(int phase) { return DIAG_PHASE_TABLE[phase].kinds; }
constexpr int diag_phase_region(int phase) { return DIAG_PHASE_TABLE[phase].region; }
constexpr int diag_kind_word(int phase, int kind) { return diag_phase_word(phase) + diag_kind_words(DIAG_PHASE_TABLE[phase].kinds & (kind - 1)); }
constexpr int diag_region_phase_words(int region) {
    int w = 0;
    for (int q = 0; q < DIAG_N_PHASES; q++)
        if (DIAG_PHASE_TABLE[q].region == region) w += diag_kind_words(DIAG_PHASE_TABLE[q].kinds);
    return w;
}
// every region begins where the one above it ends or later: no two share a word, whichever switches are defined
constexpr bool diag_regions_disjoint() {
    for (int r = 1; r < DIAG_N_REGIONS; r++)
        if (DIAG_REGION_TABLE[r].first < DIAG_REGION_TABLE[r - 1].first + DIAG_REGION_TABLE[r - 1].words) return false;
    return DIAG_REGION_TABLE[0].first >= 0;
}
// a region's phases fill it: word by word, or as the words of one row of a region of whole rows
constexpr bool diag_regions_filled() {
    for (int r = 0; r < DIAG_N_REGIONS; r++) {
        const bool rows = r == DIAG_R_WAVES;
        for (int q = 0; q < DIAG_N_PHASES; q++)
            if (DIAG_PHASE_TABLE[q].region == r && (DIAG_PHASE_TABLE[q].kinds == DIAG_ROWS) != rows) return false;
        if (rows ? diag_region_phase_words(r) != DIAG_ROW_WORDS || DIAG_REGION_TABLE[r].words % DIAG_ROW_WORDS || DIAG_REGION_TABLE[r].first % DIAG_ROW_WORDS
                 : diag_region_phase_words(r) != DIAG_REGION_TABLE[r].words)
            return false;
    }
    return true;
}
static_assert(diag_regions_disjoint(), "the regions of the slot map are listed in ascending order and share no word");
static_assert(diag_regions_filled(), "a region's length is the words of its phases (a ROWS region: whole rows of DIAG_ROW_WORDS, aligned)");
static_assert(DIAG_REGION_TABLE[DIAG_N_REGIONS - 1].first + DIAG_REGION_TABLE[DIAG_N_REGIONS - 1].words <= DIAG_MIRROR_WORDS,
              "the slot map ends inside buffers.mirror of an unsharded engine");
#define DIAG_WAVES_ROWS (DIAG_REGION_TABLE[DIAG_R_WAVES].words / DIAG_ROW_WORDS)

static inline const char *diag_kind_name(int kind) { return kind == DIAG_SUM ? "SUM" : kind == DIAG_MAX ? "MAX" : kind == DIAG_COUNT ? "COUNT" : "ROWS"; }
// the switches this translation unit was compiled with, as they stand on the command line
static inline size_t diag_switches(char *out, size_t cap) {
    return (size_t)snprintf(out, cap, "%s%s%s%s%s%s%s", DIAG_ON_OPEN ? " REINA_OPEN_STAMPS" : "", DIAG_ON_HOSP ? " REINA_HOSP_STAMPS" : "",
                            DIAG_ON_INSTALL ? " REINA_INSTALL_STAMPS" : "", DIAG_ON_DAY ? " REINA_DAY_STAMPS" : "", DIAG_ON_SMALL ? " REINA_SMALL_STAMPS" : "",
                            DIAG_ON_ABLATE ? " REINA_ABLATE" : "", DIAG_ON_PROF ? " REINA_DAY_PROF" : "");
}
// The map as text, one record a line (what reina_diag_describe returns; tools/diag.py and tests/test_diag_map.py parse it):
//   mirror <words> row <words of a row>
//   switches [<switch> ...]                  prof <part number, -1: none>
//   region <name> <switch> <first> <words> <1: this library writes it>
//   word <number> <region> <phase> <kind>    (a ROWS region: the word's place in the first row)
//   part <number> <name>                     bit <number> <name>
// Returns the length of the whole text; it is cut (and still terminated) where cap ends.
static inline size_t diag_describe(char *out, size_t cap) {
    size_t n = 0;
    char sw[160];
    diag_switches(sw, sizeof sw);
#define DIAG_PRINT(...) n += (size_t)snprintf(n < cap ? out + n : nullptr, n < cap ? cap - n : 0, __VA_ARGS__)
    DIAG_PRINT("mirror %d row %d\nswitches%s\nprof %d\n", DIAG_MIRROR_WORDS, DIAG_ROW_WORDS, sw, (int)DIAG_PROF_PART);
    for (int r = 0; r < DIAG_N_REGIONS; r++)
        DIAG_PRINT("region %s %s %d %d %d\n", DIAG_REGION_TABLE[r].name, DIAG_REGION_TABLE[r].sw, DIAG_REGION_TABLE[r].first, DIAG_REGION_TABLE[r].words,
                   DIAG_REGION_TABLE[r].on);
    for (int q = 0; q < DIAG_N_PHASES; q++)
        for (int kind = DIAG_SUM; kind <= DIAG_ROWS; kind <<= 1)
            if (DIAG_PHASE_TABLE[q].kinds & kind)
                DIAG_PRINT("word %d %s %s %s\n", diag_kind_word(q, kind), DIAG_REGION_TABLE[DIAG_PHASE_TABLE[q].region].name, DIAG_PHASE_TABLE[q].name,
                           diag_kind_name(kind));
    for (const DiagName &p : DIAG_PROF_TABLE) DIAG_PRINT("part %d %s\n", p.value, p.name);
    for (const DiagName &b : DIAG_ABLATE_TABLE) DIAG_PRINT("bit %d %s\n", b.value, b.name);
#undef DIAG_PRINT
    return n;
}

// ---- device part -------------------------------------------------------------------------------------------------------------
#ifdef __HIPCC__
#define DIAG_CAT_(a, b) a##b
#define DIAG_CAT(a, b) DIAG_CAT_(a, b)
#define DIAG_WHEN_0(...)
#define DIAG_WHEN_1(...) __VA_ARGS__
#define DIAG_WHEN(on) DIAG_CAT(DIAG_WHEN_, on)   // DIAG_WHEN(DIAG_ON_<region>)(code): the code, or nothing at all

// who stamps: thread 0 of the workgroup / lane 0 of every wave / thread 0 behind a __syncthreads() of the whole workgroup
enum { DIAG_THREAD0, DIAG_WAVE_LANE0, DIAG_BARRIER_THREAD0 };
// THE stamp: the time since `clock` -- the previous stamp (LAP: the clock moves on) or the block's first instruction -- goes to every
// word the map gives the phase: added to its SUM, atomicMax into its MAX, one more in its COUNT.
template <int REGION, int PHASE, int WHO, bool LAP>
__device__ __forceinline__ void diag_stamp(uint64_t *mirror, uint64_t &clock, bool when = true) {
    static_assert(diag_phase_region(PHASE) == REGION && !(diag_phase_kinds(PHASE) & DIAG_ROWS), "a phase of this region's, of SUM / MAX / COUNT words");
    constexpr int kinds = diag_phase_kinds(PHASE), word = diag_phase_word(PHASE);
    if (WHO == DIAG_BARRIER_THREAD0) __syncthreads();
    if ((WHO == DIAG_WAVE_LANE0 ? threadIdx.x & 63u : threadIdx.x) != 0u || !when) return;
    const uint64_t now = wall_clock64();
    unsigned long long *m = (unsigned long long *)mirror + word;
    if (kinds & DIAG_SUM) atomicAdd(m++, (unsigned long long)(now - clock));
    if (kinds & DIAG_MAX) atomicMax(m++, (unsigned long long)(now - clock));
    if (kinds & DIAG_COUNT) atomicAdd(m, 1ull);
    if (LAP) clock = now;
}
// (region, phase enumerator, who, the clock, buffers.mirror[, only when]): no code unless the region's switch is defined.  (The empty
// form is the empty statement the stamp macros of the kernel files left behind, not nothing: clang numbers a function's jump
// destinations through every do-while, and pro_imports carries such numbers as literals -- with it the production object is, kernel
// by kernel and instruction by instruction, what it was before this header: profiles/diag_frame_kernel_meta.txt.)
#define DIAG_CLOCK(R, name) DIAG_WHEN(DIAG_ON_##R)(uint64_t name = wall_clock64())
#define DIAG_LAP(R, PHASE, WHO, clock, mirror, ...) do { DIAG_WHEN(DIAG_ON_##R)(diag_stamp<DIAG_R_##R, PHASE, WHO, true>((uint64_t *)(mirror), clock, ##__VA_ARGS__);) } while (0)
#define DIAG_SINCE(R, PHASE, WHO, clock, mirror, ...) do { DIAG_WHEN(DIAG_ON_##R)(diag_stamp<DIAG_R_##R, PHASE, WHO, false>((uint64_t *)(mirror), clock, ##__VA_ARGS__);) } while (0)

// REINA_DAY_PROF: every wave of k_day sums the shader-clock cycles it spends in its whole loop and in ONE part of it (two 32-bit
// sums: anything more perturbs the kernel) and writes them as its row of the WAVES region when it is through.  The parts go by
// their names in DIAG_PROF_PARTS; a part that is not the build's costs nothing.
#define PROF_IS(part) (DIAG_PROF_PART == DIAG_PROF_##part)
#if DIAG_ON_PROF
#define PROF_NOW() ((uint32_t)__builtin_amdgcn_s_memtime())
#define PROF_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define PROF_DECL uint32_t prof_t_ = 0, prof_n_ = 0, prof_s_ = 0, prof_all_ = 0
#define PROF_BEGIN(part) do { if (PROF_IS(part) || DIAG_PROF_##part == DIAG_PROF_LOOP) { const uint32_t t_ = PROF_NOW(); if (DIAG_PROF_##part == DIAG_PROF_LOOP) prof_all_ = t_; else prof_s_ = t_; } } while (0)
#define PROF_END(part) do { if (PROF_IS(part)) { prof_t_ += PROF_NOW() - prof_s_; prof_n_++; } else if (DIAG_PROF_##part == DIAG_PROF_LOOP) prof_all_ = PROF_NOW() - prof_all_; } while (0)
// a part that exists only in its own build: everything the wave has in flight drained, and the wait timed
#define PROF_DRAINED(part) do { if (PROF_IS(part)) { PROF_BEGIN(part); PROF_DRAIN(); PROF_END(part); } } while (0)
#define PROF_TALLY(part, pieces, amount) do { if (PROF_IS(part)) { prof_n_ += (pieces); prof_t_ += (amount); } } while (0)
// the parts inside contact_batch, which has the wave's ContactState and not its loop's sums: C.prof_in / C.prof_in_n
#define PROF_IN_MEMBERS uint32_t prof_in, prof_in_n
#define PROF_IN_RESET(C) ((C).prof_in = (C).prof_in_n = 0)
#define PROF_IN_VAR(v) uint32_t v = 0
#define PROF_IN_MARK(v) (v = PROF_NOW())
#define PROF_IN_ADD(C, v, pieces) do { (C).prof_in += PROF_NOW() - (v); (C).prof_in_n += (pieces); } while (0)
#define PROF_IN_PARTS (PROF_IS(RESOLVE_TURNS) || PROF_IS(BATCH_HEAD) || PROF_IS(BATCH_STEPS) || PROF_IS(HEAD_DRAIN) || PROF_IS(HEAD_DRAINED))
// lane 0 writes the wave's row.  One row of plain stores per wave: sums by same-address atomics, as until round 4, took 8.5 ns
// each in L2 -- 140 us for a launch's 16 384, a quiet day's kernel measured at 160 us instead of 21, and every wave's stores
// queued behind them.  (A wave past the region's last row writes nothing.)
#define PROF_WRITE_ROW(mirror, wave, C)                                                                             \
    do {                                                                                                            \
        if (lane_id() == 0 && (wave) < (uint32_t)DIAG_WAVES_ROWS) {                                                 \
            if (PROF_IN_PARTS) { prof_t_ = (C).prof_in; prof_n_ = (C).prof_in_n; }                                  \
            constexpr int loop_ = diag_phase_word(DIAG_WAVES_LOOP), part_ = diag_phase_word(DIAG_WAVES_PART),       \
                          pieces_ = diag_phase_word(DIAG_WAVES_PIECES), written_ = diag_phase_word(DIAG_WAVES_WRITTEN); \
            GAS uint64_t *row_ = (mirror) + (size_t)(wave) * DIAG_ROW_WORDS;   /* (a phase's word: its place in row 0) */ \
            row_[loop_] = prof_all_; row_[part_] = prof_t_; row_[pieces_] = prof_n_; row_[written_] = 1ull;        \
        }                                                                                                           \
    } while (0)
#else
#define PROF_DRAIN()
#define PROF_DECL
#define PROF_BEGIN(part) do { } while (0)
#define PROF_END(part) do { } while (0)
#define PROF_DRAINED(part)
#define PROF_TALLY(part, pieces, amount)
#define PROF_IN_MEMBERS
#define PROF_IN_RESET(C)
#define PROF_IN_VAR(v)
#define PROF_IN_MARK(v)
#define PROF_IN_ADD(C, v, pieces)
#define PROF_WRITE_ROW(mirror, wave, C)
#endif

// REINA_ABLATE: ABLATED(part) is true while reina_debug_ablate has the part's bit set
#if DIAG_ON_ABLATE
__device__ uint32_t g_ablate_dev;
#define ABLATED(part) (g_ablate_dev & DIAG_ABLATE_##part)
#else
#define ABLATED(part) false
#endif

// what a diagnostic build exports beside the ABI (the production library has neither)
#ifdef DIAG_ANY
extern "C" size_t reina_diag_describe(char *out, size_t cap) { return diag_describe(out, cap); }
#if DIAG_ON_ABLATE
extern "C" int reina_debug_ablate(uint32_t bits) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_ablate_dev), &bits, sizeof(bits)) == hipSuccess ? 0 : -1;
}
#endif
#endif
#endif   // __HIPCC__
#endif   // REINA_DIAG_H
