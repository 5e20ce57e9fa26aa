// reina_hip.hip part: the clinical course log (include/reina_course.h; DESIGN.md section 6k).  Included behind k_txlog.inc: a
// course is attached to a transmission log, takes its form (one engine, or a group's members at blockIdx.y: MEMBER_OF_LAUNCH)
// and is recorded by the log's own launch of the day.
//
// Three kernels, each bound by memory traffic:
//   k_course_begin   streams the hot words (16 bytes a lane) and writes every record (32 bytes a lane).
//   k_course_day     takes k_txlog_day's place in the log's launch of the day when a course is attached: the same walk over
//                    the ACTIVE plane (active_tile), one tile a wave, the same update of the log word (txl_day_update, in both
//                    forms), and for the active agents in a state >= ILLNESS or with RH_DETECTED one 8-byte load of the record
//                    and a store where it changes.  An incubating undetected agent costs nothing beyond k_txlog_day.  The
//                    ACTIVE plane is enough: a record closes with its outcome, and k_scan clears RH_ACTIVE on the day AFTER a
//                    removal (tests/test_course.py holds the property on oracle B).
//   k_course_report  streams hot word, log word and record of the tiles that hold an infected agent: no links, no gathers.
//                    LDS a workgroup: delay + delay_n 8320 x 4 B, delay_sum 128 x 8 B, pathway + scalars 176 x 4 B, the age
//                    tables 644 B -- 35.6 KB, four workgroups a compute unit -- flushed once per workgroup (flush_lds); the
//                    tables by day go to global atomics aggregated in the wave (wave_add).
// One lane owns an agent: no atomics on the records, no fences (a kernel boundary lies on either side of every launch).
#include "../../include/reina_course.h"

#define CRS_HIST (REINA_COURSE_DELAY_SUM - REINA_COURSE_DELAY)                            // delay and delay_n, as the block has them
#define CRS_SUMS (REINA_COURSE_PATHWAY - REINA_COURSE_DELAY_SUM)
#define CRS_TAIL (REINA_COURSE_FIXED_WORDS - REINA_COURSE_PATHWAY)                        // pathway and the scalars
static_assert(REINA_COURSE_FIXED_WORDS == 8624u && REINA_COURSE_DAY_WORDS == 144u, "report layout");
static_assert(REINA_COURSE_MAX_GROUPS == REINA_TXLOG_MAX_GROUPS, "the groups are the log report's");
static_assert(REINA_COURSE_S_WITH_OUTCOME == REINA_COURSE_S_WITH_DETECTION + 3, "the with_* scalars stand in the order of the record's fields");
static_assert(CRS_HIST * 4u + CRS_SUMS * 8u + CRS_TAIL * 4u + sizeof(ReportAges) <= 40u * 1024u, "LDS budget of k_course_report");

typedef unsigned long long crs_rec;
#define CRS_FIELD(r, bit) ((uint32_t)((r) >> (bit)) & 0xFFFFu)
#define CRS_PACK(det, adm, icu, out)                                                                                  \
    ((crs_rec)(det) << REINA_COURSE_F_DETECTION | (crs_rec)(adm) << REINA_COURSE_F_ADMISSION | (crs_rec)(icu) << REINA_COURSE_F_ICU | \
     (crs_rec)(out) << REINA_COURSE_F_OUTCOME)

__device__ __forceinline__ crs_rec crs_begin_record(uint32_t w) {
    const uint32_t st = RH_STATE(w);
    if (st >= RS_RECOVERED) return CRS_PACK(TXL_BEFORE, TXL_BEFORE, TXL_BEFORE, TXL_BEFORE);
    return CRS_PACK(st != RS_SUSCEPTIBLE && (w & RH_DETECTED) ? TXL_BEFORE : TXL_NONE,
                    st == RS_HOSPITALIZED || st == RS_IN_ICU ? TXL_BEFORE : TXL_NONE, st == RS_IN_ICU ? TXL_BEFORE : TXL_NONE, TXL_NONE);
}

// the records are padded to whole tiles like the log (beyond n_agents: the record of a susceptible agent, never read back)
template <bool GROUP>
__global__ __launch_bounds__(REPORT_THREADS) void k_course_begin(const MemberRef *M_, const MemberRef one_, crs_rec *rec, size_t stride, uint32_t N) {
    MEMBER_OF_LAUNCH;
    const GAS uint32_t *hot = (const GAS uint32_t *)mref_.B.hot;
    GAS crs_rec *C = member_block<GROUP>(rec, stride);
    const uint32_t quads = (N + 3u) / 4u;
    for (uint32_t q = blockIdx.x * REPORT_THREADS + threadIdx.x; q < quads; q += gridDim.x * REPORT_THREADS) {
        const uint32_t i = 4u * q;
        v4u_ w;
        if (i + 3u < N) {
            w = *reinterpret_cast<const GAS v4u_ *>(hot + i);
        } else {
            w.x = hot[i];
            w.y = i + 1u < N ? hot[i + 1u] : 0u;
            w.z = i + 2u < N ? hot[i + 2u] : 0u;
            w.w = 0u;
        }
        const crs_rec r0 = crs_begin_record(w.x), r1 = crs_begin_record(w.y), r2 = crs_begin_record(w.z), r3 = crs_begin_record(w.w);
        v4u_ a, b;
        a.x = (uint32_t)r0, a.y = (uint32_t)(r0 >> 32), a.z = (uint32_t)r1, a.w = (uint32_t)(r1 >> 32);
        b.x = (uint32_t)r2, b.y = (uint32_t)(r2 >> 32), b.z = (uint32_t)r3, b.w = (uint32_t)(r3 >> 32);
        *reinterpret_cast<GAS v4u_ *>(C + i) = a;          // (i is a multiple of four and stride of 512: 32-byte aligned)
        *reinterpret_cast<GAS v4u_ *>(C + i + 2u) = b;
    }
}

// the day's update of one agent's record r (state != SUSCEPTIBLE): a closed record is left alone, a field that is NONE gets
// the day when its condition holds, and the record is stored only where it changed
__device__ __forceinline__ void crs_day_update(GAS crs_rec *C, uint32_t i, uint32_t w, crs_rec r, uint32_t day) {
    if (CRS_FIELD(r, REINA_COURSE_F_OUTCOME) != TXL_NONE) return;
    const uint32_t st = RH_STATE(w);
    const crs_rec mask = 0xFFFFull, d = day;
    crs_rec nr = r;
    if (CRS_FIELD(r, REINA_COURSE_F_DETECTION) == TXL_NONE && (w & RH_DETECTED))
        nr = (nr & ~(mask << REINA_COURSE_F_DETECTION)) | d << REINA_COURSE_F_DETECTION;
    if (CRS_FIELD(r, REINA_COURSE_F_ADMISSION) == TXL_NONE && (st == RS_HOSPITALIZED || st == RS_IN_ICU))
        nr = (nr & ~(mask << REINA_COURSE_F_ADMISSION)) | d << REINA_COURSE_F_ADMISSION;
    if (CRS_FIELD(r, REINA_COURSE_F_ICU) == TXL_NONE && st == RS_IN_ICU) nr = (nr & ~(mask << REINA_COURSE_F_ICU)) | d << REINA_COURSE_F_ICU;
    if (st >= RS_RECOVERED) nr = (nr & ~(mask << REINA_COURSE_F_OUTCOME)) | d << REINA_COURSE_F_OUTCOME;
    if (nr != r) C[i] = nr;
}

// k_txlog_day with the course update beside the log's: four waves a workgroup, one tile a wave and round
template <bool GROUP>
__global__ __launch_bounds__(REPORT_THREADS) void k_course_day(const MemberRef *M_, const MemberRef one_, uint32_t *log, crs_rec *rec, size_t stride, uint32_t N,
                                                               uint32_t day, uint32_t by_hot) {
    MEMBER_OF_LAUNCH;
    const GAS uint32_t *hot = (const GAS uint32_t *)mref_.B.hot;
    const GAS uint32_t *plane = (const GAS uint32_t *)mref_.B.active_bits;
    GAS uint32_t *L = member_block<GROUP>(log, stride);
    GAS crs_rec *C = member_block<GROUP>(rec, stride);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t tiles = (N + REPORT_TILE - 1u) / REPORT_TILE;
    const uint32_t d8 = day & 0xFFu, o8 = (day + 1u) & 0xFFu;
    for (uint32_t t = blockIdx.x * (REPORT_THREADS / 64u) + wave; t < tiles; t += gridDim.x * (REPORT_THREADS / 64u)) {
        uint32_t w[8];
        if (!active_tile(plane, hot, t, N, lane, w)) continue;
        // the records of the agents the course looks at, all in flight together (0: a closed record, nothing to do)
        crs_rec r[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t i = t * REPORT_TILE + (uint32_t)j * 64u + lane, st = RH_STATE(w[j]);
            r[j] = st >= RS_ILLNESS || (st != RS_SUSCEPTIBLE && (w[j] & RH_DETECTED)) ? C[i] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t i = t * REPORT_TILE + (uint32_t)j * 64u + lane;
            if (RH_STATE(w[j]) == RS_SUSCEPTIBLE) continue;
            txl_day_update(L, i, w[j], day, d8, o8, by_hot);
            crs_day_update(C, i, w[j], r[j], day);
        }
    }
}

// value into delay table `kind` of group g (LDS): the clipped histogram, the count and the sum before clipping; whole waves
__device__ __forceinline__ void crs_delay(uint32_t *s_h, crs_rec *s_sum, uint32_t kind, int g, bool on, int value) {
    const int cell = (int)(kind * REINA_COURSE_MAX_GROUPS) + g;
    wave_count(s_h, on ? cell * REINA_COURSE_DELAY_BINS + txl_clip(value, REINA_COURSE_DELAY_BINS - 1) : -1);
    wave_count(s_h, on ? (int)(REINA_COURSE_DELAY_N - REINA_COURSE_DELAY) + cell : -1);
    if (on) atomicAdd(&s_sum[cell], (crs_rec)(long long)value);
}

// 256 threads, tiles of 512 agents (two per thread), the workgroup's tiles strided over the grid
template <bool GROUP>
__global__ __launch_bounds__(REPORT_THREADS) void k_course_report(const MemberRef *M_, const MemberRef one_, const uint32_t *log, const crs_rec *rec,
                                                                  size_t stride, uint64_t *report, const TxlArgs a) {
    __shared__ uint32_t s_h[CRS_HIST];       // delay, delay_n
    __shared__ crs_rec s_sum[CRS_SUMS];      // delay_sum
    __shared__ uint32_t s_p[CRS_TAIL];       // pathway, scalars
    __shared__ ReportAges s_ages;
    MEMBER_OF_LAUNCH;
    const GAS uint32_t *hot = (const GAS uint32_t *)mref_.B.hot;
    const GAS uint32_t *L = member_block<GROUP>(log, stride);
    const GAS crs_rec *C = member_block<GROUP>(rec, stride);
    GAS unsigned long long *R = member_block<GROUP>((unsigned long long *)report, REINA_COURSE_REPORT_WORDS(a.n_days));
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < CRS_HIST; k += REPORT_THREADS) s_h[k] = 0u;
    if (tid < CRS_SUMS) s_sum[tid] = 0ull;
    if (tid < CRS_TAIL) s_p[tid] = 0u;
    s_ages.load(a.p);
    __syncthreads();
    const uint32_t N = a.p.n_agents, D = a.n_days, tiles = (N + REPORT_TILE - 1u) / REPORT_TILE;
    uint32_t *s_sc = s_p + (REINA_COURSE_SCALARS - REINA_COURSE_PATHWAY);
    GAS unsigned long long *day_t[3] = {R + REINA_COURSE_DETECTIONS(D), R + REINA_COURSE_ADMISSIONS(D), R + REINA_COURSE_ICU_ADMISSIONS(D)};
    GAS unsigned long long *dead_t = R + REINA_COURSE_DEATHS(D), *rcv_t = R + REINA_COURSE_RECOVERIES(D), *coh_t = R + REINA_COURSE_COHORT(D);
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        uint32_t idx[2], w[2], lw[2];
        crs_rec r[2];
        tile_words(t, N, hot, idx, w);
        if (!__ballot(RH_STATE(w[0]) != RS_SUSCEPTIBLE || RH_STATE(w[1]) != RS_SUSCEPTIBLE)) continue;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const bool inf = RH_STATE(w[j]) != RS_SUSCEPTIBLE;
            lw[j] = inf ? L[idx[j]] : 0u;
            r[j] = inf ? C[idx[j]] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint32_t st = RH_STATE(w[j]);
            const bool inf = st != RS_SUSCEPTIBLE, dead = st == RS_DEAD, rcv = st == RS_RECOVERED;
            const uint32_t ti = lw[j] & 0xFFFFu, oi = lw[j] >> 16;
            const uint32_t f[4] = {CRS_FIELD(r[j], REINA_COURSE_F_DETECTION), CRS_FIELD(r[j], REINA_COURSE_F_ADMISSION),
                                   CRS_FIELD(r[j], REINA_COURSE_F_ICU), CRS_FIELD(r[j], REINA_COURSE_F_OUTCOME)};
            const bool tk = inf && ti < TXL_BEFORE, ok = inf && oi < TXL_BEFORE;
            const bool k[4] = {inf && f[0] < TXL_BEFORE, inf && f[1] < TXL_BEFORE, inf && f[2] < TXL_BEFORE, inf && f[3] < TXL_BEFORE};
            const int det = (int)f[0], adm = (int)f[1], icu = (int)f[2], out = (int)f[3], o = (int)oi;
            int g = 0;
            if (inf) g = s_ages.group_of(idx[j]);
            // the scalars (out_of_range: one predicate a date)
            wave_tally(&s_sc[REINA_COURSE_S_INFECTED], inf);
#pragma unroll
            for (int c = 0; c < 4; c++) {
                wave_tally(&s_sc[REINA_COURSE_S_WITH_DETECTION + c], k[c]);
                wave_tally(&s_sc[REINA_COURSE_S_OUT_OF_RANGE], k[c] && f[c] >= D);
            }
            wave_tally(&s_sc[REINA_COURSE_S_DETECTED_UNDATED], inf && (w[j] & RH_DETECTED) && f[0] == TXL_NONE);
            wave_tally(&s_sc[REINA_COURSE_S_DIED_OUTSIDE], dead && (w[j] & RH_POD_OUTSIDE));
            // the delays (LDS)
            const bool ward = k[3] && k[1] && f[2] == TXL_NONE, unit = k[3] && k[2];
            crs_delay(s_h, s_sum, 0u, g, k[0] && ok, det - o + REINA_COURSE_DETECTION_SHIFT);
            crs_delay(s_h, s_sum, 1u, g, k[1] && ok, adm - o);
            crs_delay(s_h, s_sum, 2u, g, k[2] && k[1], icu - adm);
            crs_delay(s_h, s_sum, 3u, g, ward && rcv, out - adm);
            crs_delay(s_h, s_sum, 4u, g, ward && dead, out - adm);
            crs_delay(s_h, s_sum, 5u, g, unit && rcv, out - icu);
            crs_delay(s_h, s_sum, 6u, g, unit && dead, out - icu);
            crs_delay(s_h, s_sum, 7u, g, k[3] && ok && dead, out - o);
            // the pathway
            uint32_t cls = 9u;
            const bool before = f[1] == TXL_BEFORE || f[2] == TXL_BEFORE || f[3] == TXL_BEFORE;
            if (!before && (f[3] == TXL_NONE || dead || rcv))
                cls = (f[3] == TXL_NONE ? 0u : (rcv ? 3u : 6u)) + (k[2] ? 2u : (k[1] ? 1u : 0u));
            wave_count(s_p, inf ? g * REINA_COURSE_CLASSES + (int)cls : -1);
            // the tables by day (global, aggregated in the wave)
#pragma unroll
            for (int c = 0; c < 3; c++) wave_add(day_t[c], k[c] && f[c] < D ? (int)(f[c] * REINA_COURSE_MAX_GROUPS) + g : -1, 1ull);
            const int ok_out = k[3] && f[3] < D ? (int)(f[3] * REINA_COURSE_MAX_GROUPS) + g : -1;
            wave_add(dead_t, dead ? ok_out : -1, 1ull);
            wave_add(rcv_t, rcv ? ok_out : -1, 1ull);
            const int ck = tk && ti < D ? (int)((ti * REINA_COURSE_MAX_GROUPS + (uint32_t)g) * REINA_COURSE_COHORT_FIELDS) : -1;
            wave_add(coh_t, ck, 1ull);
            wave_add(coh_t + 1, ck, st >= RS_RECOVERED ? 1ull : 0ull);
            wave_add(coh_t + 2, ck, k[1] ? 1ull : 0ull);
            wave_add(coh_t + 3, ck, dead ? 1ull : 0ull);
        }
    }
    __syncthreads();
    flush_lds(s_h, CRS_HIST, R + REINA_COURSE_DELAY);
    flush_lds(s_sum, CRS_SUMS, R + REINA_COURSE_DELAY_SUM);
    flush_lds(s_p, CRS_TAIL, R + REINA_COURSE_PATHWAY);
}

// ---------------------------------------------------------------------------------------------
// host side

struct reina_course {
    reina_txlog *log = nullptr;              // the log it is attached to: its form, members and stride are the course's
    crs_rec *d_rec = nullptr;                // [members][log->stride]
};

static void free_course(reina_course *c) {
    if (c->log && c->log->course == c) c->log->course = nullptr;
    if (c->d_rec) (void)hipFree(c->d_rec);
    delete c;
}

// the log's launch of the day with a course attached (txlog_launch_day)
static int course_launch_day(reina_txlog *l, uint32_t grid, uint32_t day, uint32_t by_hot, hipStream_t s) {
    const uint32_t N = l->e0->cfg.n_agents, K = (uint32_t)l->members.size();
    launch_members(k_course_day, l->g, grid, K, REPORT_THREADS, s, l->d_refs, l->e0->h_ref, l->d_log, l->course->d_rec, l->stride, N, day, by_hot);
    return REINA_OK;
}

static void course_detach(reina_course *c) { c->log = nullptr; }

// what every entry point asks first: a course whose log is still there
static int course_live(const reina_course *c) {
    if (!c) return REINA_E_INVALID;
    if (c->log) return REINA_OK;
    return refuse("course: the transmission log it was attached to is gone");
}

extern "C" {

int reina_course_version(void) { return REINA_COURSE_VERSION; }

int reina_course_create(reina_txlog_t *l, void *stream, reina_course_t **out) {
    if (!l || !out) return REINA_E_INVALID;
    if (int rc = attachment_check_members(l->members, "course", "the log it is attached to is")) return rc;
    if (l->course) return refuse("course: the log has a course attached already");
    std::unique_ptr<reina_course, void (*)(reina_course *)> c(new reina_course(), free_course);   // (freed by a failing return)
    hipStream_t s = (hipStream_t)stream;
    const uint32_t N = l->e0->cfg.n_agents, K = (uint32_t)l->members.size();
    HIP_CHECK(hipMalloc(&c->d_rec, sizeof(crs_rec) * l->stride * K));
    const uint32_t grid = txlog_grid(l, ((N + 3u) / 4u + REPORT_THREADS - 1u) / REPORT_THREADS);
    launch_members(k_course_begin, l->g, grid, K, REPORT_THREADS, s, l->d_refs, l->e0->h_ref, c->d_rec, l->stride, N);
    c->log = l;
    l->course = c.get();
    *out = c.release();
    return REINA_OK;
}

int reina_course_destroy(reina_course_t *course) {
    if (!course) return REINA_E_INVALID;
    free_course(course);
    return REINA_OK;
}

int reina_course_report(reina_course_t *course, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days, uint64_t *dev_report, void *stream) {
    if (int rc = course_live(course)) return rc;
    reina_txlog *l = course->log;
    hipStream_t s = (hipStream_t)stream;
    return day_report(l, "course report", REINA_COURSE_MAX_GROUPS, REINA_COURSE_REPORT_WORDS(n_days), age_group, n_groups, n_days, dev_report, s,
                      [&](const TxlArgs &a, uint32_t grid, uint32_t K) -> int {
                          launch_members(k_course_report, l->g, grid, K, REPORT_THREADS, s, l->d_refs, l->e0->h_ref, l->d_log, course->d_rec, l->stride, dev_report, a);
                          return REINA_OK;
                      });
}

int reina_course_read(reina_course_t *course, uint32_t member, uint64_t *out_host, void *stream) {
    if (!out_host) return REINA_E_INVALID;
    if (int rc = course_live(course)) return rc;
    return member_copy(course->log, course->d_rec, course->log->stride, sizeof(crs_rec), member, out_host, true, "course", (hipStream_t)stream);
}

int reina_course_write(reina_course_t *course, uint32_t member, const uint64_t *in_host, void *stream) {
    if (!in_host) return REINA_E_INVALID;
    if (int rc = course_live(course)) return rc;
    return member_copy(course->log, course->d_rec, course->log->stride, sizeof(crs_rec), member, const_cast<uint64_t *>(in_host), false, "course", (hipStream_t)stream);
}

}  // extern "C"
