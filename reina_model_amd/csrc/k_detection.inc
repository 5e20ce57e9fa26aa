// reina_hip.hip part: the detection report (include/reina_detection.h; DESIGN.md section 6m).  Included behind k_course.inc: a
// report is taken of a course log and through it of its transmission log, and takes their form (one engine, or a group's
// members at blockIdx.y: MEMBER_OF_LAUNCH).  It owns nothing: no record, no launch of the day.
//
// One kernel, bound by memory traffic:
//   k_detect_report  the join of the course log with the transmission links.  load_links<true> streams hot + log, skips a tile
//                    without an infected agent, gathers the cold record of the infected agents and hot + log of their
//                    infectors; on top of that the agent's own record (8 bytes, infected agents only) and the infector's
//                    record (one more 8-byte gather, linked agents only), both of a thread's two agents in flight together.
//                    LDS a workgroup: the fixed tables at the block's own offsets, 3416 x 4 B, the two sum tables 24 x 8 B and
//                    the age tables 644 B -- 14.2 KB -- flushed once per workgroup (flush_lds); the tables by day go to
//                    global atomics aggregated in the wave (wave_add).
// One lane owns an agent; nothing but the report is written.
#include "../../include/reina_detection.h"

#define DET_SUMS (REINA_DETECT_MAX_GROUPS + REINA_DETECT_CLASSES * 2)   // at_large_sum, offspring_sum
static_assert(REINA_DETECT_FIXED_WORDS == 3416u && REINA_DETECT_DAY_WORDS == 55u, "report layout");
static_assert(REINA_DETECT_PHASE == 512u && REINA_DETECT_AT_LARGE == 576u && REINA_DETECT_AT_LARGE_SUM == 1616u && REINA_DETECT_OFFSPRING == 1632u &&
                  REINA_DETECT_OFFSPRING_SUM == 2144u && REINA_DETECT_LINK_CLASS == 2152u && REINA_DETECT_LEAD == 2232u && REINA_DETECT_PAIR == 3256u &&
                  REINA_DETECT_SCALARS == 3400u,
              "report layout");
static_assert(REINA_DETECT_MAX_GROUPS == REINA_TXLOG_MAX_GROUPS, "the groups are the log report's");
static_assert(REINA_DETECT_SEVERITIES == 8 && REINA_DETECT_CLASSES == 4, "RH_SEV has three bits; four detection classes");
static_assert(REINA_DETECT_FIXED_WORDS * 4u + DET_SUMS * 8u + sizeof(ReportAges) <= 16u * 1024u, "LDS budget of k_detect_report");
static_assert((size_t)REINA_MAX_DAYS * REINA_DETECT_MAX_GROUPS * REINA_DETECT_COHORT_FIELDS < (1u << 30), "table cells are int keys");

// the detection class of a record's detection field and the agent's hot word
__device__ __forceinline__ int det_class(uint32_t det, uint32_t w) {
    if (det < TXL_BEFORE) return REINA_DETECT_DATED;
    if (det == TXL_BEFORE) return REINA_DETECT_BEFORE;
    return (w & RH_DETECTED) ? REINA_DETECT_UNDATED : REINA_DETECT_NEVER;
}

// 256 threads, tiles of 512 agents (two per thread), the workgroup's tiles strided over the grid
template <bool GROUP>
__global__ __launch_bounds__(REPORT_THREADS) void k_detect_report(const MemberRef *M_, const MemberRef one_, const uint32_t *log, const crs_rec *rec,
                                                                 size_t stride, uint64_t *report, const TxlArgs a) {
    __shared__ uint32_t s_t[REINA_DETECT_FIXED_WORDS];   // the fixed tables and the scalars, at the block's own offsets (the sums' cells stay 0)
    __shared__ unsigned long long s_sum[DET_SUMS];       // at_large_sum, offspring_sum
    __shared__ ReportAges s_ages;
    MEMBER_OF_LAUNCH;
    const GAS uint32_t *hot = (const GAS uint32_t *)mref_.B.hot;
    const GAS reina_cold_t *cold = (const GAS reina_cold_t *)mref_.B.cold;
    const GAS uint32_t *L = member_block<GROUP>(log, stride);
    const GAS crs_rec *C = member_block<GROUP>(rec, stride);
    GAS unsigned long long *R = member_block<GROUP>((unsigned long long *)report, REINA_DETECT_REPORT_WORDS(a.n_days));
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < REINA_DETECT_FIXED_WORDS; k += REPORT_THREADS) s_t[k] = 0u;
    if (tid < DET_SUMS) s_sum[tid] = 0ull;
    s_ages.load(a.p);
    __syncthreads();
    const uint32_t N = a.p.n_agents, D = a.n_days, tiles = (N + REPORT_TILE - 1u) / REPORT_TILE;
    uint32_t *s_sc = s_t + REINA_DETECT_SCALARS;
    GAS unsigned long long *coh_t = R + REINA_DETECT_COHORT(D), *det_t = R + REINA_DETECT_DETECTIONS(D), *lnk_t = R + REINA_DETECT_LINKS_BY_DAY(D);
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        Links l;
        if (!load_links<true>(l, t, N, hot, cold, L, s_sc, REINA_DETECT_S_INFECTED, REINA_DETECT_S_ROOTS, REINA_DETECT_S_LINKED, REINA_DETECT_S_BAD_LINKS)) continue;
        // the agent's own record and its infector's, of both agents in flight together (a linked infector is in range: load_links)
        crs_rec r[2], rs[2];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            r[j] = l.inf[j] ? C[l.idx[j]] : 0ull;
            rs[j] = l.linked[j] ? C[(uint32_t)l.src[j]] : 0ull;
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint32_t w = l.w[j], st = RH_STATE(w), sev = RH_SEV(w), n = l.n[j];
            const bool inf = l.inf[j], linked = l.linked[j], closed = st >= RS_RECOVERED;
            const uint32_t ti = l.lw[j] & 0xFFFFu, oi = l.lw[j] >> 16;
            const uint32_t det = CRS_FIELD(r[j], REINA_COURSE_F_DETECTION), adm = CRS_FIELD(r[j], REINA_COURSE_F_ADMISSION);
            const uint32_t ds = CRS_FIELD(rs[j], REINA_COURSE_F_DETECTION);
            const bool tk = inf && ti < TXL_BEFORE, ok = oi < TXL_BEFORE, ak = adm < TXL_BEFORE;
            const int dc = inf ? det_class(det, w) : 0, dcs = linked ? det_class(ds, l.sw[j]) : 0;
            const bool dated = inf && dc == REINA_DETECT_DATED;
            int ph = 3;
            if (oi == TXL_NONE || (ok && det < oi))
                ph = 0;
            else if (ak && det == adm)
                ph = 1;
            else if (ok && (adm == TXL_NONE || (ak && det < adm)))
                ph = 2;
            int cls = 4;
            if (dcs == REINA_DETECT_NEVER)
                cls = 0;
            else if (dcs == REINA_DETECT_DATED && tk)
                cls = ti < ds ? 1 : (ti == ds ? 2 : 3);
            const bool ahead = linked && (cls == 1 || cls == 2);
            int g = 0, gs = 0;
            if (inf) g = s_ages.group_of(l.idx[j]);
            if (linked) gs = s_ages.group_of((uint32_t)l.src[j]);
            // the scalars beyond load_links' four (the class scalars differ by lane; out_of_range: one predicate a date)
            wave_count(s_sc, inf ? (int)REINA_DETECT_S_NEVER + dc : -1);
            wave_tally(&s_sc[REINA_DETECT_S_BREACH], linked && cls == 3);
            wave_tally(&s_sc[REINA_DETECT_S_OUT_OF_RANGE], tk && ti >= D);
            wave_tally(&s_sc[REINA_DETECT_S_OUT_OF_RANGE], dated && det >= D);
            // the fixed tables (LDS)
            wave_count(s_t, inf ? (int)REINA_DETECT_ASCERTAIN + (g * REINA_DETECT_SEVERITIES + (int)sev) * REINA_DETECT_CLASSES + dc : -1);
            wave_count(s_t, dated ? (int)REINA_DETECT_PHASE + g * REINA_DETECT_PHASES + ph : -1);
            const bool large = dated && tk;
            const int days = (int)det - (int)ti;
            wave_count(s_t, large ? (int)REINA_DETECT_AT_LARGE + g * REINA_DETECT_BINS + txl_clip(days, REINA_DETECT_BINS - 1) : -1);
            wave_count(s_t, large ? (int)REINA_DETECT_AT_LARGE_N + g : -1);
            if (large) atomicAdd(&s_sum[g], (unsigned long long)(long long)days);
            const int oc = dc * 2 + (closed ? 1 : 0);
            wave_count(s_t, inf ? (int)REINA_DETECT_OFFSPRING + oc * REINA_DETECT_BINS + (int)(n < REINA_DETECT_BINS - 1u ? n : REINA_DETECT_BINS - 1u) : -1);
            if (inf && n) atomicAdd(&s_sum[REINA_DETECT_MAX_GROUPS + oc], (unsigned long long)n);
            wave_count(s_t, linked ? (int)REINA_DETECT_LINK_CLASS + gs * REINA_DETECT_LINK_CLASSES + cls : -1);
            wave_count(s_t, ahead ? (int)REINA_DETECT_LEAD + gs * REINA_DETECT_BINS + txl_clip((int)ds - (int)ti, REINA_DETECT_BINS - 1) : -1);
            wave_count(s_t, linked && dated && dcs == REINA_DETECT_DATED
                                ? (int)REINA_DETECT_PAIR + txl_clip((int)det - (int)ds + REINA_DETECT_PAIR_SHIFT, REINA_DETECT_PAIR_BINS - 1)
                                : -1);
            wave_count(s_t, linked ? (int)REINA_DETECT_PAIR_CLASS + dcs * REINA_DETECT_CLASSES + dc : -1);
            // the tables by day (global, aggregated in the wave)
            const bool in = tk && ti < D;
            const int ck = in ? (int)((ti * REINA_DETECT_MAX_GROUPS + (uint32_t)g) * REINA_DETECT_COHORT_FIELDS) : -1;
            wave_add(coh_t, ck, 1ull);
            wave_add(coh_t + 1, ck, dc != REINA_DETECT_NEVER ? 1ull : 0ull);
            wave_add(coh_t + 2, ck, closed ? 1ull : 0ull);
            wave_add(det_t, dated && det < D ? (int)(det * REINA_DETECT_PHASES) + ph : -1, 1ull);
            const int lk = linked && in ? (int)(ti * REINA_DETECT_LINK_DAY_FIELDS) : -1;
            wave_add(lnk_t, lk, 1ull);
            wave_add(lnk_t + 1, lk, cls == 0 ? 1ull : 0ull);
            wave_add(lnk_t + 2, lk, ahead ? 1ull : 0ull);
        }
    }
    __syncthreads();
    flush_lds(s_t, REINA_DETECT_FIXED_WORDS, R);
    flush_lds(s_sum, REINA_DETECT_MAX_GROUPS, R + REINA_DETECT_AT_LARGE_SUM);
    flush_lds(s_sum + REINA_DETECT_MAX_GROUPS, REINA_DETECT_CLASSES * 2, R + REINA_DETECT_OFFSPRING_SUM);
}

// ---------------------------------------------------------------------------------------------
// host side

extern "C" {

int reina_detect_version(void) { return REINA_DETECT_VERSION; }

int reina_detect_report(reina_course_t *course, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days, uint64_t *dev_report, void *stream) {
    if (int rc = course_live(course)) return rc;
    reina_txlog *l = course->log;
    hipStream_t s = (hipStream_t)stream;
    return day_report(l, "detection report", REINA_DETECT_MAX_GROUPS, REINA_DETECT_REPORT_WORDS(n_days), age_group, n_groups, n_days, dev_report, s,
                      [&](const TxlArgs &a, uint32_t grid, uint32_t K) -> int {
                          launch_members(k_detect_report, l->g, grid, K, REPORT_THREADS, s, l->d_refs, l->e0->h_ref, l->d_log, course->d_rec, l->stride, dev_report, a);
                          return REINA_OK;
                      });
}

}  // extern "C"
