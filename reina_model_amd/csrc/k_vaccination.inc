// reina_hip.hip part: the vaccination report (include/reina_vaccination.h; DESIGN.md section 6l).  Included behind
// k_txlog.inc: a report is taken of a transmission log and takes its form (one engine, or a group's members at blockIdx.y:
// MEMBER_OF_LAUNCH).  It owns nothing: no record, no launch of the day.
//
// One kernel, bound by memory traffic:
//   k_vacc_report    streams the hot words; a wave skips a tile that holds no vaccinated and no infected agent (most of a
//                    population is neither), loads the log word of the infected agents alone and the cold record's vacc_day
//                    of the vaccinated ones alone -- one 32-byte sector for four useful bytes; the vaccinated are contiguous
//                    age runs, so whole lines are used at an eighth.  LDS a workgroup: the fixed tables at the block's own
//                    offsets, 4928 x 4 B, and the age tables 644 B -- 19.9 KB -- flushed once per workgroup (flush_lds); the
//                    tables by day go to global atomics aggregated in the wave (wave_add).
// One lane owns an agent; nothing but the report is written.
#include "../../include/reina_vaccination.h"

static_assert(REINA_VACC_FIXED_WORDS == 4928u && REINA_VACC_DAY_WORDS == 76u, "report layout");
static_assert(REINA_VACC_SEVERITY == 0u && REINA_VACC_OUTCOME == 512u && REINA_VACC_SINCE == 768u && REINA_VACC_POPULATION == 4864u && REINA_VACC_SCALARS == 4912u,
              "report layout");
static_assert(REINA_VACC_MAX_GROUPS == REINA_TXLOG_MAX_GROUPS, "the groups are the log report's");
static_assert(REINA_VACC_SEVERITIES == 8 && REINA_VACC_STATUSES == 4 && REINA_VACC_DATED_STATUSES == 3, "RH_SEV has three bits; status 3 has no date");
static_assert(REINA_VACC_FIXED_WORDS * 4u + sizeof(ReportAges) <= 20u * 1024u, "LDS budget of k_vacc_report");
static_assert((size_t)REINA_MAX_DAYS * REINA_VACC_MAX_GROUPS * REINA_VACC_DATED_STATUSES < (1u << 30), "table cells are int keys");

// 256 threads, tiles of 512 agents (two per thread), the workgroup's tiles strided over the grid
template <bool GROUP>
__global__ __launch_bounds__(REPORT_THREADS) void k_vacc_report(const MemberRef *M_, const MemberRef one_, const uint32_t *log, size_t stride, uint64_t *report,
                                                               const TxlArgs a) {
    __shared__ uint32_t s_t[REINA_VACC_FIXED_WORDS];   // the fixed tables and the scalars, at the block's own offsets
    __shared__ ReportAges s_ages;
    MEMBER_OF_LAUNCH;
    const GAS uint32_t *hot = (const GAS uint32_t *)mref_.B.hot;
    const GAS reina_cold_t *cold = (const GAS reina_cold_t *)mref_.B.cold;
    const GAS uint32_t *L = member_block<GROUP>(log, stride);
    GAS unsigned long long *R = member_block<GROUP>((unsigned long long *)report, REINA_VACC_REPORT_WORDS(a.n_days));
    const uint32_t tid = threadIdx.x;
    for (uint32_t k = tid; k < REINA_VACC_FIXED_WORDS; k += REPORT_THREADS) s_t[k] = 0u;
    s_ages.load(a.p);
    __syncthreads();
    const uint32_t N = a.p.n_agents, D = a.n_days, tiles = (N + REPORT_TILE - 1u) / REPORT_TILE;
    uint32_t *s_sc = s_t + REINA_VACC_SCALARS;
    GAS unsigned long long *vac_t = R + REINA_VACC_VACCINATIONS(D), *inf_t = R + REINA_VACC_INFECTIONS(D), *coh_t = R + REINA_VACC_COHORT(D);
    for (uint32_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        uint32_t idx[2], w[2], lw[2];
        int32_t vd[2];
        tile_words(t, N, hot, idx, w);
        if (!__ballot(((w[0] | w[1]) & (7u | RH_VACCINATED)) != 0u)) continue;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            lw[j] = RH_STATE(w[j]) != RS_SUSCEPTIBLE ? L[idx[j]] : 0u;
            vd[j] = (w[j] & RH_VACCINATED) ? cold[idx[j]].vacc_day : -1;
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const uint32_t st = RH_STATE(w[j]), sev = RH_SEV(w[j]);
            const bool inf = st != RS_SUSCEPTIBLE, vac = (w[j] & RH_VACCINATED) != 0u;
            const bool valid = vac && (uint32_t)vd[j] < (uint32_t)REINA_MAX_DAYS;
            const uint32_t ti = lw[j] & 0xFFFFu;
            const bool tk = inf && ti < TXL_BEFORE;
            const int since = valid && tk ? (int)ti - vd[j] : 0;   // (both below 2^16)
            int status = -1;
            bool after = false;
            if (inf) {
                if (!vac) {
                    status = REINA_VACC_UNVACCINATED;
                } else if (!valid || !tk) {
                    status = REINA_VACC_UNDETERMINED;
                } else if (since < 0) {
                    status = REINA_VACC_UNVACCINATED;
                    after = true;
                } else {
                    status = since <= REINA_VACC_PROTECTION_DAYS ? REINA_VACC_RECENT : REINA_VACC_PROTECTED;
                }
            }
            int g = 0;
            if (inf || vac) g = s_ages.group_of(idx[j]);
            const bool dated = status >= 0 && status < REINA_VACC_DATED_STATUSES && tk;
            // the scalars (out_of_range: one predicate a date)
            wave_tally(&s_sc[REINA_VACC_S_VACCINATED], vac);
            wave_tally(&s_sc[REINA_VACC_S_INFECTED], inf);
            wave_tally(&s_sc[REINA_VACC_S_VACCINATED_INFECTED], vac && inf);
            wave_tally(&s_sc[REINA_VACC_S_AFTER_INFECTION], after);
            wave_tally(&s_sc[REINA_VACC_S_UNDETERMINED], status == REINA_VACC_UNDETERMINED);
            wave_tally(&s_sc[REINA_VACC_S_BAD_VACC_DAY], vac && !valid);
            wave_tally(&s_sc[REINA_VACC_S_OUT_OF_RANGE], valid && (uint32_t)vd[j] >= D);
            wave_tally(&s_sc[REINA_VACC_S_OUT_OF_RANGE], dated && ti >= D);
            // the fixed tables (LDS)
            const int cell = status * REINA_VACC_MAX_GROUPS + g;
            const bool closed = st >= RS_RECOVERED, dead = st == RS_DEAD, severe = sev >= RV_SEVERE;
            wave_count(s_t, inf ? (int)REINA_VACC_SEVERITY + cell * REINA_VACC_SEVERITIES + (int)sev : -1);
            const int oc = (int)REINA_VACC_OUTCOME + cell * REINA_VACC_OUTCOME_FIELDS;
            wave_count(s_t, inf ? oc : -1);
            wave_count(s_t, inf && closed ? oc + 1 : -1);
            wave_count(s_t, inf && dead ? oc + 2 : -1);
            wave_count(s_t, inf && (w[j] & RH_DETECTED) ? oc + 3 : -1);
            const bool timed = status == REINA_VACC_RECENT || status == REINA_VACC_PROTECTED;
            const int sc = (int)REINA_VACC_SINCE + g * REINA_VACC_SINCE_BINS + txl_clip(since, REINA_VACC_SINCE_BINS - 1);
            wave_count(s_t, timed ? sc : -1);
            wave_count(s_t, timed && severe ? sc + REINA_VACC_MAX_GROUPS * REINA_VACC_SINCE_BINS : -1);
            const int pc = (int)REINA_VACC_POPULATION + g * REINA_VACC_POPULATION_FIELDS;
            wave_count(s_t, vac ? pc : -1);
            wave_count(s_t, vac ? pc + (inf ? 2 : 1) : -1);
            // the tables by day (global, aggregated in the wave)
            wave_add(vac_t, valid && (uint32_t)vd[j] < D ? vd[j] * REINA_VACC_MAX_GROUPS + g : -1, 1ull);
            const bool in = dated && ti < D;
            wave_add(inf_t, in ? (int)((ti * REINA_VACC_MAX_GROUPS + (uint32_t)g) * REINA_VACC_DATED_STATUSES) + status : -1, 1ull);
            const int ck = in ? (int)((ti * REINA_VACC_DATED_STATUSES + (uint32_t)status) * REINA_VACC_COHORT_FIELDS) : -1;
            wave_add(coh_t, ck, 1ull);
            wave_add(coh_t + 1, ck, severe ? 1ull : 0ull);
            wave_add(coh_t + 2, ck, dead ? 1ull : 0ull);
            wave_add(coh_t + 3, ck, closed ? 1ull : 0ull);
        }
    }
    __syncthreads();
    flush_lds(s_t, REINA_VACC_FIXED_WORDS, R);
}

// ---------------------------------------------------------------------------------------------
// host side

extern "C" {

int reina_vacc_version(void) { return REINA_VACC_VERSION; }

int reina_vacc_report(reina_txlog_t *l, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days, uint64_t *dev_report, void *stream) {
    if (!l) return REINA_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    return day_report(l, "vaccination report", REINA_VACC_MAX_GROUPS, REINA_VACC_REPORT_WORDS(n_days), age_group, n_groups, n_days, dev_report, s,
                      [&](const TxlArgs &a, uint32_t grid, uint32_t K) -> int {
                          launch_members(k_vacc_report, l->g, grid, K, REPORT_THREADS, s, l->d_refs, l->e0->h_ref, l->d_log, l->stride, dev_report, a);
                          return REINA_OK;
                      });
}

}  // extern "C"
