/* A vaccination report: coverage by date and age group, breakthrough infections by the time since the dose, and the protection
 * the programme realised against severe disease and death (companion of reina_txlog.h; same library, same error codes;
 * DESIGN.md section 6l; reina_model_amd/vaccination.py: report_numpy is the executable specification).
 *
 * A report is taken of a transmission log -- of one engine, or of the members of a group -- between two days.  It keeps no
 * state and changes none: it READS the hot words, the cold records' vacc_day (only where RH_VACCINATED is set), the log words,
 * the population's age_start and a caller table age -> group (< REINA_VACC_MAX_GROUPS, the log report's groups), and WRITES
 * the report block alone.
 *
 * PER AGENT, with w the hot word:  st = RH_STATE(w),  vac = w & RH_VACCINATED,  inf = st != 0,  sev = RH_SEV(w) (the severity
 * drawn at infection, bits 3-5, never cleared),  vd = vacc_day (read when vac),  t = the log's infection half word (KNOWN when
 * it is neither REINA_TXLOG_NONE nor REINA_TXLOG_BEFORE),  g = the group of the agent's age.  vd is VALID when
 * 0 <= vd < REINA_MAX_DAYS.  An agent that is neither vac nor inf contributes nothing.
 *
 * STATUS AT INFECTION of an inf agent (REINA_VACC_STATUSES):
 *     0 UNVACCINATED   not vac; or vac, vd valid, t known and vd > t: vaccinated AFTER the infection (the reference vaccinates
 *                      undetected infected and recovered people; such an agent also counts in the scalar AFTER_INFECTION)
 *     1 RECENT         vac, vd valid, t known, 0 <= t - vd <= REINA_VACC_PROTECTION_DAYS
 *     2 PROTECTED      vac, vd valid, t known, t - vd > REINA_VACC_PROTECTION_DAYS.  This is exactly the condition under which
 *                      the infection drew its severity with the factor 0.1: install_infection (csrc/k_common.inc: RH_VACCINATED
 *                      and day - vacc_day > 14 -> vmod = 0.1f), the reference's main.pyx:1051-1055
 *     3 UNDETERMINED   vac and t not known (BEFORE: infected before the log began; NONE: a state whose day is not recorded yet);
 *                      or vac and vd not valid
 * Every vac agent -- infected or not -- whose vd is not valid counts in the scalar BAD_VACC_DAY, which is 0 in every simulated
 * state.
 *
 * THE BLOCK holds REINA_VACC_REPORT_WORDS(n_days) little-endian uint64 words at the offsets below (arrays row-major):
 *   severity[4][16][8]        inf agents by (status, g, sev)
 *   outcome[4][16][4]         inf agents by (status, g): agents, closed (st >= RS_RECOVERED), dead (st == RS_DEAD), detected
 *                             (w & RH_DETECTED)
 *   since[2][16][128]         agents of status 1 or 2 by (k, g, t - vd clipped to 0..127): k = 0 every such agent, k = 1 those
 *                             with sev >= RV_SEVERE -- the step at REINA_VACC_PROTECTION_DAYS made visible
 *   population[16][3]         vac agents by g: all, still susceptible (st == 0), infected (st != 0)
 *   scalars                   REINA_VACC_S_* below
 *   vaccinations[n_days][16]  vac agents by (vd, g), vd valid and < n_days
 *   infections[n_days][16][3] inf agents of status 0..2 by (t, g, status), t known and < n_days
 *   cohort[n_days][3][4]      the same agents by (t, status): agents, sev >= RV_SEVERE, dead (st == RS_DEAD), closed (st >=
 *                             RS_RECOVERED)
 * A valid vd >= n_days (of any vac agent), and a known t >= n_days (of an inf agent of status 0..2), count once each into the
 * scalar OUT_OF_RANGE instead of the tables by day.  The fixed tables take every agent.  So, whatever n_days is:
 *     sum(vaccinations) + (OUT_OF_RANGE's vd part) + BAD_VACC_DAY == VACCINATED == sum(population[.][0])
 *     sum(outcome[.][.][0]) == INFECTED,   sum(outcome[3][.][0]) == UNDETERMINED
 *
 * REFUSED (REINA_E_INVALID + reina_last_error): what reina_txlog_report refuses, through the same checks and in the same words
 * under the prefix "vaccination report" -- an age_group table that is null, n_groups outside 1..REINA_VACC_MAX_GROUPS, an
 * age's group not below n_groups, n_days outside 1..REINA_MAX_DAYS, a report that is not a 16-byte aligned device buffer --
 * and a null log.  Sharded engines cannot have a log. */
#ifndef REINA_VACCINATION_H
#define REINA_VACCINATION_H

#include <stddef.h>
#include <stdint.h>

#include "reina_txlog.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REINA_VACC_VERSION 1
#define REINA_VACC_MAX_GROUPS 16
#define REINA_VACC_STATUSES 4
#define REINA_VACC_DATED_STATUSES 3     /* the statuses of the tables by day: 0..2 */
#define REINA_VACC_PROTECTION_DAYS 14
#define REINA_VACC_SEVERITIES 8         /* RH_SEV has three bits */
#define REINA_VACC_OUTCOME_FIELDS 4     /* agents, closed, dead, detected */
#define REINA_VACC_SINCE_KINDS 2        /* all, sev >= RV_SEVERE */
#define REINA_VACC_SINCE_BINS 128
#define REINA_VACC_POPULATION_FIELDS 3  /* vaccinated, still susceptible, infected */
#define REINA_VACC_COHORT_FIELDS 4      /* agents, severe, dead, closed */

/* the statuses */
#define REINA_VACC_UNVACCINATED 0
#define REINA_VACC_RECENT 1
#define REINA_VACC_PROTECTED 2
#define REINA_VACC_UNDETERMINED 3

/* word offsets of the report block: the fixed part ... */
#define REINA_VACC_SEVERITY 0u
#define REINA_VACC_OUTCOME (REINA_VACC_SEVERITY + REINA_VACC_STATUSES * REINA_VACC_MAX_GROUPS * REINA_VACC_SEVERITIES)
#define REINA_VACC_SINCE (REINA_VACC_OUTCOME + REINA_VACC_STATUSES * REINA_VACC_MAX_GROUPS * REINA_VACC_OUTCOME_FIELDS)
#define REINA_VACC_POPULATION (REINA_VACC_SINCE + REINA_VACC_SINCE_KINDS * REINA_VACC_MAX_GROUPS * REINA_VACC_SINCE_BINS)
#define REINA_VACC_SCALARS (REINA_VACC_POPULATION + REINA_VACC_MAX_GROUPS * REINA_VACC_POPULATION_FIELDS)
enum {
    REINA_VACC_S_VACCINATED = 0,         /* agents with RH_VACCINATED */
    REINA_VACC_S_INFECTED,               /* agents with RH_STATE != 0 */
    REINA_VACC_S_VACCINATED_INFECTED,    /* ... with both */
    REINA_VACC_S_AFTER_INFECTION,        /* status 0 although vaccinated: vd > t */
    REINA_VACC_S_UNDETERMINED,           /* inf agents of status 3 */
    REINA_VACC_S_BAD_VACC_DAY,           /* vac agents whose vd is not valid: 0 in a simulated state */
    REINA_VACC_S_OUT_OF_RANGE,
    REINA_VACC_S_NR = 16
};
/* ... and the tables by day */
#define REINA_VACC_FIXED_WORDS (REINA_VACC_SCALARS + REINA_VACC_S_NR)
#define REINA_VACC_VACCINATIONS(n_days) ((size_t)REINA_VACC_FIXED_WORDS)
#define REINA_VACC_INFECTIONS(n_days) (REINA_VACC_VACCINATIONS(n_days) + (size_t)(n_days) * REINA_VACC_MAX_GROUPS)
#define REINA_VACC_COHORT(n_days) (REINA_VACC_INFECTIONS(n_days) + (size_t)(n_days) * REINA_VACC_MAX_GROUPS * REINA_VACC_DATED_STATUSES)
#define REINA_VACC_DAY_WORDS (REINA_VACC_MAX_GROUPS * (1 + REINA_VACC_DATED_STATUSES) + REINA_VACC_DATED_STATUSES * REINA_VACC_COHORT_FIELDS)   /* 76 */
#define REINA_VACC_REPORT_WORDS(n_days) (REINA_VACC_FIXED_WORDS + (size_t)(n_days) * REINA_VACC_DAY_WORDS)

int reina_vacc_version(void);
/* the report of the days [0, n_days) into dev_report (device, 16-byte aligned, REINA_VACC_REPORT_WORDS(n_days) uint64 words
 * per member, the members' blocks one after the other; overwritten), queued on `stream`: one entry point for a single engine's
 * log and a group's.  age_group: host table [REINA_MAX_AGES] of the group of every age, each < n_groups <=
 * REINA_VACC_MAX_GROUPS.  Reads the engine's state and the log, writes nothing but dev_report, owns no state. */
int reina_vacc_report(reina_txlog_t *log, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days, uint64_t *dev_report,
                      void *stream);

#ifdef __cplusplus
}
#endif

#endif
