/* A policy and a transmission log in one run, and the regime report: transmission by the level in force (companion of
 * reina_policy.h and reina_txlog.h; same library, same error codes; reina_model_amd/regime.py:
 * report_numpy is the executable specification of the report, policy.run_host_driven with a host-kept log that of the run).
 *
 * A. THE RUN.  reina_policy_txlog_run_days / reina_group_policy_txlog_run_days queue, per day and in one stream, exactly the
 * launches of reina_policy_run_days and of reina_txlog_run_days: k_policy ahead of the day's opening launch, the three-launch
 * day, the log's record launch behind its last one (k_txlog_day in the form reina_txlog_run_days would take that day, or
 * k_course_day when a course log is attached to the log).  The logs observe and never steer: history, trace, tables and final
 * state are those of reina_policy_run_days, the log words and course records those of reina_txlog_run_days of the same days.
 *
 * REFUSED (REINA_E_INVALID + reina_last_error) before any day is queued, with state, log and trace untouched: a null policy,
 * log or day list; a policy and a log of which one was made for an engine and the other for a group, or made for different
 * engines or groups; the entry point of the other kind; and everything reina_policy_run_days and reina_txlog_run_days refuse
 * (a day >= REINA_MAX_DAYS, a bank level never uploaded).
 *
 * B. THE REPORT, taken of a transmission log between two days like reina_txlog_report, with one more argument: LABELS, per
 * member uint8[n_days], day -> regime 0..REINA_REGIME_MAX - 1, or REINA_REGIME_NONE for a day without one.  The SLOT of a day d:
 *     labels[d]           when d is known (neither REINA_TXLOG_NONE nor REINA_TXLOG_BEFORE), d < n_days and labels[d] < 8
 *     REINA_REGIME_MAX    otherwise: a day before the log began, a day beyond n_days, an unlabelled day
 * t(.), o(.), v, the group g of an agent's age, "infected", "link", "bad link" and the link phase are those of reina_txlog.h.
 * With i an infected agent, s its infector on a link and r = slot(t(i)) the regime at transmission, the block holds
 * REINA_REGIME_REPORT_WORDS little-endian uint64 words at the offsets below (arrays row-major; 9 = REINA_REGIME_SLOTS):
 *   days[9]               the days d in [0, n_days) by slot(d)
 *   infections[9][4][16]  infected agents by (slot(t(i)), v, g)
 *   cohort[9][4][3]       infected agents by (slot(t(i)), v): agents, the sum of their n_infected, those with RH_STATE >=
 *                         RS_RECOVERED
 *   offspring[9][32]      the agents with RH_STATE >= RS_RECOVERED (closed cases) by (slot(t(i)), min(n_infected, 31))
 *   generation[9][64]     per link: (r, t(i) - t(s) clipped to 0..63), both known
 *   serial[9][128]        per link: (r, o(i) - o(s) + 32 clipped to 0..127), both known
 *   tost[9][64]           per link: (r, t(i) - o(s) + 24 clipped to 0..63), both known
 *   link_phase[9][4]      every link by (r, phase)
 *   crossing[9][9]        every link by (slot(t(s)), slot(t(i)))
 *   mixing[9][16][16]     every link by (r, g(s), g(i))
 *   scalars[8]            REINA_REGIME_S_* below
 * The block has no tables by day: its size does not depend on n_days.  Whatever the labels are:
 *     sum(crossing) == LINKS == sum(link_phase) == sum(mixing),    sum(infections) == INFECTED,
 *     sum(infections[r < 8]) == IN_RANGE - UNLABELLED,             sum(days) == n_days
 *
 * REFUSED (REINA_E_INVALID + reina_last_error): what reina_txlog_report refuses, through the same checks, in the same order and
 * in the same words under the prefix "regime report"; then null labels, a label that is neither below REINA_REGIME_MAX nor
 * REINA_REGIME_NONE, and more label bytes (members x n_days rounded up to 16) than REINA_REGIME_STAGE_BYTES.  A null log; a
 * group's log used with the single-engine entry point and the other way round.  A refused call queues nothing. */
#ifndef REINA_REGIME_H
#define REINA_REGIME_H

#include <stddef.h>
#include <stdint.h>

#include "reina_policy.h"
#include "reina_txlog.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REINA_REGIME_VERSION 1
#define REINA_REGIME_MAX 8                 /* regimes: REINA_POLICY_MAX_LEVELS */
#define REINA_REGIME_SLOTS (REINA_REGIME_MAX + 1)   /* ... and the slot of everything without one */
#define REINA_REGIME_NONE 0xFFu            /* the label of a day without a regime */
#define REINA_REGIME_MAX_GROUPS 16         /* the log report's groups */
#define REINA_REGIME_VARIANTS 4
#define REINA_REGIME_COHORT_FIELDS 3       /* agents, sum of n_infected, removed */
#define REINA_REGIME_OFFSPRING_BINS 32
#define REINA_REGIME_GENERATION_BINS 64
#define REINA_REGIME_SERIAL_BINS 128
#define REINA_REGIME_TOST_BINS 64
#define REINA_REGIME_PHASES 4
#define REINA_REGIME_STAGE_BYTES (1u << 20)   /* the labels of one call: members x (n_days rounded up to 16) bytes at most */

/* word offsets of the report block */
#define REINA_REGIME_DAYS 0u
#define REINA_REGIME_INFECTIONS (REINA_REGIME_DAYS + REINA_REGIME_SLOTS)
#define REINA_REGIME_COHORT (REINA_REGIME_INFECTIONS + REINA_REGIME_SLOTS * REINA_REGIME_VARIANTS * REINA_REGIME_MAX_GROUPS)
#define REINA_REGIME_OFFSPRING (REINA_REGIME_COHORT + REINA_REGIME_SLOTS * REINA_REGIME_VARIANTS * REINA_REGIME_COHORT_FIELDS)
#define REINA_REGIME_GENERATION (REINA_REGIME_OFFSPRING + REINA_REGIME_SLOTS * REINA_REGIME_OFFSPRING_BINS)
#define REINA_REGIME_SERIAL (REINA_REGIME_GENERATION + REINA_REGIME_SLOTS * REINA_REGIME_GENERATION_BINS)
#define REINA_REGIME_TOST (REINA_REGIME_SERIAL + REINA_REGIME_SLOTS * REINA_REGIME_SERIAL_BINS)
#define REINA_REGIME_LINK_PHASE (REINA_REGIME_TOST + REINA_REGIME_SLOTS * REINA_REGIME_TOST_BINS)
#define REINA_REGIME_CROSSING (REINA_REGIME_LINK_PHASE + REINA_REGIME_SLOTS * REINA_REGIME_PHASES)
#define REINA_REGIME_MIXING (REINA_REGIME_CROSSING + REINA_REGIME_SLOTS * REINA_REGIME_SLOTS)
#define REINA_REGIME_SCALARS (REINA_REGIME_MIXING + REINA_REGIME_SLOTS * REINA_REGIME_MAX_GROUPS * REINA_REGIME_MAX_GROUPS)
enum {
    REINA_REGIME_S_INFECTED = 0,     /* agents with RH_STATE != 0 */
    REINA_REGIME_S_DATED,            /* ... whose t is known */
    REINA_REGIME_S_IN_RANGE,         /* ... and < n_days */
    REINA_REGIME_S_UNLABELLED,       /* ... on a day whose label is not below REINA_REGIME_MAX */
    REINA_REGIME_S_LINKS,
    REINA_REGIME_S_LINKS_DATED,      /* links with t(i) and t(s) known */
    REINA_REGIME_S_LINKS_CROSSING,   /* links with slot(t(s)) and slot(t(i)) below REINA_REGIME_MAX and different */
    REINA_REGIME_S_BAD_LINKS,
    REINA_REGIME_S_NR = 8
};
#define REINA_REGIME_REPORT_WORDS (REINA_REGIME_SCALARS + REINA_REGIME_S_NR)   /* 5714 */

int reina_regime_version(void);

/* n_days days under the policy with the log's record launch behind every day, queued on `stream`; arguments as
 * reina_policy_run_days / reina_group_policy_run_days.  `p` and `log` were made for the same engine (the same group). */
int reina_policy_txlog_run_days(reina_policy_t *p, reina_txlog_t *log, const reina_day_t *days, uint32_t n_days,
                                int32_t *history_base, void *stream);
int reina_group_policy_txlog_run_days(reina_policy_t *p, reina_txlog_t *log, const reina_day_t *days, uint32_t n_days,
                                      int32_t *const *history_bases, void *stream);

/* the report into dev_report (device, 16-byte aligned, REINA_REGIME_REPORT_WORDS uint64 words per member, the members' blocks
 * one after the other; overwritten), queued on `stream` as one launch for all members.  age_group, n_groups, n_days: as
 * reina_txlog_report.  labels: host, [members][n_days], copied before the call returns (staged in page-locked memory the
 * library keeps and copied on `stream` into a device buffer the log owns, made by its first report: nothing is allocated per
 * call after that and the host does not wait for the stream).  Reads the engine's state and the log, writes nothing but
 * dev_report. */
int reina_regime_report(reina_txlog_t *log, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days, const uint8_t *labels,
                        uint64_t *dev_report, void *stream);
int reina_group_regime_report(reina_txlog_t *log, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days, const uint8_t *labels,
                              uint64_t *dev_report, void *stream);

#ifdef __cplusplus
}
#endif

#endif
