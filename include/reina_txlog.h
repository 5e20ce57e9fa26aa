/* A dated transmission log: the day of infection and the day of symptom onset of every agent (companion of reina_hip.h; same
 * library, same error codes; reina_model_amd/txlog.py: begin_numpy / record_numpy / report_numpy are
 * the executable specification).
 *
 * A LOG is one uint32 per agent, owned by the log object, outside the engine state (snapshots, the counter block and every
 * kernel of a day know nothing of it):
 *
 *     word = onset_day << 16 | infection_day        codes: REINA_TXLOG_NONE (not yet / never), REINA_TXLOG_BEFORE (before the log began)
 *
 * Days are absolute day numbers (reina_day_t.day < REINA_MAX_DAYS = 4096 < REINA_TXLOG_BEFORE).  A day is KNOWN when it is
 * neither code.
 *
 * BEGIN (reina_txlog_create queues it): every agent with RH_STATE(hot) != 0 gets infection BEFORE; of those, the ones with
 * RH_STATE >= RS_ILLNESS get onset BEFORE too; every other half word is NONE.
 *
 * RECORD DAY d (queued behind day d's last launch), for every agent, with w its hot word after day d:
 *     infection == NONE and RH_STATE(w) != 0          ->  infection = d
 *     onset == NONE     and RH_STATE(w) >= RS_ILLNESS ->  onset = d
 * Nothing is ever overwritten.  The definition is observational: it does not depend on how the day's kernels encode their
 * countdowns.  Every day run after the begin pass must be recorded, in order.
 *
 * REPORT, between two days, from the hot words, the cold records' infector and n_infected, the log, the population's
 * age_start and a caller table age -> group (< REINA_TXLOG_MAX_GROUPS), for the days [0, n_days).  "Infected", "root", "link"
 * and "bad link" are those of reina_transmission.h.  With t(.) / o(.) an agent's infection / onset day, v its own variant,
 * i an infected agent and s its infector on a link, the block holds REINA_TXLOG_REPORT_WORDS(n_days) little-endian uint64
 * words at the offsets below (arrays row-major):
 *   incubation[4][64]        o(i) - t(i), both known, clipped to 0..63
 *   generation[4][64]        per link: t(i) - t(s), both known, clipped to 0..63
 *   serial[4][128]           per link: o(i) - o(s) + 32, both known, clipped to 0..127
 *   tost[4][64]              per link: t(i) - o(s) + 24, both known, clipped to 0..63 (time from the infector's onset to transmission)
 *   link_phase[4][4]         per link: 0 t(i) < o(s), both known (presymptomatic transmission); 1 t(i) >= o(s), both known;
 *                            2 t(i) known and o(s) NONE (the infector had not fallen ill by the report); 3 anything else
 *                            (t(i) not known, or o(s) BEFORE)
 *   scalars                  REINA_TXLOG_S_* below
 *   incidence[n_days][4][16] agents by (t, v, group of the agent's age), t known and < n_days
 *   onsets[n_days][4]        agents by (o, v), o known and < n_days
 *   cohort[n_days][4][3]     by (t, v), t known and < n_days: agents, the sum of their n_infected, those with RH_STATE >=
 *                            RS_RECOVERED (how far the cohort is closed: the case reproduction number of an open cohort is
 *                            censored)
 * A known day >= n_days counts into the scalar OUT_OF_RANGE instead of the three dated tables (once per such half word); the
 * interval histograms take every known day.
 *
 * REFUSED (REINA_E_INVALID + reina_last_error): sharded engines and exact attribution (links are global ids, and a shard sees
 * only its own agents' onsets), day >= REINA_MAX_DAYS, n_days outside 1..REINA_MAX_DAYS, an age's group not below n_groups,
 * hot words that are not 16-byte aligned, a group's log used with a single-engine entry point and the other way round. */
#ifndef REINA_TXLOG_H
#define REINA_TXLOG_H

#include <stddef.h>
#include <stdint.h>

#include "reina_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REINA_TXLOG_VERSION 1
#define REINA_TXLOG_NONE 0xFFFFu
#define REINA_TXLOG_BEFORE 0xFFFEu
#define REINA_TXLOG_VARIANTS 4
#define REINA_TXLOG_MAX_GROUPS 16
#define REINA_TXLOG_INCUBATION_BINS 64
#define REINA_TXLOG_GENERATION_BINS 64
#define REINA_TXLOG_SERIAL_BINS 128
#define REINA_TXLOG_SERIAL_SHIFT 32
#define REINA_TXLOG_TOST_BINS 64
#define REINA_TXLOG_TOST_SHIFT 24
#define REINA_TXLOG_PHASES 4
#define REINA_TXLOG_COHORT_FIELDS 3   /* agents, sum of n_infected, agents removed */

/* word offsets of the report block: the fixed part ... */
#define REINA_TXLOG_INCUBATION 0u
#define REINA_TXLOG_GENERATION (REINA_TXLOG_INCUBATION + REINA_TXLOG_VARIANTS * REINA_TXLOG_INCUBATION_BINS)
#define REINA_TXLOG_SERIAL (REINA_TXLOG_GENERATION + REINA_TXLOG_VARIANTS * REINA_TXLOG_GENERATION_BINS)
#define REINA_TXLOG_TOST (REINA_TXLOG_SERIAL + REINA_TXLOG_VARIANTS * REINA_TXLOG_SERIAL_BINS)
#define REINA_TXLOG_LINK_PHASE (REINA_TXLOG_TOST + REINA_TXLOG_VARIANTS * REINA_TXLOG_TOST_BINS)
#define REINA_TXLOG_SCALARS (REINA_TXLOG_LINK_PHASE + REINA_TXLOG_VARIANTS * REINA_TXLOG_PHASES)
enum {
    REINA_TXLOG_S_INFECTED = 0,            /* agents with RH_STATE != 0 */
    REINA_TXLOG_S_DATED,                   /* ... with a known infection day */
    REINA_TXLOG_S_BEFORE,                  /* ... with infection BEFORE */
    REINA_TXLOG_S_WITH_ONSET,              /* ... with a known onset day */
    REINA_TXLOG_S_LINKS,
    REINA_TXLOG_S_LINKS_DATED,             /* links with both infection days known */
    REINA_TXLOG_S_GENERATION_NONPOSITIVE,  /* ... of which t(i) <= t(s): 0 in a simulated state */
    REINA_TXLOG_S_FIRST_DAY,               /* smallest known infection day; all ones when nobody is dated */
    REINA_TXLOG_S_LAST_DAY,                /* largest known infection day; 0 when nobody is dated */
    REINA_TXLOG_S_OUT_OF_RANGE,
    REINA_TXLOG_S_BAD_LINKS,
    REINA_TXLOG_S_NR = 16
};
/* ... and the tables by day */
#define REINA_TXLOG_FIXED_WORDS (REINA_TXLOG_SCALARS + REINA_TXLOG_S_NR)
#define REINA_TXLOG_INCIDENCE(n_days) ((size_t)REINA_TXLOG_FIXED_WORDS)
#define REINA_TXLOG_ONSETS(n_days) (REINA_TXLOG_INCIDENCE(n_days) + (size_t)(n_days) * REINA_TXLOG_VARIANTS * REINA_TXLOG_MAX_GROUPS)
#define REINA_TXLOG_COHORT(n_days) (REINA_TXLOG_ONSETS(n_days) + (size_t)(n_days) * REINA_TXLOG_VARIANTS)
#define REINA_TXLOG_DAY_WORDS (REINA_TXLOG_VARIANTS * (REINA_TXLOG_MAX_GROUPS + 1 + REINA_TXLOG_COHORT_FIELDS))   /* 80 */
#define REINA_TXLOG_REPORT_WORDS(n_days) (REINA_TXLOG_FIXED_WORDS + (size_t)(n_days) * REINA_TXLOG_DAY_WORDS)

typedef struct reina_txlog reina_txlog_t;

int reina_txlog_version(void);
/* a log of one engine / of every member of a group (the engine / group must outlive it): allocates the words and queues the
 * begin pass on `stream` */
int reina_txlog_create(reina_engine_t *e, void *stream, reina_txlog_t **out);
int reina_group_txlog_create(reina_group_t *g, void *stream, reina_txlog_t **out);
int reina_txlog_destroy(reina_txlog_t *log);
/* the one launch of a day, for a caller that steps days itself: queue it behind day `day`'s last launch (a group's log: one
 * launch for all members) */
int reina_txlog_record_day(reina_txlog_t *log, uint32_t day, void *stream);
/* reina_run_days_hist / reina_group_run_days with the record launch queued behind every day (use the one that matches how the
 * log was created).  Always the three-launch day: the several-days-in-one-launch form of a small population has no place
 * between its days. */
int reina_txlog_run_days(reina_txlog_t *log, const reina_day_t *days, uint32_t n_days, int32_t *history_base, void *stream);
int reina_group_txlog_run_days(reina_txlog_t *log, const reina_day_t *days, uint32_t n_days, int32_t *const *history_bases,
                               void *stream);
/* the report of the days [0, n_days) into dev_report (device, 16-byte aligned, REINA_TXLOG_REPORT_WORDS(n_days) uint64 words
 * per member, the members' blocks one after the other; overwritten), queued on `stream`.  age_group: host table
 * [REINA_MAX_AGES] of the group of every age, each < n_groups <= REINA_TXLOG_MAX_GROUPS.  Reads the engine's state and the
 * log, writes nothing but dev_report. */
int reina_txlog_report(reina_txlog_t *log, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days, uint64_t *dev_report,
                       void *stream);
int reina_group_txlog_report(reina_txlog_t *log, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days,
                             uint64_t *dev_report, void *stream);
/* the words of member `member` (0 for a single engine's log) to out_host [n_agents]; synchronises `stream` */
int reina_txlog_read(reina_txlog_t *log, uint32_t member, uint32_t *out_host, void *stream);
/* ... and back: the member's words replaced by in_host [n_agents] (a log saved by reina_txlog_read, continued on the same
 * state); synchronises `stream` */
int reina_txlog_write(reina_txlog_t *log, uint32_t member, const uint32_t *in_host, void *stream);

#ifdef __cplusplus
}
#endif

#endif
