/* A clinical course log: the day of detection, of admission, of ICU admission and of the outcome of every agent (companion of
 * reina_txlog.h; same library, same error codes; reina_model_amd/course.py: begin_numpy / record_numpy /
 * report_numpy are the executable specification).
 *
 * A COURSE RECORD is one uint64 per agent, owned by the course log, outside the engine state (snapshots, the counter block and
 * every kernel of a day know nothing of it):
 *
 *     record = detection_day | admission_day << 16 | icu_day << 32 | outcome_day << 48
 *
 * Each field is an absolute day number (reina_day_t.day < REINA_MAX_DAYS) or one of the transmission log's codes,
 * REINA_TXLOG_NONE (not yet / never) and REINA_TXLOG_BEFORE (before the course log began).  A field is KNOWN when it is neither.
 *
 * A course log is ATTACHED TO A TRANSMISSION LOG (reina_course_create; the log must outlive it; one course a log): it takes the
 * log's form -- one engine or the members of a group -- and from then on every record launch of that log (reina_txlog_record_day,
 * both *_txlog_run_days) records the course in the same launch.  A report reads the log's infection and onset days.
 *
 * BEGIN (reina_course_create queues it), with w the hot word and st = RH_STATE(w):
 *     st >= RS_RECOVERED                       ->  all four fields BEFORE (the record is closed, its past unknown)
 *     otherwise   detection  BEFORE when st != 0 and w & RH_DETECTED,              else NONE
 *                 admission  BEFORE when st is RS_HOSPITALIZED or RS_IN_ICU,       else NONE
 *                 icu        BEFORE when st == RS_IN_ICU,                          else NONE
 *                 outcome    NONE
 *
 * RECORD DAY d (in the log's record launch of day d), for every agent, with w its hot word after day d and r its record:
 *     outcome(r) != NONE or st == 0  ->  nothing is written.  Otherwise every field that is still NONE gets d when
 *         detection  w & RH_DETECTED
 *         admission  st is RS_HOSPITALIZED or RS_IN_ICU
 *         icu        st == RS_IN_ICU
 *         outcome    st >= RS_RECOVERED
 * Nothing is ever overwritten.  A record CLOSES WITH ITS OUTCOME: a detection that reaches an agent after its outcome day
 * (contact tracing queues infectees whatever their state) is not dated; the report counts such agents in DETECTED_UNDATED.
 * The kind of outcome is not stored: the report reads it from the hot word (RS_DEAD or RS_RECOVERED, RH_POD_OUTSIDE).
 * The definition is observational: it does not depend on how the day's kernels encode their countdowns.
 *
 * REPORT, between two days, from the hot words, the log, the records, the population's age_start and a caller table age ->
 * group (< REINA_COURSE_MAX_GROUPS), for the days [0, n_days).  Every agent with st != 0 is counted.  g is the group of the
 * agent's age, t / o its infection / onset day (the log), det / adm / icu / out its record's fields.  The block holds
 * REINA_COURSE_REPORT_WORDS(n_days) little-endian uint64 words at the offsets below (arrays row-major):
 *   delay[8][16][64]     by (kind, g, value clipped to 0..63); a kind counts the agents for which the days it names are known:
 *                          0 det - o + 16 (tracing can detect before onset)     1 adm - o      2 icu - adm
 *                          3 out - adm, icu NONE, st == RS_RECOVERED            4 the same, st == RS_DEAD
 *                          5 out - icu, st == RS_RECOVERED                      6 the same, st == RS_DEAD
 *                          7 out - o, st == RS_DEAD
 *   delay_n[8][16]       the agents of every (kind, g) ...
 *   delay_sum[8][16]     ... and the sum of their values before clipping (kind 0: of det - o + 16), as a two's-complement
 *                        64-bit number: means stay exact where the histogram clips
 *   pathway[16][10]      by (g, class):  9 (undetermined) when adm, icu or out is BEFORE, or out is known and st < RS_RECOVERED
 *                        (no recorded state); otherwise  outcome: open (out NONE) 0..2, st == RS_RECOVERED 3..5, st == RS_DEAD
 *                        6..8,  plus  0 never admitted (adm and icu NONE), 1 admitted, no ICU (icu NONE), 2 ICU reached
 *   scalars              REINA_COURSE_S_* below
 *   detections[n_days][16], admissions, icu_admissions   by (det | adm | icu, g), the day known and < n_days
 *   deaths[n_days][16], recoveries[n_days][16]           by (out, g), out known and < n_days, st == RS_DEAD | RS_RECOVERED
 *   cohort[n_days][16][4]                                by (t, g), t known and < n_days: agents, closed (st >= RS_RECOVERED),
 *                                                        admitted (adm known), dead (st == RS_DEAD)
 * A known record field >= n_days counts into the scalar OUT_OF_RANGE (once per field) instead of the tables by day; the delay
 * tables and the pathways take every known day.
 *
 * REFUSED (REINA_E_INVALID + reina_last_error): what reina_txlog.h refuses (sharded engines through the log they cannot
 * have, n_days outside 1..REINA_MAX_DAYS, an age's group not below n_groups, a report that is not a 16-byte aligned device
 * buffer), a second course on one log, member out of range. */
#ifndef REINA_COURSE_H
#define REINA_COURSE_H

#include <stddef.h>
#include <stdint.h>

#include "reina_txlog.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REINA_COURSE_VERSION 1
#define REINA_COURSE_MAX_GROUPS 16
#define REINA_COURSE_KINDS 8
#define REINA_COURSE_DELAY_BINS 64
#define REINA_COURSE_DETECTION_SHIFT 16
#define REINA_COURSE_CLASSES 10
#define REINA_COURSE_DAY_TABLES 5      /* detections, admissions, icu_admissions, deaths, recoveries */
#define REINA_COURSE_COHORT_FIELDS 4   /* agents, closed, admitted, dead */

/* the record's fields: the bit each begins at */
#define REINA_COURSE_F_DETECTION 0
#define REINA_COURSE_F_ADMISSION 16
#define REINA_COURSE_F_ICU 32
#define REINA_COURSE_F_OUTCOME 48

/* word offsets of the report block: the fixed part ... */
#define REINA_COURSE_DELAY 0u
#define REINA_COURSE_DELAY_N (REINA_COURSE_DELAY + REINA_COURSE_KINDS * REINA_COURSE_MAX_GROUPS * REINA_COURSE_DELAY_BINS)
#define REINA_COURSE_DELAY_SUM (REINA_COURSE_DELAY_N + REINA_COURSE_KINDS * REINA_COURSE_MAX_GROUPS)
#define REINA_COURSE_PATHWAY (REINA_COURSE_DELAY_SUM + REINA_COURSE_KINDS * REINA_COURSE_MAX_GROUPS)
#define REINA_COURSE_SCALARS (REINA_COURSE_PATHWAY + REINA_COURSE_MAX_GROUPS * REINA_COURSE_CLASSES)
enum {
    REINA_COURSE_S_INFECTED = 0,        /* agents with RH_STATE != 0 */
    REINA_COURSE_S_WITH_DETECTION,      /* ... with a known detection day */
    REINA_COURSE_S_WITH_ADMISSION,      /* ... admission day */
    REINA_COURSE_S_WITH_ICU,            /* ... ICU day */
    REINA_COURSE_S_WITH_OUTCOME,        /* ... outcome day */
    REINA_COURSE_S_DETECTED_UNDATED,    /* RH_DETECTED set and detection NONE: detected after the record closed */
    REINA_COURSE_S_OUT_OF_RANGE,
    REINA_COURSE_S_DIED_OUTSIDE,        /* st == RS_DEAD with RH_POD_OUTSIDE */
    REINA_COURSE_S_NR = 16
};
/* ... and the tables by day */
#define REINA_COURSE_FIXED_WORDS (REINA_COURSE_SCALARS + REINA_COURSE_S_NR)
#define REINA_COURSE_DETECTIONS(n_days) ((size_t)REINA_COURSE_FIXED_WORDS)
#define REINA_COURSE_ADMISSIONS(n_days) (REINA_COURSE_DETECTIONS(n_days) + (size_t)(n_days) * REINA_COURSE_MAX_GROUPS)
#define REINA_COURSE_ICU_ADMISSIONS(n_days) (REINA_COURSE_ADMISSIONS(n_days) + (size_t)(n_days) * REINA_COURSE_MAX_GROUPS)
#define REINA_COURSE_DEATHS(n_days) (REINA_COURSE_ICU_ADMISSIONS(n_days) + (size_t)(n_days) * REINA_COURSE_MAX_GROUPS)
#define REINA_COURSE_RECOVERIES(n_days) (REINA_COURSE_DEATHS(n_days) + (size_t)(n_days) * REINA_COURSE_MAX_GROUPS)
#define REINA_COURSE_COHORT(n_days) (REINA_COURSE_RECOVERIES(n_days) + (size_t)(n_days) * REINA_COURSE_MAX_GROUPS)
#define REINA_COURSE_DAY_WORDS (REINA_COURSE_MAX_GROUPS * (REINA_COURSE_DAY_TABLES + REINA_COURSE_COHORT_FIELDS))   /* 144 */
#define REINA_COURSE_REPORT_WORDS(n_days) (REINA_COURSE_FIXED_WORDS + (size_t)(n_days) * REINA_COURSE_DAY_WORDS)

typedef struct reina_course reina_course_t;

int reina_course_version(void);
/* a course log attached to `log` (of one engine or of a group; it must outlive the course): allocates the records and queues
 * the begin pass on `stream`.  From here on the log's record launches record the course too. */
int reina_course_create(reina_txlog_t *log, void *stream, reina_course_t **out);
/* detaches it: the log records alone again */
int reina_course_destroy(reina_course_t *course);
/* the report of the days [0, n_days) into dev_report (device, 16-byte aligned, REINA_COURSE_REPORT_WORDS(n_days) uint64 words
 * per member, the members' blocks one after the other; overwritten), queued on `stream`: one entry point for a single engine's
 * course and a group's.  age_group: host table [REINA_MAX_AGES] of the group of every age, each < n_groups <=
 * REINA_COURSE_MAX_GROUPS.  Reads the engine's state, the log and the records, writes nothing but dev_report. */
int reina_course_report(reina_course_t *course, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days, uint64_t *dev_report,
                        void *stream);
/* the records of member `member` (0 for a single engine's) to out_host [n_agents]; synchronises `stream` */
int reina_course_read(reina_course_t *course, uint32_t member, uint64_t *out_host, void *stream);
/* ... and back: the member's records replaced by in_host [n_agents]; synchronises `stream` */
int reina_course_write(reina_course_t *course, uint32_t member, const uint64_t *in_host, void *stream);

#ifdef __cplusplus
}
#endif

#endif
