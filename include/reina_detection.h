/* A detection report: ascertainment by age, severity and date of infection, transmission before and without detection, and
 * what contact tracing adds (companion of reina_course.h; same library, same error codes; DESIGN.md section 6m;
 * reina_model_amd/detection.py: report_numpy is the executable specification).
 *
 * A report is taken of a course log, and through it of its transmission log -- of one engine, or of the members of a group --
 * between two days.  It keeps no state and changes none: it READS the hot words, the cold records' infector and n_infected (of
 * infected agents), the log words, the course records (of infected agents, and of the infectors of linked agents), the
 * population's age_start and a caller table age -> group (< REINA_DETECT_MAX_GROUPS, the log report's groups), and WRITES the
 * report block alone.
 *
 * PER AGENT with RH_STATE(w) != 0, w the hot word:  st = RH_STATE(w),  sev = RH_SEV(w) (0..7),  g = the group of the agent's
 * age,  n = n_infected,  t and o the log's infection and onset half words,  det, adm and out the record's fields.  A day is
 * KNOWN when it is neither REINA_TXLOG_NONE nor REINA_TXLOG_BEFORE (reina_txlog.h, reina_course.h).  closed: st >=
 * RS_RECOVERED.
 *
 * DETECTION CLASS dc (REINA_DETECT_CLASSES): the record first
 *     1 DATED     det known
 *     2 BEFORE    det BEFORE (detected before the course began -- or removed by then, detected or not: the begin pass closes
 *                 such a record with BEFORE in every field)
 *     3 UNDATED   det NONE and RH_DETECTED (the detection reached the agent after its record closed)
 *     0 NEVER     det NONE and not RH_DETECTED
 *
 * PHASE AT DETECTION ph (REINA_DETECT_PHASES), of dc == 1 only, the first line that applies:
 *     0 before onset            o NONE, or o known and det < o
 *     1 at admission            adm known and det == adm
 *     2 ill, in the community   o known, and adm NONE or (adm known and det < adm)
 *     3 undetermined            anything else
 *
 * LINKS.  Link, root and bad link are those of reina_transmission.h.  Of a link s -> i (s the infector), the LINK CLASS
 * (REINA_DETECT_LINK_CLASSES) is the first line that applies:
 *     0 infector never detected   dc(s) == 0
 *     4 undetermined              dc(s) is 2 or 3, or t(i) not known
 *     1 before detection          t(i) < det(s)
 *     2 same day                  t(i) == det(s)
 *     3 after                     t(i) > det(s): a BREACH of the quarantine -- a detected agent exposes nobody
 *
 * THE BLOCK holds REINA_DETECT_REPORT_WORDS(n_days) little-endian uint64 words at the offsets below (arrays row-major):
 *   ascertain[16][8][4]       agents by (g, sev, dc)
 *   phase[16][4]              agents with dc == 1 by (g, ph)
 *   at_large[16][64]          agents with dc == 1 and t known by (g, det - t clipped to 0..63) ...
 *   at_large_n[16]            ... their number ...
 *   at_large_sum[16]          ... and the sum of det - t before clipping, a two's-complement 64-bit number
 *   offspring[4][2][64]       agents by (dc, closed, min(n, 63))
 *   offspring_sum[4][2]       the sum of n by (dc, closed)
 *   link_class[16][5]         links by (g(s), link class)
 *   lead[16][64]              links of class 1 and 2 by (g(s), det(s) - t(i) clipped to 0..63)
 *   pair[128]                 links with dc(s) == dc(i) == 1 by det(i) - det(s) + REINA_DETECT_PAIR_SHIFT clipped to 0..127
 *   pair_class[4][4]          links by (dc(s), dc(i))
 *   scalars                   REINA_DETECT_S_* below
 *   cohort[n_days][16][3]     agents by (t, g), t known and < n_days: agents, detected (dc != 0), closed
 *   detections[n_days][4]     agents with dc == 1 by (det, ph), det < n_days
 *   links_by_day[n_days][3]   links by t(i), t(i) known and < n_days: links, links of class 0, links of class 1 or 2
 * An agent's known t >= n_days, and the det >= n_days of an agent with dc == 1, count once each into the scalar OUT_OF_RANGE
 * instead of the tables by day (a link's t(i) is its infectee's t: counted there).  The fixed tables take every agent and every
 * link, whatever n_days is.  So:
 *     sum(ascertain) == INFECTED == ROOTS + LINKED + BAD_LINKS,   sum(link_class) == LINKED == sum(pair_class)
 *     sum(ascertain[.][.][dc]) == the scalar of dc,   sum(link_class[.][3]) == BREACH
 *
 * REFUSED (REINA_E_INVALID + reina_last_error): what reina_course_report refuses, through the same checks and in the same words
 * under the prefix "detection report" -- a null course, a course whose log is gone, an age_group table that is null, n_groups
 * outside 1..REINA_DETECT_MAX_GROUPS, an age's group not below n_groups, n_days outside 1..REINA_MAX_DAYS, a report that is not
 * a 16-byte aligned device buffer.  A refused call queues nothing. */
#ifndef REINA_DETECTION_H
#define REINA_DETECTION_H

#include <stddef.h>
#include <stdint.h>

#include "reina_course.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REINA_DETECT_VERSION 1
#define REINA_DETECT_MAX_GROUPS 16
#define REINA_DETECT_SEVERITIES 8       /* RH_SEV has three bits */
#define REINA_DETECT_CLASSES 4          /* never, dated, before, undated */
#define REINA_DETECT_PHASES 4
#define REINA_DETECT_LINK_CLASSES 5
#define REINA_DETECT_BINS 64            /* at_large, offspring and lead */
#define REINA_DETECT_PAIR_BINS 128
#define REINA_DETECT_PAIR_SHIFT 64
#define REINA_DETECT_COHORT_FIELDS 3    /* agents, detected, closed */
#define REINA_DETECT_LINK_DAY_FIELDS 3  /* links, of class 0, of class 1 or 2 */

/* the detection classes */
#define REINA_DETECT_NEVER 0
#define REINA_DETECT_DATED 1
#define REINA_DETECT_BEFORE 2
#define REINA_DETECT_UNDATED 3

/* word offsets of the report block: the fixed part ... */
#define REINA_DETECT_ASCERTAIN 0u
#define REINA_DETECT_PHASE (REINA_DETECT_ASCERTAIN + REINA_DETECT_MAX_GROUPS * REINA_DETECT_SEVERITIES * REINA_DETECT_CLASSES)
#define REINA_DETECT_AT_LARGE (REINA_DETECT_PHASE + REINA_DETECT_MAX_GROUPS * REINA_DETECT_PHASES)
#define REINA_DETECT_AT_LARGE_N (REINA_DETECT_AT_LARGE + REINA_DETECT_MAX_GROUPS * REINA_DETECT_BINS)
#define REINA_DETECT_AT_LARGE_SUM (REINA_DETECT_AT_LARGE_N + REINA_DETECT_MAX_GROUPS)
#define REINA_DETECT_OFFSPRING (REINA_DETECT_AT_LARGE_SUM + REINA_DETECT_MAX_GROUPS)
#define REINA_DETECT_OFFSPRING_SUM (REINA_DETECT_OFFSPRING + REINA_DETECT_CLASSES * 2 * REINA_DETECT_BINS)
#define REINA_DETECT_LINK_CLASS (REINA_DETECT_OFFSPRING_SUM + REINA_DETECT_CLASSES * 2)
#define REINA_DETECT_LEAD (REINA_DETECT_LINK_CLASS + REINA_DETECT_MAX_GROUPS * REINA_DETECT_LINK_CLASSES)
#define REINA_DETECT_PAIR (REINA_DETECT_LEAD + REINA_DETECT_MAX_GROUPS * REINA_DETECT_BINS)
#define REINA_DETECT_PAIR_CLASS (REINA_DETECT_PAIR + REINA_DETECT_PAIR_BINS)
#define REINA_DETECT_SCALARS (REINA_DETECT_PAIR_CLASS + REINA_DETECT_CLASSES * REINA_DETECT_CLASSES)
enum {
    REINA_DETECT_S_INFECTED = 0,         /* agents with RH_STATE != 0 */
    REINA_DETECT_S_ROOTS,                /* ... without an infector */
    REINA_DETECT_S_LINKED,               /* ... with an infector that was infected itself: the links */
    REINA_DETECT_S_BAD_LINKS,            /* ... with anything else in the infector word */
    REINA_DETECT_S_NEVER,                /* agents of dc 0 */
    REINA_DETECT_S_DATED,                /* ... 1 */
    REINA_DETECT_S_BEFORE,               /* ... 2 */
    REINA_DETECT_S_UNDATED,              /* ... 3 */
    REINA_DETECT_S_BREACH,               /* links of class 3: 0 in a simulated state */
    REINA_DETECT_S_OUT_OF_RANGE,
    REINA_DETECT_S_NR = 16
};
/* ... and the tables by day */
#define REINA_DETECT_FIXED_WORDS (REINA_DETECT_SCALARS + REINA_DETECT_S_NR)
#define REINA_DETECT_COHORT(n_days) ((size_t)REINA_DETECT_FIXED_WORDS)
#define REINA_DETECT_DETECTIONS(n_days) (REINA_DETECT_COHORT(n_days) + (size_t)(n_days) * REINA_DETECT_MAX_GROUPS * REINA_DETECT_COHORT_FIELDS)
#define REINA_DETECT_LINKS_BY_DAY(n_days) (REINA_DETECT_DETECTIONS(n_days) + (size_t)(n_days) * REINA_DETECT_PHASES)
#define REINA_DETECT_DAY_WORDS (REINA_DETECT_MAX_GROUPS * REINA_DETECT_COHORT_FIELDS + REINA_DETECT_PHASES + REINA_DETECT_LINK_DAY_FIELDS)   /* 55 */
#define REINA_DETECT_REPORT_WORDS(n_days) (REINA_DETECT_FIXED_WORDS + (size_t)(n_days) * REINA_DETECT_DAY_WORDS)

int reina_detect_version(void);
/* the report of the days [0, n_days) into dev_report (device, 16-byte aligned, REINA_DETECT_REPORT_WORDS(n_days) uint64 words
 * per member, the members' blocks one after the other; overwritten), queued on `stream`: one entry point for a single engine's
 * course and a group's, the arguments in reina_course_report's order.  age_group: host table [REINA_MAX_AGES] of the group of
 * every age, each < n_groups <= REINA_DETECT_MAX_GROUPS.  Reads the engine's state, the log and the course, writes nothing but
 * dev_report, owns no state. */
int reina_detect_report(reina_course_t *course, const uint8_t *age_group, uint32_t n_groups, uint32_t n_days, uint64_t *dev_report,
                        void *stream);

#ifdef __cplusplus
}
#endif

#endif
