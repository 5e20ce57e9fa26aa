/* Lineage reports: who infects whom by period, and the trees of a run by the period they were seeded in (companion of
 * reina_hip.h; same library, same error codes; reina_model_amd/lineage.py: report_numpy is the
 * executable specification).
 *
 * A report is taken between two days, of a transmission log (reina_txlog.h) and the engine state it belongs to.  It joins the
 * two facts the engine and the log keep per infected agent: the tree it belongs to (reina_transmission.h) and the day it was
 * infected (reina_txlog.h).
 *
 * PARAMETERS  period_days in 1..REINA_MAX_DAYS; n_periods = P in 1..REINA_LINEAGE_MAX_PERIODS, Q = P + 1; the table age ->
 * group of the other reports (< REINA_LINEAGE_MAX_GROUPS); max_depth as in reina_tx_report (0: the member's day word + 1, read
 * on the device).
 *
 * PERIOD CLASS of a log half word d:  pc(d) = d / period_days when d is known (neither REINA_TXLOG_NONE nor
 * REINA_TXLOG_BEFORE) and that quotient is < P; otherwise pc(d) = P (before the log, undated or out of range).
 *
 * "Infected", "root", "link", "bad link", "converged" and "tree" are those of reina_transmission.h: a bad link's agent heads a
 * tree of its own; agents whose root is not reached in the rounds run are UNCONVERGED and count in no tree.  t(.) is the log's
 * infection half word.  An agent is ALIVE when RS_INCUBATION <= RH_STATE <= RS_IN_ICU.  With i an infected agent, s its
 * infector on a link and r the root of a converged agent, the block holds REINA_LINEAGE_REPORT_WORDS(P) little-endian uint64
 * words at the offsets below (arrays row-major):
 *   scalars[16]          REINA_LINEAGE_S_* below
 *   seed[Q][4]           by seed class pc(t(r)): trees, trees with an alive converged agent, converged agents, alive converged
 *                        agents
 *   tree_sizes[Q][33]    trees by (seed class, floor(log2(size)))
 *   cohort[Q][16][2]     infected agents by (pc(t(i)), own age group): agents, those with RH_STATE >= RS_RECOVERED
 *   lineage[Q][Q]        converged agents by (seed class of their root, pc(t(i)))
 *   mixing_t[Q][16][16]  links by (pc(t(i)), group of s, group of i): who infects whom by time of transmission
 *   mixing_c[Q][16][16]  links by (pc(t(s)), group of s, group of i): the next-generation counts of the cohort infected then
 *
 * REFUSED (REINA_E_INVALID + reina_last_error): period_days or n_periods out of range, an age's group not below n_groups,
 * scratch or report not 16-byte aligned, a group's log at the single-engine entry point and the other way round.  (Sharded
 * engines are refused when the log is created.) */
#ifndef REINA_LINEAGE_H
#define REINA_LINEAGE_H

#include <stddef.h>
#include <stdint.h>

#include "reina_hip.h"
#include "reina_txlog.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REINA_LINEAGE_VERSION 1
#define REINA_LINEAGE_MAX_PERIODS 256
#define REINA_LINEAGE_MAX_GROUPS 16
#define REINA_LINEAGE_SIZE_BINS 33
#define REINA_LINEAGE_SEED_FIELDS 4     /* trees, alive trees, converged agents, alive converged agents */
#define REINA_LINEAGE_COHORT_FIELDS 2   /* agents, agents removed */

enum {
    REINA_LINEAGE_S_INFECTED = 0,   /* agents with RH_STATE != 0 */
    REINA_LINEAGE_S_LINKS,
    REINA_LINEAGE_S_BAD_LINKS,
    REINA_LINEAGE_S_ROOTS,          /* infector -1 */
    REINA_LINEAGE_S_TREES,          /* heads of trees: roots plus bad-link heads */
    REINA_LINEAGE_S_UNCONVERGED,
    REINA_LINEAGE_S_ROUNDS,         /* pointer-jumping rounds run: ceil(log2(max_depth + 1)) */
    REINA_LINEAGE_S_ALIVE_AGENTS,   /* converged and alive */
    REINA_LINEAGE_S_ALIVE_TREES,    /* trees with at least one alive converged agent */
    REINA_LINEAGE_S_LARGEST_TREE,   /* agents in the largest tree (0: no tree) */
    REINA_LINEAGE_S_LARGEST_ROOT,   /* ... its head; the smallest index on ties; all ones when there is no tree */
    REINA_LINEAGE_S_UNDATED,        /* infected agents with pc(t) = P */
    REINA_LINEAGE_S_LARGEST_KEY,    /* (internal) size << 32 | ~head of the largest tree */
    REINA_LINEAGE_S_NR = 16
};

/* word offsets of the report block: the scalars, then the tables of P periods */
#define REINA_LINEAGE_SCALARS 0u
#define REINA_LINEAGE_SEED(P) ((size_t)REINA_LINEAGE_S_NR)
#define REINA_LINEAGE_TREE_SIZES(P) (REINA_LINEAGE_SEED(P) + ((size_t)(P) + 1u) * REINA_LINEAGE_SEED_FIELDS)
#define REINA_LINEAGE_COHORT(P) (REINA_LINEAGE_TREE_SIZES(P) + ((size_t)(P) + 1u) * REINA_LINEAGE_SIZE_BINS)
#define REINA_LINEAGE_LINEAGE(P) (REINA_LINEAGE_COHORT(P) + ((size_t)(P) + 1u) * REINA_LINEAGE_MAX_GROUPS * REINA_LINEAGE_COHORT_FIELDS)
#define REINA_LINEAGE_MIXING_T(P) (REINA_LINEAGE_LINEAGE(P) + ((size_t)(P) + 1u) * ((size_t)(P) + 1u))
#define REINA_LINEAGE_MIXING_C(P) (REINA_LINEAGE_MIXING_T(P) + ((size_t)(P) + 1u) * REINA_LINEAGE_MAX_GROUPS * REINA_LINEAGE_MAX_GROUPS)
#define REINA_LINEAGE_REPORT_WORDS(P) (REINA_LINEAGE_MIXING_C(P) + ((size_t)(P) + 1u) * REINA_LINEAGE_MAX_GROUPS * REINA_LINEAGE_MAX_GROUPS)

/* Caller-owned device scratch of one report, 16-byte aligned: two buffers of (parent, distance) pairs, the tree sizes and the
 * trees' alive counts.  Everything in it is written before it is read: it needs no initialisation and may be reused. */
#define REINA_LINEAGE_SCRATCH_BYTES(n_agents) ((((size_t)(n_agents) * 24u) + 255u) & ~(size_t)255u)

int reina_lineage_version(void);
/* The report of the log's engine into dev_report (device, 16-byte aligned, REINA_LINEAGE_REPORT_WORDS(n_periods) uint64 words,
 * overwritten), queued on `stream`.  age_group: host table [REINA_MAX_AGES] of the group of every age, each < n_groups <=
 * REINA_LINEAGE_MAX_GROUPS.  Reads the engine's state and the log, writes nothing but dev_scratch and dev_report. */
int reina_lineage_report(reina_txlog_t *log, const uint8_t *age_group, uint32_t n_groups, uint32_t period_days,
                         uint32_t n_periods, uint32_t max_depth, void *dev_scratch, uint64_t *dev_report, void *stream);
/* The same for every member of a group's log, one launch per pass: dev_scratch is a host array of one scratch block per
 * member, dev_report K consecutive report blocks.  Waits for the stream (the member table is freed after the passes). */
int reina_group_lineage_report(reina_txlog_t *log, const uint8_t *age_group, uint32_t n_groups, uint32_t period_days,
                               uint32_t n_periods, uint32_t max_depth, void *const *dev_scratch, uint64_t *dev_report,
                               void *stream);

#ifdef __cplusplus
}
#endif

#endif
