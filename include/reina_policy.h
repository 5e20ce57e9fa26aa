/* Triggered interventions: on-device policies that react to a run's own counters (companion of reina_hip.h; same library,
 * same error codes; reina_model_amd/policy.py: step_numpy is the executable specification).
 *
 * A POLICY is a ladder of L levels (2 <= L <= REINA_POLICY_MAX_LEVELS).  Every level stands for a set of contact tables
 * (the dated tables with the level's undated limit-mobility / wear-masks interventions applied); a rule moves a run up and
 * down the ladder from its own counters.  The decision and the table switch are one kernel, k_policy, queued ahead of every
 * day's opening launch: per member of a group (blockIdx.y), from that member's counter block.  Nothing waits on the host.
 *
 * SIGNAL.  x_now(d) = the sum over the REINA_MAX_AGES words of per-age counter row `signal` (a REINA_C_* index) of the member's
 * counter block BEFORE day d's opening: the values history row d holds.  kind REINA_POLICY_LEVEL: x(d) = x_now(d);
 * REINA_POLICY_INCREMENT over n = n_days days (1..28): x(d) = x_now(d) - x_now(max(d - n, first)), `first` = the first day of
 * the unbroken sequence of days this policy has seen (a policy keeps the last 32 daily values in a ring; a day that does not
 * follow the last one seen starts a new sequence).  int32 arithmetic, integer comparisons.  The tests hold this on rows whose
 * absolute values sum to less than 2^31, where every summation order in int32 gives the same x_now; beyond that domain it is
 * not tested.
 *
 * RULE.  A run starts at level 0.  Day d is a review day when d >= start_day and (d - start_day) % review_every == 0.  On a
 * review day, with l the current level: the run escalates to the highest j > l with x >= up[j - 1], if there is one (jumps
 * allowed); otherwise, if l > 0, x < down[l - 1] and level l has governed at least min_days days, it relaxes to l - 1.  The
 * level decided before day d's opening governs day d.  up[] is non-decreasing and down[j] <= up[j].
 *
 * BANK.  L entries in device memory, each what reina_upload_contact_tables derives from a reina_contact_tables_t (the Tables
 * image and the table-dependent parts of the parameter block).  One bank serves all members.  When a member's level changes,
 * or on the first day after any level was uploaded (a new stretch of dated tables: EVERY member takes its level's entry), the
 * member's workgroups copy the entry's used rows into the member's own tables, which the day's kernels then read as ever.
 *
 * STATE AND TRACE live in buffers the policy owns (the engine's state, its snapshots and counter block know nothing of
 * them).  The trace holds, per member and day (absolute day number < REINA_MAX_DAYS), two int32 words: the level in force
 * that day and x(d).
 *
 * A policy run always takes the three-launch day (the several-days-in-one-launch form of a small population has no place
 * between its days for a decision), and carves k_day's LDS for the most rows any level of the bank holds.
 *
 * REFUSED (REINA_E_INVALID + reina_last_error): sharded engines (the signal would need the all-reduce), exact attribution,
 * L out of range, inconsistent thresholds, an unknown signal row or kind, n_days outside 1..28, review_every = 0, a run
 * with a bank level that was never uploaded. */
#ifndef REINA_POLICY_H
#define REINA_POLICY_H

#include <stdint.h>

#include "reina_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REINA_POLICY_VERSION 1
#define REINA_POLICY_MAX_LEVELS 8
#define REINA_POLICY_RING 32      /* daily signal values a policy keeps (n_days <= 28) */
#define REINA_POLICY_LEVEL 0
#define REINA_POLICY_INCREMENT 1
#define REINA_POLICY_TRACE_WORDS 2   /* per member and day: level in force, x(d) */

typedef struct {
    uint32_t n_levels;      /* L */
    uint32_t signal;        /* REINA_C_* row */
    uint32_t kind;          /* REINA_POLICY_LEVEL / REINA_POLICY_INCREMENT */
    uint32_t n_days;        /* increment: over so many days (1..28) */
    uint32_t review_every;  /* >= 1 */
    uint32_t min_days;      /* days a level must have governed before it is relaxed */
    uint32_t start_day;     /* first review day (absolute day number) */
    uint32_t reserved_;
    int32_t up[REINA_POLICY_MAX_LEVELS];     /* [0 .. L - 2] */
    int32_t down[REINA_POLICY_MAX_LEVELS];   /* [0 .. L - 2] */
} reina_policy_rule_t;

typedef struct reina_policy reina_policy_t;

int reina_policy_version(void);
/* a policy for one engine / for the members of a group (the engine / group must outlive it); every member starts at level 0
 * with an empty ring */
int reina_policy_create(reina_engine_t *e, const reina_policy_rule_t *rule, reina_policy_t **out);
int reina_group_policy_create(reina_group_t *g, const reina_policy_rule_t *rule, reina_policy_t **out);
int reina_policy_destroy(reina_policy_t *p);
/* bank entry `level` from host tables, through the pinned-staging route of reina_upload_contact_tables; queued on `stream`.
 * The next day run gives every member its level's entry. */
int reina_policy_upload_level(reina_policy_t *p, uint32_t level, const reina_contact_tables_t *t, void *stream);
/* reina_run_days_hist / reina_group_run_days with k_policy queued ahead of every day's opening launch (use the one that
 * matches how the policy was created) */
int reina_policy_run_days(reina_policy_t *p, const reina_day_t *days, uint32_t n_days, int32_t *history_base, void *stream);
int reina_group_policy_run_days(reina_policy_t *p, const reina_day_t *days, uint32_t n_days, int32_t *const *history_bases,
                                void *stream);
/* the trace of days [first_day, first_day + n_days) to out_host [members][n_days][REINA_POLICY_TRACE_WORDS]; synchronises
 * `stream`.  When the range ends on the last day run, the members' host-side table mirrors are set from their final levels,
 * so that plain uploads and runs that follow behave as ever: call it once after every policy run. */
int reina_policy_read_trace(reina_policy_t *p, uint32_t first_day, uint32_t n_days, int32_t *out_host, void *stream);

#ifdef __cplusplus
}
#endif

#endif
