/* Transmission-tree reports of an engine's state between two days (companion of reina_hip.h; same library, same error codes).
 *
 * The engine keeps every agent's true infector (reina_cold_t.infector, -1 for imports and the initial condition) and its count
 * of secondary infections (reina_cold_t.n_infected).  A report turns them into exact integer counts (DESIGN.md "Transmission
 * reports"), taken between two days of an UNSHARDED engine.  With w = hot[i], an agent is infected when RH_STATE(w) != 0; for
 * every infected agent:
 *   variant   RH_VARIANT(w) (0..3);  severity  min(RH_SEV(w), 4) (0..4)
 *   outcome   0 active (INCUBATION .. IN_ICU), 1 removed and counted into R (state >= RECOVERED with RH_INCLUDED),
 *             2 removed, not yet counted
 *   detected  RH_DETECTED (0 / 1)
 *   link      infector -1: a ROOT.  An infector out of [0, n_agents), equal to the agent itself or not infected is a BAD link:
 *             the agent is cut from it and heads a tree of its own (generation 0; not counted in n_roots).  Any other infector
 *             is a LINK (n_linked).
 *   root      the agent reached by following links; generation = number of links followed (a root: 0).  Agents whose root is
 *             not reached within the rounds run (a chain deeper than max_depth, or a cycle of links) are UNCONVERGED: they
 *             count in no generation and in no tree.
 *   age group a caller table age -> group (< REINA_TX_MAX_GROUPS) for the age of the agent and of its infector.
 *
 * The report block holds REINA_TX_REPORT_WORDS little-endian uint64 words at the offsets below (arrays row-major):
 *   offspring[4][5][3][2][64]  infected agents by (variant, severity, outcome, detected, min(n_infected, 63))
 *   offspring_sum[4][3], offspring_sumsq[4][3]  sum of n_infected and of its square by (variant, outcome)
 *   matrix[4][16][16]          linked agents by (own variant, infector's age group, own age group)
 *   generations[4][256]        converged infected agents by (variant, min(generation, 255))
 *   clusters[33], cluster_agents[33]  trees, and the agents in them, by floor(log2(tree size))
 *   scalars                    REINA_TX_S_* below
 *
 * Sharded engines are refused (REINA_E_INVALID): mirror attribution keeps stand-in infectors, exact attribution global ids. */
#ifndef REINA_TRANSMISSION_H
#define REINA_TRANSMISSION_H

#include <stddef.h>
#include <stdint.h>

#include "reina_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REINA_TX_VERSION 1
#define REINA_TX_VARIANTS 4
#define REINA_TX_SEVERITIES 5
#define REINA_TX_OUTCOMES 3
#define REINA_TX_BINS 64              /* offspring bins: n_infected 0..62, and 63 for 63 or more */
#define REINA_TX_MAX_GROUPS 16
#define REINA_TX_GENERATIONS 256      /* generation bins: 0..254, and 255 for 255 or more */
#define REINA_TX_CLUSTER_BINS 33

/* word offsets of the report block */
#define REINA_TX_OFFSPRING 0u
#define REINA_TX_OFFSPRING_SUM (REINA_TX_OFFSPRING + REINA_TX_VARIANTS * REINA_TX_SEVERITIES * REINA_TX_OUTCOMES * 2u * REINA_TX_BINS)
#define REINA_TX_OFFSPRING_SUMSQ (REINA_TX_OFFSPRING_SUM + REINA_TX_VARIANTS * REINA_TX_OUTCOMES)
#define REINA_TX_MATRIX (REINA_TX_OFFSPRING_SUMSQ + REINA_TX_VARIANTS * REINA_TX_OUTCOMES)
#define REINA_TX_GENERATION (REINA_TX_MATRIX + REINA_TX_VARIANTS * REINA_TX_MAX_GROUPS * REINA_TX_MAX_GROUPS)
#define REINA_TX_CLUSTERS (REINA_TX_GENERATION + REINA_TX_VARIANTS * REINA_TX_GENERATIONS)
#define REINA_TX_CLUSTER_AGENTS (REINA_TX_CLUSTERS + REINA_TX_CLUSTER_BINS)
#define REINA_TX_SCALARS (REINA_TX_CLUSTER_AGENTS + REINA_TX_CLUSTER_BINS)
enum {
    REINA_TX_S_N_INFECTED_AGENTS = 0, REINA_TX_S_N_ROOTS, REINA_TX_S_N_LINKED, REINA_TX_S_SUM_N_INFECTED,
    REINA_TX_S_MAX_GENERATION,
    REINA_TX_S_LARGEST_CLUSTER,       /* agents in the largest tree (0: no tree) */
    REINA_TX_S_LARGEST_ROOT,          /* ... its root; the smallest root index on ties; all ones when there is no tree */
    REINA_TX_S_BAD_LINKS, REINA_TX_S_UNCONVERGED,
    REINA_TX_S_ROUNDS,                /* pointer-jumping rounds run: ceil(log2(max_depth + 1)) */
    REINA_TX_S_LARGEST_KEY,           /* (internal) size << 32 | ~root of the largest tree */
    REINA_TX_S_NR = 16
};
#define REINA_TX_REPORT_WORDS (REINA_TX_SCALARS + REINA_TX_S_NR)

/* Caller-owned device scratch of one report, 16-byte aligned: two buffers of (parent, distance) pairs and the tree sizes.
 * Everything in it is written before it is read: it needs no initialisation and may be reused. */
#define REINA_TX_SCRATCH_BYTES(n_agents) ((((size_t)(n_agents) * 20u) + 255u) & ~(size_t)255u)

int reina_tx_version(void);
/* The report of engine `e` into dev_report (device, REINA_TX_REPORT_WORDS uint64 words, overwritten), queued on `stream`.
 * age_group: host table [REINA_MAX_AGES] of the group of every age, each < n_groups <= REINA_TX_MAX_GROUPS.
 * max_depth: the deepest generation to resolve; 0 = the engine's counter word REINA_S_DAY + 1 (an agent infected on day d
 * infects nobody before day d + 1, so no chain is deeper after the days run), read on the device: at most 13 rounds.
 * Reads the engine's state, writes nothing but dev_scratch and dev_report. */
int reina_tx_report(reina_engine_t *e, const uint8_t *age_group, uint32_t n_groups, uint32_t max_depth, void *dev_scratch,
                    uint64_t *dev_report, void *stream);
/* The same for every member of an engine group, one launch per pass: dev_scratch is a host array of one scratch block per
 * member, dev_report K consecutive report blocks.  Waits for the stream (the member table is freed after the passes). */
int reina_group_tx_report(reina_group_t *g, const uint8_t *age_group, uint32_t n_groups, uint32_t max_depth,
                          void *const *dev_scratch, uint64_t *dev_report, void *stream);

#ifdef __cplusplus
}
#endif

#endif
