/* Particle filters over engine groups (companion of reina_hip.h; same library, same error codes; DESIGN.md "Particle
 * filter").
 *
 * A bootstrap particle filter resamples the members of an engine group between two days: member dst is overwritten by
 * member src's carried state and continues as an independent future under its own seed (the RNG is Philox keyed by the
 * seed, so nothing is reseeded).  Under one plan (make_plan / run_group_plan) the members' host-side scenario state is the
 * same, so only device state moves.
 *
 * Carried state -- the snapshot's inventory (reina_snapshot.h): the hot word, the 32-byte cold record and the inline
 * infectee slots of every agent, both bit planes (the words of the n_tiles 512-agent tiles), the counter block, the control
 * block, and queue0 / queue1 / level1 up to the source's lengths (its control block's REINA_L_QUEUE0.. words, clamped to
 * [0, max_queue]).  Per-day scratch is not copied.
 *
 * The copy is a delta on the invariant a snapshot relies on (hot = 0 => the cold record, claim aside, and the slots are
 * k_init's):
 *   src hot != 0              dst gets src's hot word, cold record (claim included) and slots
 *   src hot = 0, dst hot != 0 dst gets hot 0, k_init's cold record (claim ~0) and slots -1
 *   both 0                    the agent is not touched
 * reina_model_amd/filtering.py: clone_state is the executable specification. */
#ifndef REINA_FILTER_H
#define REINA_FILTER_H

#include <stdint.h>

#include "reina_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REINA_FILTER_VERSION 1
#define REINA_CLONE_MAX_PAIRS 896u   /* pairs per launch (they travel as a kernel argument); longer lists take more launches */

int reina_filter_version(void);
/* For every pair (pairs[2 j], pairs[2 j + 1]) = (dst, src) of member indices, member dst gets member src's carried state:
 * all pairs in one launch (up to REINA_CLONE_MAX_PAIRS), queued on `stream`; no allocation, no host wait.  `pairs` is a
 * host array.  REINA_E_INVALID + reina_last_error, with every member untouched, on an index out of range, a duplicate dst,
 * a src that is also a dst (dst == src included), or members whose testing_ever flags differ. */
int reina_group_clone(reina_group_t *g, const uint32_t *pairs, uint32_t n_pairs, void *stream);

#ifdef __cplusplus
}
#endif

#endif
