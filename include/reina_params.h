/* Per-member disease parameters of an engine group (companion of reina_hip.h; same library, same error codes; DESIGN.md
 * section 6p "Parameters per particle").
 *
 * Every member of an engine group reads the disease through a parameter block of its own.  A `reina_params_t` keeps one BASE
 * disease and a table of up to REINA_PARAMS_MAX_KNOBS knobs; a knob scales one field of reina_disease_t on some of its cells.
 * reina_group_params_set hands every listed member a vector theta of one multiplier per knob, and one launch (k_group_params)
 * expands base and theta into the members' device blocks before the next day runs.
 *
 * THE RULE (reina_model_amd/parameters.py: expand_numpy is the same rule in numpy):
 *   a cell a knob covers      base * theta, one float32 multiplication; for the probabilities -- the fields whose name
 *                             begins with p_, but p_susceptibility -- the product is then clamped to 1.0f.
 *                             (p_susceptibility is a RELATIVE susceptibility: the default scenario's reaches 1.47, and the
 *                             day's kernels use it only as p_susceptibility / psus_max and psus_max * multiplier.  It is
 *                             scaled and not clamped.)
 *   a cell no knob covers     the base's, and never written
 *   psus_max[v]               the maximum over a < nr_ages of the new p_susceptibility[v][a], from 0.0f, as reina_create
 *                             computes it (written for the variants a p_susceptibility knob covers)
 * theta = 1 reproduces the base bit for bit (base probabilities above 1 are refused); two knobs never cover one cell, so
 * the order of the knobs cannot matter.  infectiousness_over_time, the mask fields, the ratios and the import classes
 * are no knobs. */
#ifndef REINA_PARAMS_H
#define REINA_PARAMS_H

#include <stdint.h>

#include "reina_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REINA_PARAMS_VERSION 1
#define REINA_PARAMS_MAX_KNOBS 8

/* reina_knob_t.field, in the order of reina_disease_t */
enum {
    /* per variant: `variants` picks them, age_lo = age_hi = 0 */
    REINA_PF_INFECTIOUSNESS_MULTIPLIER = 0, REINA_PF_P_ASYMPTOMATIC_INFECTION, REINA_PF_P_HOSPITAL_DEATH_NO_BEDS,
    REINA_PF_P_ICU_DEATH_NO_BEDS, REINA_PF_MEAN_INCUBATION_DURATION, REINA_PF_MEAN_DURATION_FROM_ONSET_TO_DEATH,
    REINA_PF_MEAN_DURATION_FROM_ONSET_TO_RECOVERY,
    /* per variant and age */
    REINA_PF_P_SUSCEPTIBILITY,
    /* per age: `variants` must be 0 */
    REINA_PF_P_SYMPTOMATIC, REINA_PF_P_SEVERE_GIVEN_SYMPTOMATIC, REINA_PF_P_CRITICAL_GIVEN_SEVERE,
    REINA_PF_P_FATAL_GIVEN_CRITICAL, REINA_PF_P_DEATH_OUTSIDE_HOSPITAL,
    REINA_PF_NR
};

typedef struct {
    uint32_t field;             /* REINA_PF_* */
    uint32_t variants;          /* bit mask over [0, nr_variants) */
    uint32_t age_lo, age_hi;    /* inclusive; per-age fields only */
} reina_knob_t;

/* Members and their theta travel as the kernel argument: REINA_PARAMS_CHUNK_WORDS 32-bit words a launch, 1 + n_knobs a
 * member, so one launch serves REINA_PARAMS_CHUNK(n_knobs) members (432 with one knob, 172 with four, 96 with eight) and
 * a longer list takes more launches. */
#define REINA_PARAMS_CHUNK_WORDS 864u
#define REINA_PARAMS_CHUNK(n_knobs) (REINA_PARAMS_CHUNK_WORDS / (1u + (n_knobs)))

typedef struct reina_params reina_params_t;

int reina_params_version(void);
/* Keeps a device copy of `base` and of the knob table for the group.  REINA_E_INVALID + reina_last_error on: a member whose
 * current disease is not `base` byte for byte; sharded members; n_knobs of 0 or above REINA_PARAMS_MAX_KNOBS; an unknown
 * field; a per-variant knob without a variant or with a variant bit at or above nr_variants; a per-age knob with variant
 * bits; an age range outside [0, nr_ages) or reversed (a per-variant scalar's ages must be 0); two knobs that cover a
 * common cell; a base probability (a clamped field, above) that is not in [0, 1]; a base p_susceptibility that is negative
 * or not finite. */
int reina_group_params_create(reina_group_t *g, const reina_disease_t *base, const reina_knob_t *knobs, uint32_t n_knobs,
                              reina_params_t **out);
int reina_group_params_destroy(reina_params_t *p);
/* Member members[j] gets theta[j * n_knobs .. ]: queued on `stream`, REINA_PARAMS_CHUNK(n_knobs) members a launch; no
 * allocation, no host wait, no per-member copy.  `members` and `theta` are host arrays.  The listed members' host mirrors
 * (what a snapshot's disease hash and a later table upload see) follow in the same call, by the same rule.
 * REINA_E_INVALID + reina_last_error, before anything is queued and with every block untouched, on a member out of range,
 * a member listed twice, and a theta that is negative, NaN or infinite. */
int reina_group_params_set(reina_params_t *p, const uint32_t *members, uint32_t n, const float *theta, void *stream);
/* For inspection and tests: copies member's DEVICE block to `out` and its psus_max [REINA_MAX_VARIANTS] to `psus_max_out`
 * (host pointers) and synchronises `stream`. */
int reina_group_params_read(reina_params_t *p, uint32_t member, reina_disease_t *out, float *psus_max_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif
