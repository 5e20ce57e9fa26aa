/* Snapshots of an engine's state between two days (companion of reina_hip.h; same library, same error codes).
 *
 * A snapshot ("image") is one contiguous little-endian byte block of 32-bit words, taken after day d - 1 has finished and
 * before day d opens, of an UNSHARDED engine.  Layout, in words (REINA_SNAP_* below, DESIGN.md "Snapshots"):
 *
 *   [0, 64)             header: REINA_SNAP_H_* words
 *   counters            REINA_COUNTER_WORDS, verbatim
 *   control             REINA_L_NR, verbatim
 *   base tile table     n_tiles + 1 exclusive offsets (records of 512-agent tile t: [tb[t], tb[t + 1]))
 *   slot tile table     n_tiles + 1 exclusive offsets into the slot stream
 *   (zero words up to a multiple of 8)
 *   base records        n_base x 8 words: index | has_slots << 31, hot, infector, n_infected, onset_days bits, vacc_day,
 *                       first_infectee, next_sibling -- one per agent whose hot word is non-zero, in agent order
 *   slot records        n_slot x 8 words: the REINA_INLINE_INFECTEES inline infectee slots of the base records flagged
 *                       has_slots, in the same order
 *   queues              queue0[len_q0], queue1[len_q1], level1[len_l1]
 *
 * Everything else is restored from k_init's defaults: an agent without a record has hot 0, the cold record
 * {claim ~0, infector -1, n_infected 0, onset 0.0, vacc_day -1, first_infectee -1, next_sibling -1} and slots -1; every
 * agent's claim is restored as ~0; the bit planes are rebuilt from the hot words; per-day scratch (work lists, candidates,
 * bed / ICU events, scan lists and k_vaccinate's chain words) stays as reina_init_state left it.  So an image is restored
 * into an engine that reina_init_state has initialised and that has not stepped a day. */
#ifndef REINA_SNAPSHOT_H
#define REINA_SNAPSHOT_H

#include <stdint.h>

#include "reina_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REINA_SNAPSHOT_VERSION 2   /* 2: the FNV-1a 64 hashes of the header with the standard offset basis (1 had a wrong one) */
#define REINA_SNAP_MAGIC 0x504E5352u   /* "RSNP" */
#define REINA_SNAP_TILE 512u           /* agents per tile of the offset tables (k_day's wave tiles) */
#define REINA_SNAP_HEADER_WORDS 64u
#define REINA_SNAP_RECORD_WORDS 8u

/* header words */
enum {
    REINA_SNAP_H_MAGIC = 0, REINA_SNAP_H_VERSION, REINA_SNAP_H_N_AGENTS, REINA_SNAP_H_NR_AGES, REINA_SNAP_H_NR_VARIANTS,
    REINA_SNAP_H_N_TILES, REINA_SNAP_H_N_BASE, REINA_SNAP_H_N_SLOT,
    REINA_SNAP_H_FLAGS,                     /* bit 0: the engine has run a day with testing on (selects the day-opening form) */
    REINA_SNAP_H_LEN_Q0, REINA_SNAP_H_LEN_Q1, REINA_SNAP_H_LEN_L1,
    REINA_SNAP_H_AGES_HASH = 12,            /* [2] FNV-1a 64 of reina_config_t.age_start (int32[REINA_MAX_AGES + 1]) */
    REINA_SNAP_H_DISEASE_HASH = 14,         /* [2] FNV-1a 64 of the reina_disease_t bytes */
    REINA_SNAP_H_BYTES = 16                 /* [2] bytes of the whole image */
};
#define REINA_SNAP_FLAG_TESTING_EVER 1u

int reina_snapshot_version(void);
/* count + scan of the engine's records; waits for the stream.  *bytes = size of the image reina_snap_pack would write */
int reina_snap_measure(reina_engine_t *e, uint64_t *bytes, void *stream);
/* writes the image to dev_out (device, >= the measured bytes, 16-byte aligned); the copies are queued on `stream` */
int reina_snap_pack(reina_engine_t *e, void *dev_out, uint64_t cap, void *stream);
/* restores an image (device) into an engine made for the same population, variants and disease, freshly initialised;
 * validates the header against the engine (REINA_E_INVALID + reina_last_error on a mismatch); waits for the stream once to
 * read the header */
int reina_snap_unpack(reina_engine_t *e, const void *dev_in, void *stream);
/* the same into every member of an engine group: one launch, each tile's records read once for all members */
int reina_group_snap_unpack(reina_group_t *g, const void *dev_in, void *stream);

#ifdef __cplusplus
}
#endif

#endif
