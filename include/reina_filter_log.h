/* Particle filters over LOGGED engine groups: the in-group clone that carries the dated transmission log and the clinical
 * course log (companion of reina_filter.h, reina_txlog.h and reina_course.h; same library, same error codes; DESIGN.md section
 * 6d "Logged filters"; reina_model_amd/filtering.py: clone_log_numpy / clone_course_numpy are the executable specification,
 * clone_log_delta_numpy the kernel's rule).
 *
 * A clone (reina_group_clone) overwrites member dst's carried state with member src's.  The logs live outside the engine
 * state, so a logged group is cloned through its log: for every (dst, src) pair
 *     the log word of every agent of dst equals that of src,
 *     the course record of every agent of dst equals that of src, when a course is attached to the log,
 *     dst's carried state is what reina_group_clone makes it.
 * Members in no pair, and every source, are untouched.  After the call a particle's log is the log of its whole ancestral
 * path, and the next recorded day follows the last one: the day byte of dst's hot words and dst's log words both come from src.
 *
 * The copy is a delta on an INVARIANT of the logs:
 *     hot == 0  =>  the log word is NONE | NONE << 16 and the course record is four NONE
 * (the begin passes and the record launches write only where RH_STATE(hot) != 0, and a hot word never returns to 0).  Where
 * either member's hot word is non-zero the word (and record) is copied from src to dst; agents susceptible in both members
 * are not touched.  reina_txlog_write and reina_course_write leave the invariant to the caller: words written for an agent
 * whose hot word is 0 must be all NONE, or a later clone will not carry them.
 *
 * Per chunk of at most REINA_CLONE_MAX_PAIRS pairs the log's launch is queued AHEAD of the state's on the same stream: it
 * reads dst's hot words, which the state's launch overwrites.
 *
 * REFUSED (REINA_E_INVALID + reina_last_error, state and logs untouched): a NULL log, a single engine's log, a course whose
 * log is gone, and everything reina_group_clone refuses (an index out of range, a duplicate dst, a src that is also a dst,
 * members whose testing_ever flags differ).  n_pairs == 0 succeeds and does nothing. */
#ifndef REINA_FILTER_LOG_H
#define REINA_FILTER_LOG_H

#include <stdint.h>

#include "reina_course.h"
#include "reina_filter.h"
#include "reina_txlog.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REINA_FILTER_LOG_VERSION 1

int reina_filter_log_version(void);
/* reina_group_clone for a logged group: for every (dst, src) pair member dst also gets member src's log words and, when a
 * course is attached to the log, its course records.  `log` must be a group's log (reina_group_txlog_create).  Two launches
 * per REINA_CLONE_MAX_PAIRS pairs, queued on `stream`; no allocation, no host wait. */
int reina_group_txlog_clone(reina_txlog_t *log, const uint32_t *pairs, uint32_t n_pairs, void *stream);

#ifdef __cplusplus
}
#endif

#endif
