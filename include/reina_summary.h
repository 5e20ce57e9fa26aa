/* Ensemble summaries: quantile bands, sums, peaks and exceedance of the members' counter histories, computed where the rows
 * are (companion of reina_hip.h; same library, same error codes; reina_model_amd/summary.py:
 * summarise_numpy is the executable specification).
 *
 * INPUT  K members, 1 <= K <= REINA_SUMMARY_MAX_MEMBERS; of each member `days` history rows (1 <= days <= REINA_MAX_DAYS) of
 * REINA_COUNTER_WORDS int32, as reina_run_days_hist and reina_group_run_days write them; nr_ages in 1..REINA_MAX_AGES; the
 * table age -> group of the other reports, n_groups = G <= REINA_SUMMARY_MAX_GROUPS, every group < G.  The summary takes no
 * engine: it reads history rows and writes its own block.
 *
 * SERIES  every row is reduced to S = REINA_SUMMARY_SERIES(G) = REINA_C_NR * (1 + G) + REINA_S_NR values, int32:
 *   series c * (1 + G)                counter c summed over the ages [0, nr_ages)
 *   series c * (1 + G) + 1 + g        the same sum over the ages whose group is g
 *   series REINA_C_NR * (1 + G) + s   scalar slot s, copied
 * Words of ages >= nr_ages are ignored.  The sums are taken as uint32 and reinterpreted: they wrap (numpy's
 * .sum(dtype=int32)).  No counter of a real run comes near the wrap.  A quantile of a total is not a sum of quantiles, which
 * is why the sums come first.
 *
 * REPORT BLOCK  REINA_SUMMARY_REPORT_WORDS(K, days, S, Q, T) int64 words, tables row-major at the offsets below:
 *   order[days][S][Q]     for Q <= REINA_SUMMARY_MAX_RANKS caller-given ranks 0 <= r_q <= K - 1 (any order, repeats allowed):
 *                         the r_q-th smallest of the K members' values of that series on that day
 *   sum[days][S]          the sum over the members, in 64 bits
 *   peak[K][S][2]         of each member: the largest value over the days, and the first day on which it is reached
 *   final[K][S]           of each member: the value on the last day
 *   exceed[T][days]       for T <= REINA_SUMMARY_MAX_THRESHOLDS thresholds (series, value): the members whose series is
 *                         > value on that day
 *   first_exceed[T][K]    of each member: the first such day, or -1
 * Ranks come from quantile levels on the host by rank(q, K) = max(ceil(q * K) - 1, 0): the inverted CDF.
 *
 * REFUSED (REINA_E_INVALID + reina_last_error, nothing queued): K, days, nr_ages, n_groups, n_ranks or n_thresholds out of
 * range; an age's group not below n_groups; a rank >= K; a threshold's series >= S; a null pointer; a member's rows, the
 * scratch or the report not 16-byte aligned. */
#ifndef REINA_SUMMARY_H
#define REINA_SUMMARY_H

#include <stddef.h>
#include <stdint.h>

#include "reina_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define REINA_SUMMARY_VERSION 1
#define REINA_SUMMARY_MAX_MEMBERS 1024
#define REINA_SUMMARY_MAX_GROUPS 16
#define REINA_SUMMARY_MAX_RANKS 16
#define REINA_SUMMARY_MAX_THRESHOLDS 32
#define REINA_SUMMARY_PEAK_FIELDS 2     /* value, first day */

typedef struct {
    uint32_t series;   /* < S */
    int32_t value;     /* a member exceeds when its series is > value */
} reina_summary_threshold_t;

/* series of a row with G age groups */
#define REINA_SUMMARY_SERIES(G) (REINA_C_NR * (1u + (G)) + REINA_S_NR)

/* word offsets of the report block (int64 words) */
#define REINA_SUMMARY_ORDER(K, days, S, Q, T) ((size_t)0u)
#define REINA_SUMMARY_SUM(K, days, S, Q, T) (REINA_SUMMARY_ORDER(K, days, S, Q, T) + (size_t)(days) * (S) * (Q))
#define REINA_SUMMARY_PEAK(K, days, S, Q, T) (REINA_SUMMARY_SUM(K, days, S, Q, T) + (size_t)(days) * (S))
#define REINA_SUMMARY_FINAL(K, days, S, Q, T) (REINA_SUMMARY_PEAK(K, days, S, Q, T) + (size_t)(K) * (S) * REINA_SUMMARY_PEAK_FIELDS)
#define REINA_SUMMARY_EXCEED(K, days, S, Q, T) (REINA_SUMMARY_FINAL(K, days, S, Q, T) + (size_t)(K) * (S))
#define REINA_SUMMARY_FIRST_EXCEED(K, days, S, Q, T) (REINA_SUMMARY_EXCEED(K, days, S, Q, T) + (size_t)(T) * (days))
#define REINA_SUMMARY_REPORT_WORDS(K, days, S, Q, T) (REINA_SUMMARY_FIRST_EXCEED(K, days, S, Q, T) + (size_t)(T) * (K))

/* Caller-owned device scratch of one summary, 16-byte aligned: a head (the ranks, the thresholds, the group table and the K
 * member pointers, copied there on the stream) and the series, int32 [days][K][S].  Everything in it is written before it is
 * read: it needs no initialisation and may be reused. */
#define REINA_SUMMARY_HEAD_BYTES(K) ((512u + (size_t)(K) * 8u + 255u) & ~(size_t)255u)
#define REINA_SUMMARY_SCRATCH_BYTES(K, days, S) (REINA_SUMMARY_HEAD_BYTES(K) + (((size_t)(days) * (K) * (S) * 4u + 255u) & ~(size_t)255u))

int reina_summary_version(void);
/* The summary of K members' histories into dev_report (device, 16-byte aligned, REINA_SUMMARY_REPORT_WORDS int64 words, every
 * one of them overwritten), queued on `stream`; the call does not wait for it.  history_bases: HOST array of K device pointers,
 * member m's rows [days][REINA_COUNTER_WORDS], each 16-byte aligned; the members need not be contiguous or in any order.
 * age_group: host table of the group of every age below nr_ages.  ranks: host array [n_ranks]; thresholds: host array
 * [n_thresholds] (either may be NULL when its count is 0).  The host arrays are read before the call returns.  Reads the
 * rows, writes nothing but dev_scratch (REINA_SUMMARY_SCRATCH_BYTES) and dev_report. */
int reina_summary(const int32_t *const *history_bases, uint32_t K, uint32_t days, uint32_t nr_ages,
                  const uint8_t *age_group, uint32_t n_groups, const uint32_t *ranks, uint32_t n_ranks,
                  const reina_summary_threshold_t *thresholds, uint32_t n_thresholds,
                  void *dev_scratch, int64_t *dev_report, void *stream);

#ifdef __cplusplus
}
#endif

#endif
