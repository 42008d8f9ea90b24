/* storm_prune_order.h — the order planner of LD pruning and clumping (storm.h: STORM_dosage_lag_prune): from one priority
 * per row, the order in which the greedy walks the rows. Host only: no HIP, no container state, so a stand-alone program can
 * link storm_prune_order.c alone (tests/test_prune_order.py builds it with the host compiler). */
#ifndef STORM_PRUNE_ORDER_H
#define STORM_PRUNE_ORDER_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STORM_PRUNE_ORDER_OK 0
#define STORM_PRUNE_ORDER_NAN 1        /* priority[*bad] is NaN (*bad: the first such row) */
#define STORM_PRUNE_ORDER_TOO_MANY 2   /* n does not fit the uint32 entries */
#define STORM_PRUNE_ORDER_NOMEM 3      /* no host memory for the sort's second buffer (n uint32) */

/* order[k] = the row that is walked k-th, rank[order[k]] = k (rank may be NULL): higher priority first, ties to the lower
 * row index (-0.0f and +0.0f tie; +inf comes first, -inf last). priority == NULL: the identity, without sorting. A stable
 * bottom-up merge sort, O(n log n) comparisons, n uint32 of temporary memory.
 * Returns one of the codes above; on a refusal nothing of order and rank is written, and *bad (may be NULL) is the row the
 * refusal is about. */
int storm_prune_order_plan(const float* priority, uint64_t n, uint32_t* order, uint32_t* rank, uint64_t* bad);

#ifdef __cplusplus
}
#endif
#endif
