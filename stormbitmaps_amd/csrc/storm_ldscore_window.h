/* storm_ldscore_window.h — the window planner of the stratified LD scores (storm.h: STORM_dosage_lag_ldscore_annot,
 * STORM_ldscore_window_lag): from the rows' coordinates and a maximum distance, the first and the last row every row is
 * summed against. Host only: no HIP, no container state, so a stand-alone program can link storm_ldscore_window.c alone
 * (tests/test_ldscore_window.py builds it with the host compiler). */
#ifndef STORM_LDSCORE_WINDOW_H
#define STORM_LDSCORE_WINDOW_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STORM_LDSCORE_WINDOW_OK 0
#define STORM_LDSCORE_WINDOW_BAD_DIST 1     /* max_dist is negative or NaN */
#define STORM_LDSCORE_WINDOW_NOT_FINITE 2   /* pos[*bad] is NaN or infinite */
#define STORM_LDSCORE_WINDOW_DECREASING 3   /* pos[*bad] < pos[*bad - 1] */
#define STORM_LDSCORE_WINDOW_TOO_MANY 4     /* n does not fit the uint32 bounds */

/* Row i is summed against the rows j of [lo[i], hi[i]], j != i: those with |pos[j] - pos[i]| <= max_dist. pos is not
 * decreasing (equal positions are allowed: ties are inside every window that holds one of them); max_dist = +inf gives
 * [0, n - 1] for every row. Two pointers, O(n). *lag (may be NULL) = max_i max(i - lo[i], hi[i] - i), 0 for n < 2; lo and
 * hi may both be NULL (the lag alone). The distance of a pair is computed once, as pos[later] - pos[earlier], on either
 * side: j is in row i's window exactly when i is in row j's.
 * Returns one of the codes above; on a refusal nothing of lo, hi and *lag is written, and *bad (may be NULL) is the index
 * the refusal is about. */
int storm_ldscore_window_plan(const double* pos, uint64_t n, double max_dist, uint32_t* lo, uint32_t* hi, uint64_t* lag,
                              uint64_t* bad);

#ifdef __cplusplus
}
#endif
#endif
