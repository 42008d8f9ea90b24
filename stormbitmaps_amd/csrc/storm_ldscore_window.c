/* storm_ldscore_window.c — the window planner of the stratified LD scores (storm_ldscore_window.h). Host only. */
#include "storm_ldscore_window.h"

#include <math.h>
#include <stddef.h>

int storm_ldscore_window_plan(const double* pos, uint64_t n, double max_dist, uint32_t* lo, uint32_t* hi, uint64_t* lag,
                              uint64_t* bad) {
    if (!(max_dist >= 0.0)) return STORM_LDSCORE_WINDOW_BAD_DIST;   /* (a NaN fails every comparison) */
    if (n > 0xFFFFFFFFull) return STORM_LDSCORE_WINDOW_TOO_MANY;
    /* every refusal before the first write */
    for (uint64_t i = 0; i < n; ++i) {
        if (!isfinite(pos[i])) {
            if (bad) *bad = i;
            return STORM_LDSCORE_WINDOW_NOT_FINITE;
        }
        if (i && pos[i] < pos[i - 1]) {
            if (bad) *bad = i;
            return STORM_LDSCORE_WINDOW_DECREASING;
        }
    }
    uint64_t first = 0, last = 0, need = 0;
    for (uint64_t i = 0; i < n; ++i) {
        /* pos does not decrease and a rounded difference is monotone in either operand: neither pointer ever steps back */
        while (pos[i] - pos[first] > max_dist) ++first;                     /* (first <= i: the difference at i is 0) */
        if (last < i) last = i;
        while (last + 1 < n && pos[last + 1] - pos[i] <= max_dist) ++last;
        if (lo && hi) lo[i] = (uint32_t)first, hi[i] = (uint32_t)last;
        if (i - first > need) need = i - first;
        if (last - i > need) need = last - i;
    }
    if (lag) *lag = need;
    return STORM_LDSCORE_WINDOW_OK;
}
