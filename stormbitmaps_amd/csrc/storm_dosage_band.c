/* storm_dosage_band.c — what the dosage container's calls on the band of r^2 share (storm_dosage_ldscore.c,
 * storm_dosage_ldscore_annot.c, storm_dosage_prune.c): the statistic's refusals, the windows of the host-only planner
 * (storm_ldscore_window.h) resolved into a lag and per-row bounds, and the report of a band call. storm.h's
 * STORM_ldscore_window_lag is here too: it is the same planner without the bounds. */
#include <stdint.h>
#include <stdlib.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"
#include "storm_dosage_internal.h"
#include "storm_ldscore_window.h"

/* the window planner's refusal in words: -3, or 0 */
static int window_refusal(const char* who, int code, const double* pos, uint64_t bad) {
    switch (code) {
        case STORM_LDSCORE_WINDOW_OK: return 0;
        case STORM_LDSCORE_WINDOW_BAD_DIST: return storm_host_refuse(who, "max_dist must be a number >= 0 (+inf: every row)");
        case STORM_LDSCORE_WINDOW_NOT_FINITE: return storm_host_refuse(who, "pos[%llu] is not finite", (unsigned long long)bad);
        case STORM_LDSCORE_WINDOW_DECREASING:
            return storm_host_refuse(who, "pos[%llu] = %.17g is less than pos[%llu] = %.17g: positions must not decrease",
                                     (unsigned long long)bad, pos[bad], (unsigned long long)(bad - 1), pos[bad - 1]);
        default: return storm_host_refuse(who, "more than 2^32 - 1 rows");
    }
}

int STORM_ldscore_window_lag(const double* pos, uint64_t n, double max_dist, uint64_t* lag) {
    if (!lag || (!pos && n)) return -2;
    uint64_t need = 0, bad = 0;
    const int code = storm_ldscore_window_plan(pos, n, max_dist, NULL, NULL, &need, &bad);
    if (code) {   /* (no device is involved: the lock only orders the report with the other calls', as it always did) */
        storm_host_lock();
        const int rc = window_refusal("STORM_ldscore_window_lag", code, pos, bad);
        storm_host_unlock();
        return rc;
    }
    *lag = need;
    return 0;
}

int storm_dosage_band_windows(const char* who, uint64_t n, uint64_t max_lag, const double* pos, double max_dist,
                              unsigned extra_words_per_row, uint32_t** plan, uint64_t* lag) {
    *plan = NULL;
    *lag = max_lag;
    if (n && (pos || extra_words_per_row)) {
        *plan = (uint32_t*)malloc((size_t)n * (2u + extra_words_per_row) * sizeof(uint32_t));
        if (!*plan)
            return storm_host_refuse(who, "out of host memory for the windows%s of %llu rows",
                                     extra_words_per_row ? " and the order" : "", (unsigned long long)n);
    }
    if (!pos) return 0;
    uint64_t need = 0, bad = 0;
    const int code = storm_ldscore_window_plan(pos, n, max_dist, *plan, *plan ? *plan + n : NULL, &need, &bad);
    if (window_refusal(who, code, pos, bad)) return -3;
    if (max_lag != 0 && need > max_lag)
        return storm_host_refuse(who, "the windows need a lag of %llu rows, max_lag is %llu (0 takes what the windows need)",
                                 (unsigned long long)need, (unsigned long long)max_lag);
    if (max_lag == 0) *lag = need ? need : 1u;   /* (no row has a neighbour: the windows still say so) */
    return 0;
}

int storm_dosage_ldscore_stat_refusal(const char* who, int stat, int complete, uint64_t n_samples) {
    if (stat != STORM_LDSCORE_R2 && stat != STORM_LDSCORE_R2_ADJ)
        return storm_host_refuse(who, "stat must be 0 (STORM_LDSCORE_R2) or 1 (STORM_LDSCORE_R2_ADJ)");
    if (!complete && stat == STORM_LDSCORE_R2_ADJ && n_samples < 3)
        return storm_host_refuse(who, "STORM_LDSCORE_R2_ADJ divides by n_samples - 2: at least 3 samples");
    return 0;
}

int storm_dosage_band_result(storm_hip_ctx_t* ctx, int rc, int device, const char* name) {
    /* The one place that asks for the wait. A _device form of the LD scores, the stratified scores and pruning returns with
     * its work queued while lo / hi / order, host arrays its caller here frees on return, are still being read, and a caller
     * of storm.h has no handle on that stream: it is waited for. Every other _device form leaves no host array of the
     * library's behind it, passes wait 0 and returns with its work queued — as does the sparse list's _device form where it
     * was given no positions (storm_dosage_lag_sparse.c passes `device` only with windows). */
    return storm_host_shim_result(ctx, rc, device, name);
}
