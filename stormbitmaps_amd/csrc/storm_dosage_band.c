/* storm_dosage_band.c — what the dosage container's calls on the band of r^2 share (storm_dosage_ldscore.c,
 * storm_dosage_ldscore_annot.c, storm_dosage_prune.c, and storm_dosage_lag.c for the last): the statistic's refusals, the
 * windows of the host-only planner (storm_ldscore_window.h) resolved into a lag and per-row bounds, and the report of a
 * shim call. storm.h's STORM_ldscore_window_lag is here too: it is the same planner without the bounds. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"
#include "storm_dosage_internal.h"
#include "storm_ldscore_window.h"

/* the window planner's refusal in words: -3, or 0 */
static int window_refusal(const char* who, int code, const double* pos, uint64_t bad) {
    char msg[240];
    switch (code) {
        case STORM_LDSCORE_WINDOW_OK: return 0;
        case STORM_LDSCORE_WINDOW_BAD_DIST: snprintf(msg, sizeof(msg), "%s: max_dist must be a number >= 0 (+inf: every row)", who); break;
        case STORM_LDSCORE_WINDOW_NOT_FINITE:
            snprintf(msg, sizeof(msg), "%s: pos[%llu] is not finite", who, (unsigned long long)bad);
            break;
        case STORM_LDSCORE_WINDOW_DECREASING:
            snprintf(msg, sizeof(msg), "%s: pos[%llu] = %.17g is less than pos[%llu] = %.17g: positions must not decrease", who,
                     (unsigned long long)bad, pos[bad], (unsigned long long)(bad - 1), pos[bad - 1]);
            break;
        default: snprintf(msg, sizeof(msg), "%s: more than 2^32 - 1 rows", who); break;
    }
    storm_host_error(msg);
    return -3;
}

int STORM_ldscore_window_lag(const double* pos, uint64_t n, double max_dist, uint64_t* lag) {
    if (!lag || (!pos && n)) return -2;
    uint64_t need = 0, bad = 0;
    const int code = storm_ldscore_window_plan(pos, n, max_dist, NULL, NULL, &need, &bad);
    if (code) {
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
    char msg[320];
    *plan = NULL;
    *lag = max_lag;
    if (n && (pos || extra_words_per_row)) {
        *plan = (uint32_t*)malloc((size_t)n * (2u + extra_words_per_row) * sizeof(uint32_t));
        if (!*plan) {
            snprintf(msg, sizeof(msg), "%s: out of host memory for the windows%s of %llu rows", who,
                     extra_words_per_row ? " and the order" : "", (unsigned long long)n);
            storm_host_error(msg);
            return -3;
        }
    }
    if (!pos) return 0;
    uint64_t need = 0, bad = 0;
    const int code = storm_ldscore_window_plan(pos, n, max_dist, *plan, *plan ? *plan + n : NULL, &need, &bad);
    if (window_refusal(who, code, pos, bad)) return -3;
    if (max_lag != 0 && need > max_lag) {
        snprintf(msg, sizeof(msg), "%s: the windows need a lag of %llu rows, max_lag is %llu (0 takes what the windows need)", who,
                 (unsigned long long)need, (unsigned long long)max_lag);
        storm_host_error(msg);
        return -3;
    }
    if (max_lag == 0) *lag = need ? need : 1u;   /* (no row has a neighbour: the windows still say so) */
    return 0;
}

int storm_dosage_ldscore_stat_refusal(const char* who, int stat, int complete, uint64_t n_samples) {
    char msg[200];
    if (stat != STORM_LDSCORE_R2 && stat != STORM_LDSCORE_R2_ADJ)
        snprintf(msg, sizeof(msg), "%s: stat must be 0 (STORM_LDSCORE_R2) or 1 (STORM_LDSCORE_R2_ADJ)", who);
    else if (!complete && stat == STORM_LDSCORE_R2_ADJ && n_samples < 3)
        snprintf(msg, sizeof(msg), "%s: STORM_LDSCORE_R2_ADJ divides by n_samples - 2: at least 3 samples", who);
    else
        return 0;
    storm_host_error(msg);
    return -3;
}

int storm_dosage_shim_result(storm_hip_ctx_t* ctx, int rc, int device, const char* name) {
    if (rc == STORM_HIP_OK && device) rc = storm_hip_ctx_synchronize(ctx);
    if (rc != STORM_HIP_OK) {
        storm_host_device_error(name);
        return -3;
    }
    return 0;
}
