/* storm_dosage_prune.c — greedy LD pruning and clumping on the dosage container (storm.h: STORM_dosage_lag_prune, _complete
 * and their _device forms): the rows kept when the rows are walked in order of priority and a row is dropped as soon as a
 * kept row within its window exceeds min_r2 with it, resolved on the device from the band storm_dosage_lag.c's corr calls
 * write (storm_hip.h: storm_hip_lag_dosage_prune). The windows are resolved in storm_dosage_band.c, the order comes from the
 * host-only planner storm_prune_order.h; the container, its device copy and the locked paths are storm_dosage.c's; the order of the
 * checks is storm_dosage_ldscore_annot.c's. No CPU fallback. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"
#include "storm_dosage_internal.h"
#include "storm_prune_order.h"

/* the shim call on the container's device copy: 0 or -3 */
static int prune_run(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t lag, float min_r2,
                     const uint32_t* lo, const uint32_t* hi, const uint32_t* order, uint8_t* keep, uint32_t* owner, int complete,
                     int device) {
    static const char* const names[] = {"storm_hip_lag_dosage_prune", "storm_hip_lag_dosage_prune_complete"};
    int rc;
    if (complete)
        rc = device ? storm_hip_lag_dosage_prune_complete_device(ctx, m, n_samples, lag, min_r2, lo, hi, order, keep, owner)
                    : storm_hip_lag_dosage_prune_complete(ctx, m, n_samples, lag, min_r2, lo, hi, order, keep, owner);
    else
        rc = device ? storm_hip_lag_dosage_prune_device(ctx, m, n_samples, lag, min_r2, lo, hi, order, keep, owner)
                    : storm_hip_lag_dosage_prune(ctx, m, n_samples, lag, min_r2, lo, hi, order, keep, owner);
    return storm_dosage_band_result(ctx, rc, device, names[complete]);
}

static int dosage_prune(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist, const float* priority,
                        uint8_t* keep, uint32_t* owner, uint64_t out_len, int complete, int device, const char* who) {
    if (!h) return -1;
    if (!keep) return -2;
    int rc = storm_host_begin(who);
    const uint64_t n = h->n_rows;
    const int no_lag = max_lag == 0 && !pos;   /* (with positions, max_lag 0 asks for the lag the windows need) */
    if (!rc && !no_lag && out_len < n) rc = -4;
    if (!rc && no_lag) rc = storm_host_refuse(who, "max_lag must be at least 1 where no positions are given");
    if (!rc && isnan(min_r2)) rc = storm_host_refuse(who, "min_r2 is NaN");
    if (!rc && n > STORM_PRUNE_MAX_ROWS)
        rc = storm_host_refuse(who, "%llu rows: at most %d (the device keeps a bit per row in one workgroup's memory)",
                               (unsigned long long)n, STORM_PRUNE_MAX_ROWS);
    uint32_t* plan = NULL;   /* lo, then hi, then the order */
    uint64_t lag = max_lag;
    /* (one buffer of three words per row as soon as either the windows or the order want one) */
    if (!rc) rc = storm_dosage_band_windows(who, n, max_lag, pos, max_dist, pos || priority, &plan, &lag);
    if (!rc && priority && n) {
        uint64_t bad = 0;
        const int code = storm_prune_order_plan(priority, n, plan + 2 * n, NULL, &bad);
        if (code == STORM_PRUNE_ORDER_NAN) rc = storm_host_refuse(who, "priority[%llu] is NaN", (unsigned long long)bad);
        else if (code) rc = storm_host_refuse(who, "out of host memory for the order of %llu rows", (unsigned long long)n);
    }
    if (!rc && n == 1 && !device) {   /* a row without any edge is kept and owns itself: no device is asked */
        keep[0] = 1;
        if (owner) owner[0] = 0;
    } else if (!rc && n >= 1) {
        storm_hip_ctx_t* ctx = NULL;
        const storm_hip_matrix_t* m = NULL;
        rc = storm_dosage_operands(h, NULL, &ctx, &m, NULL);
        if (!rc)
            rc = prune_run(ctx, m, h->n_samples, lag, min_r2, pos ? plan : NULL, pos ? plan + n : NULL, priority ? plan + 2 * n : NULL,
                           keep, owner, complete, device);
    }
    free(plan);
    return storm_host_end(rc);
}

int STORM_dosage_lag_prune(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist,
                           const float* priority, uint8_t* keep, uint32_t* owner, uint64_t out_len) {
    return dosage_prune(h, min_r2, max_lag, pos, max_dist, priority, keep, owner, out_len, 0, 0, "STORM_dosage_lag_prune");
}
int STORM_dosage_lag_prune_device(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist,
                                  const float* priority, uint8_t* d_keep, uint32_t* d_owner, uint64_t out_len) {
    return dosage_prune(h, min_r2, max_lag, pos, max_dist, priority, d_keep, d_owner, out_len, 0, 1, "STORM_dosage_lag_prune_device");
}
int STORM_dosage_lag_prune_complete(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist,
                                    const float* priority, uint8_t* keep, uint32_t* owner, uint64_t out_len) {
    return dosage_prune(h, min_r2, max_lag, pos, max_dist, priority, keep, owner, out_len, 1, 0, "STORM_dosage_lag_prune_complete");
}
int STORM_dosage_lag_prune_complete_device(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist,
                                           const float* priority, uint8_t* d_keep, uint32_t* d_owner, uint64_t out_len) {
    return dosage_prune(h, min_r2, max_lag, pos, max_dist, priority, d_keep, d_owner, out_len, 1, 1,
                        "STORM_dosage_lag_prune_complete_device");
}
