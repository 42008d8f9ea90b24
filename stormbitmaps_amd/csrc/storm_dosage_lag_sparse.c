/* storm_dosage_lag_sparse.c — the sparse LD report on the dosage container (storm.h: STORM_dosage_lag_corr_sparse, _complete
 * and their _device forms): the pairs within the lag and the rows' windows whose r^2 exceeds min_r2, as a CSR list compacted
 * on the device from the band storm_dosage_lag.c's corr calls write (storm_hip.h: storm_hip_lag_dosage_corr_sparse) — the
 * edge set storm_dosage_prune.c's calls walk. The windows are resolved in storm_dosage_band.c; the container, its device copy
 * and the locked paths are storm_dosage.c's; the order of the checks is storm_dosage_prune.c's. No CPU fallback. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"
#include "storm_dosage_internal.h"

/* the shim call on the container's device copy: 0, -3, or -4 where a host form's capacity is below the total (*n_pairs) */
static int sparse_run(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t lag, float min_r2,
                      const uint32_t* lo, const uint32_t* hi, uint64_t* row_start, uint32_t* col, float* val, uint64_t capacity,
                      uint64_t* n_pairs, int complete, int device, const char* who) {
    static const char* const names[] = {"storm_hip_lag_dosage_corr_sparse", "storm_hip_lag_dosage_corr_sparse_complete"};
    int rc;
    if (complete)
        rc = device ? storm_hip_lag_dosage_corr_sparse_complete_device(ctx, m, n_samples, lag, min_r2, lo, hi, row_start, col, val,
                                                                       capacity)
                    : storm_hip_lag_dosage_corr_sparse_complete(ctx, m, n_samples, lag, min_r2, lo, hi, row_start, col, val, capacity,
                                                                n_pairs);
    else
        rc = device ? storm_hip_lag_dosage_corr_sparse_device(ctx, m, n_samples, lag, min_r2, lo, hi, row_start, col, val, capacity)
                    : storm_hip_lag_dosage_corr_sparse(ctx, m, n_samples, lag, min_r2, lo, hi, row_start, col, val, capacity, n_pairs);
    if (!device && rc == STORM_HIP_EINVAL && col && *n_pairs > capacity) {   /* the list is longer than its buffers */
        (void)storm_host_refuse(who, "%llu pairs are listed, capacity is %llu", (unsigned long long)*n_pairs,
                                (unsigned long long)capacity);
        return -4;
    }
    /* (a _device form is waited for where it was given windows: lo / hi are freed on return) */
    return storm_dosage_band_result(ctx, rc, device && lo, names[complete]);
}

static int dosage_lag_sparse(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist,
                             uint64_t* row_start, uint64_t out_rows, uint32_t* col, float* val, uint64_t capacity, uint64_t* n_pairs,
                             int complete, int device, const char* who) {
    if (!h) return -1;
    if (!row_start || (!device && !n_pairs)) return -2;
    if (!col != !val || (!col && capacity != 0)) return -2;
    int rc = storm_host_begin(who);
    const uint64_t n = h->n_rows;
    const int no_lag = max_lag == 0 && !pos;   /* (with positions, max_lag 0 asks for the lag the windows need) */
    if (!rc && !no_lag && out_rows < n + 1 && !(n == 0 && out_rows == 0)) rc = -4;
    if (!rc && no_lag) rc = storm_host_refuse(who, "max_lag must be at least 1 where no positions are given");
    if (!rc && isnan(min_r2)) rc = storm_host_refuse(who, "min_r2 is NaN");
    uint32_t* plan = NULL;   /* lo, then hi */
    uint64_t lag = max_lag;
    if (!rc) rc = storm_dosage_band_windows(who, n, max_lag, pos, max_dist, 0, &plan, &lag);
    if (!rc && n < 2 && !device) {   /* no pair: the offsets alone, and no device is asked */
        for (uint64_t i = 0; i <= n && i < out_rows; ++i) row_start[i] = 0;
        *n_pairs = 0;
    } else if (!rc && out_rows) {
        storm_hip_ctx_t* ctx = NULL;
        const storm_hip_matrix_t* m = NULL;
        if (n_pairs) *n_pairs = 0;
        rc = storm_dosage_operands(h, NULL, &ctx, &m, NULL);
        if (!rc)
            rc = sparse_run(ctx, m, h->n_samples, lag, min_r2, pos ? plan : NULL, pos ? plan + n : NULL, row_start, col, val, capacity,
                            n_pairs, complete, device, who);
    }
    free(plan);
    return storm_host_end(rc);
}

int STORM_dosage_lag_corr_sparse(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist,
                                 uint64_t* row_start, uint64_t out_rows, uint32_t* col, float* val, uint64_t capacity,
                                 uint64_t* n_pairs) {
    return dosage_lag_sparse(h, min_r2, max_lag, pos, max_dist, row_start, out_rows, col, val, capacity, n_pairs, 0, 0,
                             "STORM_dosage_lag_corr_sparse");
}
int STORM_dosage_lag_corr_sparse_device(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist,
                                        uint64_t* d_row_start, uint64_t out_rows, uint32_t* d_col, float* d_val, uint64_t capacity) {
    return dosage_lag_sparse(h, min_r2, max_lag, pos, max_dist, d_row_start, out_rows, d_col, d_val, capacity, NULL, 0, 1,
                             "STORM_dosage_lag_corr_sparse_device");
}
int STORM_dosage_lag_corr_sparse_complete(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist,
                                          uint64_t* row_start, uint64_t out_rows, uint32_t* col, float* val, uint64_t capacity,
                                          uint64_t* n_pairs) {
    return dosage_lag_sparse(h, min_r2, max_lag, pos, max_dist, row_start, out_rows, col, val, capacity, n_pairs, 1, 0,
                             "STORM_dosage_lag_corr_sparse_complete");
}
int STORM_dosage_lag_corr_sparse_complete_device(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos,
                                                 double max_dist, uint64_t* d_row_start, uint64_t out_rows, uint32_t* d_col,
                                                 float* d_val, uint64_t capacity) {
    return dosage_lag_sparse(h, min_r2, max_lag, pos, max_dist, d_row_start, out_rows, d_col, d_val, capacity, NULL, 1, 1,
                             "STORM_dosage_lag_corr_sparse_complete_device");
}
