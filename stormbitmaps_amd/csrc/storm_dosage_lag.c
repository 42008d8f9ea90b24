/* storm_dosage_lag.c — the dosage container's pairwise calls for the pairs within max_lag rows of each other (storm.h:
 * STORM_dosage_pairw_lag_dot, _lag_corr, _lag_nobs, _lag_corr_complete and their _device forms): row i against the next L
 * rows, an n x L matrix in the lag layout (storm_hip.h: storm_hip_pairw_lag_dosage_matrix_device). The container, its
 * device copy and the locked paths are storm_dosage.c's; the order of the checks is storm_lag.c's. No CPU fallback. */
#include <stdint.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"
#include "storm_dosage_internal.h"

enum { LAG_DOT, LAG_CORR, LAG_NOBS, LAG_CORR_COMPLETE };

/* the shim call of `what` on the container's device copy: 0 or -3 */
static int lag_run(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int what, int measure, uint64_t n_samples, uint64_t max_lag,
                   void* out, uint64_t out_ld, int device) {
    static const char* const names[] = {"storm_hip_pairw_lag_dosage_matrix", "storm_hip_pairw_lag_dosage_corr",
                                        "storm_hip_pairw_lag_dosage_nobs", "storm_hip_pairw_lag_dosage_corr_complete"};
    int rc;
    switch (what) {
        case LAG_DOT:
            rc = device ? storm_hip_pairw_lag_dosage_matrix_device(ctx, m, max_lag, 0, ~0ull, (uint32_t*)out, out_ld)
                        : storm_hip_pairw_lag_dosage_matrix(ctx, m, max_lag, (uint32_t*)out, out_ld);
            break;
        case LAG_CORR:
            rc = device ? storm_hip_pairw_lag_dosage_corr_device(ctx, m, measure, n_samples, max_lag, (float*)out, out_ld)
                        : storm_hip_pairw_lag_dosage_corr(ctx, m, measure, n_samples, max_lag, (float*)out, out_ld);
            break;
        case LAG_NOBS:
            rc = device ? storm_hip_pairw_lag_dosage_nobs_device(ctx, m, n_samples, max_lag, (uint32_t*)out, out_ld)
                        : storm_hip_pairw_lag_dosage_nobs(ctx, m, n_samples, max_lag, (uint32_t*)out, out_ld);
            break;
        default:
            rc = device ? storm_hip_pairw_lag_dosage_corr_complete_device(ctx, m, measure, n_samples, max_lag, (float*)out, out_ld)
                        : storm_hip_pairw_lag_dosage_corr_complete(ctx, m, measure, n_samples, max_lag, (float*)out, out_ld);
    }
    /* (these calls read no host array after they return, so a _device form is not waited for) */
    return storm_host_shim_result(ctx, rc, 0, names[what]);
}

static int dosage_lag(STORM_dosage_t* h, int what, int measure, uint64_t max_lag, void* out, uint64_t out_rows, uint64_t out_ld,
                      int device, const char* who) {
    if (!h) return -1;
    if (!out) return -2;
    int rc = storm_host_begin(who);
    const uint64_t n = h->n_rows;
    const uint64_t lag = n ? (max_lag < n - 1 ? max_lag : n - 1) : 0;
    if (!rc && max_lag != 0 && (out_rows < n || out_ld < lag)) rc = -4;
    if (!rc && max_lag == 0) rc = storm_host_refuse(who, "max_lag must be at least 1");
    if (!rc && (what == LAG_CORR || what == LAG_CORR_COMPLETE)) rc = storm_dosage_measure_refusal(who, measure);
    if (!rc && n >= 2) {
        storm_hip_ctx_t* ctx = NULL;
        const storm_hip_matrix_t* m = NULL;
        rc = storm_dosage_operands(h, NULL, &ctx, &m, NULL);
        if (!rc) rc = lag_run(ctx, m, what, measure, h->n_samples, max_lag, out, out_ld, device);
    }
    return storm_host_end(rc);
}

int STORM_dosage_pairw_lag_dot(STORM_dosage_t* h, uint64_t max_lag, uint32_t* out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_lag(h, LAG_DOT, 0, max_lag, out, out_rows, out_ld, 0, "STORM_dosage_pairw_lag_dot");
}
int STORM_dosage_pairw_lag_dot_device(STORM_dosage_t* h, uint64_t max_lag, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_lag(h, LAG_DOT, 0, max_lag, d_out, out_rows, out_ld, 1, "STORM_dosage_pairw_lag_dot_device");
}
int STORM_dosage_pairw_lag_corr(STORM_dosage_t* h, int measure, uint64_t max_lag, float* out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_lag(h, LAG_CORR, measure, max_lag, out, out_rows, out_ld, 0, "STORM_dosage_pairw_lag_corr");
}
int STORM_dosage_pairw_lag_corr_device(STORM_dosage_t* h, int measure, uint64_t max_lag, float* d_out, uint64_t out_rows,
                                       uint64_t out_ld) {
    return dosage_lag(h, LAG_CORR, measure, max_lag, d_out, out_rows, out_ld, 1, "STORM_dosage_pairw_lag_corr_device");
}
int STORM_dosage_pairw_lag_nobs(STORM_dosage_t* h, uint64_t max_lag, uint32_t* out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_lag(h, LAG_NOBS, 0, max_lag, out, out_rows, out_ld, 0, "STORM_dosage_pairw_lag_nobs");
}
int STORM_dosage_pairw_lag_nobs_device(STORM_dosage_t* h, uint64_t max_lag, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_lag(h, LAG_NOBS, 0, max_lag, d_out, out_rows, out_ld, 1, "STORM_dosage_pairw_lag_nobs_device");
}
int STORM_dosage_pairw_lag_corr_complete(STORM_dosage_t* h, int measure, uint64_t max_lag, float* out, uint64_t out_rows,
                                         uint64_t out_ld) {
    return dosage_lag(h, LAG_CORR_COMPLETE, measure, max_lag, out, out_rows, out_ld, 0, "STORM_dosage_pairw_lag_corr_complete");
}
int STORM_dosage_pairw_lag_corr_complete_device(STORM_dosage_t* h, int measure, uint64_t max_lag, float* d_out, uint64_t out_rows,
                                                uint64_t out_ld) {
    return dosage_lag(h, LAG_CORR_COMPLETE, measure, max_lag, d_out, out_rows, out_ld, 1,
                      "STORM_dosage_pairw_lag_corr_complete_device");
}
