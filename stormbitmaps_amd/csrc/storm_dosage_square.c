/* storm_dosage_square.c — r / r^2 and the numbers of shared samples between TWO dosage containers (storm.h:
 * STORM_dosage_square_corr, _square_nobs, _square_corr_complete and their _device forms). The container, its device copy
 * and the locked paths are storm_dosage.c's; argument checks and return codes are those of STORM_dosage_square_dot
 * (storm_dosage_complete.c). No CPU fallback. */
#include <stdint.h>
#include <stdio.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"
#include "storm_dosage_internal.h"

enum { SQUARE_CORR, SQUARE_NOBS, SQUARE_CORR_COMPLETE };

/* what: one of the three above; measure is read by the two correlations only */
static int square_stat(STORM_dosage_t* a, STORM_dosage_t* b, int what, int measure, void* out, uint64_t out_rows, uint64_t out_ld,
                       int device, const char* who) {
    if (!a || !b) return -1;
    if (!out) return -2;
    storm_host_lock();
    int rc = storm_host_one_slot_or_refuse(who);
    if (!rc && (out_rows < a->n_rows || out_ld < b->n_rows)) rc = -4;
    if (!rc && a->n_samples != b->n_samples) {
        char msg[200];
        snprintf(msg, sizeof(msg), "%s: containers of %llu and of %llu samples", who, (unsigned long long)a->n_samples,
                 (unsigned long long)b->n_samples);
        storm_host_error(msg);
        rc = -3;
    }
    if (!rc && what != SQUARE_NOBS && measure != STORM_DOSAGE_R2 && measure != STORM_DOSAGE_R) {
        char msg[200];
        snprintf(msg, sizeof(msg), "%s: measure %d must be 0 (STORM_DOSAGE_R2) or 1 (STORM_DOSAGE_R)", who, measure);
        storm_host_error(msg);
        rc = -3;
    }
    if (!rc && a->n_rows != 0 && b->n_rows != 0) {
        storm_hip_ctx_t *ctx = NULL, *ctx_b = NULL;
        const storm_hip_matrix_t* ma = storm_dosage_mirror(a, &ctx);
        const storm_hip_matrix_t* mb = ma ? (a == b ? ma : storm_dosage_mirror(b, &ctx_b)) : NULL;
        const uint64_t S = a->n_samples;
        const char* name = "storm_hip_square_dosage_corr";
        if (!ma || !mb) rc = -3;
        else {
            int hrc;
            if (what == SQUARE_NOBS) {
                name = "storm_hip_square_dosage_nobs";
                hrc = device ? storm_hip_square_dosage_nobs_device(ctx, ma, mb, S, (uint32_t*)out, out_ld)
                             : storm_hip_square_dosage_nobs(ctx, ma, mb, S, (uint32_t*)out, out_ld);
            } else if (what == SQUARE_CORR_COMPLETE) {
                name = "storm_hip_square_dosage_corr_complete";
                hrc = device ? storm_hip_square_dosage_corr_complete_device(ctx, ma, mb, measure, S, (float*)out, out_ld)
                             : storm_hip_square_dosage_corr_complete(ctx, ma, mb, measure, S, (float*)out, out_ld);
            } else {
                hrc = device ? storm_hip_square_dosage_corr_device(ctx, ma, mb, measure, S, (float*)out, out_ld)
                             : storm_hip_square_dosage_corr(ctx, ma, mb, measure, S, (float*)out, out_ld);
            }
            if (hrc != STORM_HIP_OK) {
                storm_host_device_error(name);
                rc = -3;
            }
        }
    }
    storm_host_unlock();
    return rc;
}

int STORM_dosage_square_corr(STORM_dosage_t* a, STORM_dosage_t* b, int measure, float* out, uint64_t out_rows, uint64_t out_ld) {
    return square_stat(a, b, SQUARE_CORR, measure, out, out_rows, out_ld, 0, "STORM_dosage_square_corr");
}
int STORM_dosage_square_corr_device(STORM_dosage_t* a, STORM_dosage_t* b, int measure, float* d_out, uint64_t out_rows,
                                    uint64_t out_ld) {
    return square_stat(a, b, SQUARE_CORR, measure, d_out, out_rows, out_ld, 1, "STORM_dosage_square_corr_device");
}
int STORM_dosage_square_nobs(STORM_dosage_t* a, STORM_dosage_t* b, uint32_t* out, uint64_t out_rows, uint64_t out_ld) {
    return square_stat(a, b, SQUARE_NOBS, 0, out, out_rows, out_ld, 0, "STORM_dosage_square_nobs");
}
int STORM_dosage_square_nobs_device(STORM_dosage_t* a, STORM_dosage_t* b, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld) {
    return square_stat(a, b, SQUARE_NOBS, 0, d_out, out_rows, out_ld, 1, "STORM_dosage_square_nobs_device");
}
int STORM_dosage_square_corr_complete(STORM_dosage_t* a, STORM_dosage_t* b, int measure, float* out, uint64_t out_rows,
                                      uint64_t out_ld) {
    return square_stat(a, b, SQUARE_CORR_COMPLETE, measure, out, out_rows, out_ld, 0, "STORM_dosage_square_corr_complete");
}
int STORM_dosage_square_corr_complete_device(STORM_dosage_t* a, STORM_dosage_t* b, int measure, float* d_out, uint64_t out_rows,
                                             uint64_t out_ld) {
    return square_stat(a, b, SQUARE_CORR_COMPLETE, measure, d_out, out_rows, out_ld, 1, "STORM_dosage_square_corr_complete_device");
}
