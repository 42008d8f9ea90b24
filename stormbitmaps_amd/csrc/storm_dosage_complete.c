/* storm_dosage_complete.c — the dosage container's rectangle (STORM_dosage_square_dot) and its calls for rows with missing
 * genotypes (storm.h: STORM_dosage_row_missing, _pairw_nobs, _pairw_corr_complete: the value 3 means "missing" there and
 * only there). The container, its device copy and the locked paths are storm_dosage.c's; argument checks and return codes
 * are those of STORM_dosage_pairw_corr. No CPU fallback. */
#include <stdint.h>
#include <stdio.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"
#include "storm_dosage_internal.h"

static int square_dot(STORM_dosage_t* a, STORM_dosage_t* b, uint32_t* out, uint64_t out_rows, uint64_t out_ld, int device,
                      const char* who) {
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
    if (!rc && a->n_rows != 0 && b->n_rows != 0) {
        storm_hip_ctx_t *ctx = NULL, *ctx_b = NULL;
        const storm_hip_matrix_t* ma = storm_dosage_mirror(a, &ctx);
        const storm_hip_matrix_t* mb = ma ? (a == b ? ma : storm_dosage_mirror(b, &ctx_b)) : NULL;
        if (!ma || !mb) rc = -3;
        else if ((device ? storm_hip_square_dosage_matrix_device(ctx, ma, mb, out, out_ld)
                         : storm_hip_square_dosage_matrix(ctx, ma, mb, out, out_ld)) != STORM_HIP_OK) {
            storm_host_device_error("storm_hip_square_dosage_matrix");
            rc = -3;
        }
    }
    storm_host_unlock();
    return rc;
}

int STORM_dosage_square_dot(STORM_dosage_t* a, STORM_dosage_t* b, uint32_t* out, uint64_t out_rows, uint64_t out_ld) {
    return square_dot(a, b, out, out_rows, out_ld, 0, "STORM_dosage_square_dot");
}
int STORM_dosage_square_dot_device(STORM_dosage_t* a, STORM_dosage_t* b, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld) {
    return square_dot(a, b, d_out, out_rows, out_ld, 1, "STORM_dosage_square_dot_device");
}

int STORM_dosage_row_missing(STORM_dosage_t* h, uint32_t* missing) {
    if (!h) return -1;
    if (!missing) return -2;
    storm_host_lock();
    int rc = storm_host_one_slot_or_refuse("STORM_dosage_row_missing");
    if (!rc && h->n_rows != 0) {
        storm_hip_ctx_t* ctx = NULL;
        const storm_hip_matrix_t* m = storm_dosage_mirror(h, &ctx);
        if (!m) rc = -3;
        else if (storm_hip_dosage_row_missing(ctx, m, h->n_samples, missing) != STORM_HIP_OK) {
            storm_host_device_error("storm_hip_dosage_row_missing");
            rc = -3;
        }
    }
    storm_host_unlock();
    return rc;
}

/* measure < 0: the numbers of shared samples N */
static int complete_pairw(STORM_dosage_t* h, int measure, void* out, uint64_t out_rows, uint64_t out_ld, int device, const char* who) {
    if (!h) return -1;
    if (!out) return -2;
    storm_host_lock();
    int rc = storm_host_one_slot_or_refuse(who);
    const uint64_t n = h->n_rows;
    if (!rc && (out_rows < n || out_ld < n)) rc = -4;
    if (!rc && measure >= 0 && measure != STORM_DOSAGE_R2 && measure != STORM_DOSAGE_R) {
        char msg[160];
        snprintf(msg, sizeof(msg), "%s: measure must be 0 (STORM_DOSAGE_R2) or 1 (STORM_DOSAGE_R)", who);
        storm_host_error(msg);
        rc = -3;
    }
    if (!rc && n >= 2) {
        storm_hip_ctx_t* ctx = NULL;
        const storm_hip_matrix_t* m = storm_dosage_mirror(h, &ctx);
        if (!m) rc = -3;
        else {
            int hrc;
            if (measure < 0)
                hrc = device ? storm_hip_pairw_dosage_nobs_device(ctx, m, h->n_samples, (uint32_t*)out, out_ld)
                             : storm_hip_pairw_dosage_nobs(ctx, m, h->n_samples, (uint32_t*)out, out_ld);
            else
                hrc = device ? storm_hip_pairw_dosage_corr_complete_device(ctx, m, measure, h->n_samples, (float*)out, out_ld)
                             : storm_hip_pairw_dosage_corr_complete(ctx, m, measure, h->n_samples, (float*)out, out_ld);
            if (hrc != STORM_HIP_OK) {
                storm_host_device_error(measure < 0 ? "storm_hip_pairw_dosage_nobs" : "storm_hip_pairw_dosage_corr_complete");
                rc = -3;
            }
        }
    }
    storm_host_unlock();
    return rc;
}

int STORM_dosage_pairw_nobs(STORM_dosage_t* h, uint32_t* out, uint64_t out_rows, uint64_t out_ld) {
    return complete_pairw(h, -1, out, out_rows, out_ld, 0, "STORM_dosage_pairw_nobs");
}
int STORM_dosage_pairw_nobs_device(STORM_dosage_t* h, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld) {
    return complete_pairw(h, -1, d_out, out_rows, out_ld, 1, "STORM_dosage_pairw_nobs_device");
}
int STORM_dosage_pairw_corr_complete(STORM_dosage_t* h, int measure, float* out, uint64_t out_rows, uint64_t out_ld) {
    return complete_pairw(h, measure < 0 ? STORM_DOSAGE_R + 1 : measure, out, out_rows, out_ld, 0, "STORM_dosage_pairw_corr_complete");
}
int STORM_dosage_pairw_corr_complete_device(STORM_dosage_t* h, int measure, float* d_out, uint64_t out_rows, uint64_t out_ld) {
    return complete_pairw(h, measure < 0 ? STORM_DOSAGE_R + 1 : measure, d_out, out_rows, out_ld, 1,
                          "STORM_dosage_pairw_corr_complete_device");
}
