/* storm_dosage_pairs.c — the per-pair matrices of the dosage container (storm.h: STORM_dosage_pairw_dot, _corr, _nobs,
 * _corr_complete, the same four as STORM_dosage_square_* between TWO containers, and their _device forms): one body over the
 * statistic, the triangle of one container or the rectangle of two, and the host or device form. In the _nobs and _complete
 * calls the value 3 means "missing". The container, its device copy and the shared checks are storm_dosage.c's; the frame is
 * storm_host_call.c's. No CPU fallback. */
#include <stdint.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"
#include "storm_dosage_internal.h"

enum { DOT, CORR, NOBS, CORR_COMPLETE };

#define FORM(call, ...) (device ? call##_device(__VA_ARGS__) : call(__VA_ARGS__))

/* the shim call of `stat` on the device copies (`square`: ma's rows against mb's): 0 or -3 */
static int pairs_run(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* ma, const storm_hip_matrix_t* mb, int square, int stat,
                     int measure, uint64_t S, void* out, uint64_t ld, int device) {
    static const char* const names[2][4] = {
        {"storm_hip_pairw_dosage_matrix", "storm_hip_pairw_dosage_corr", "storm_hip_pairw_dosage_nobs",
         "storm_hip_pairw_dosage_corr_complete"},
        {"storm_hip_square_dosage_matrix", "storm_hip_square_dosage_corr", "storm_hip_square_dosage_nobs",
         "storm_hip_square_dosage_corr_complete"}};
    int rc;
    switch (stat) {
        case DOT:
            rc = square ? FORM(storm_hip_square_dosage_matrix, ctx, ma, mb, (uint32_t*)out, ld)
                        : FORM(storm_hip_pairw_dosage_matrix, ctx, ma, (uint32_t*)out, ld);
            break;
        case CORR:
            rc = square ? FORM(storm_hip_square_dosage_corr, ctx, ma, mb, measure, S, (float*)out, ld)
                        : FORM(storm_hip_pairw_dosage_corr, ctx, ma, measure, S, (float*)out, ld);
            break;
        case NOBS:
            rc = square ? FORM(storm_hip_square_dosage_nobs, ctx, ma, mb, S, (uint32_t*)out, ld)
                        : FORM(storm_hip_pairw_dosage_nobs, ctx, ma, S, (uint32_t*)out, ld);
            break;
        default:
            rc = square ? FORM(storm_hip_square_dosage_corr_complete, ctx, ma, mb, measure, S, (float*)out, ld)
                        : FORM(storm_hip_pairw_dosage_corr_complete, ctx, ma, measure, S, (float*)out, ld);
    }
    return storm_host_shim_result(ctx, rc, 0, names[square][stat]);
}

/* square: a's rows against b's, else the rows of `a` among themselves (b unused). measure is read by the two correlations only */
static int dosage_pairs(STORM_dosage_t* a, STORM_dosage_t* b, int square, int stat, int measure, void* out, uint64_t out_rows,
                        uint64_t out_ld, int device, const char* who) {
    if (!a || (square && !b)) return -1;
    if (!out) return -2;
    int rc = storm_host_begin(who);
    const uint64_t n_a = a->n_rows, n_b = square ? b->n_rows : n_a;
    if (!rc && (out_rows < n_a || out_ld < n_b)) rc = -4;
    if (!rc && square) rc = storm_dosage_samples_refusal(who, a, b);
    if (!rc && (stat == CORR || stat == CORR_COMPLETE)) {
        /* (the rectangle's refusal also names the value it was given, the triangle's and every other call's does not: the
         * texts are as they were when the two had a body each, and a text is behaviour) */
        if (!square) rc = storm_dosage_measure_refusal(who, measure);
        else if (measure != STORM_DOSAGE_R2 && measure != STORM_DOSAGE_R)
            rc = storm_host_refuse(who, "measure %d must be 0 (STORM_DOSAGE_R2) or 1 (STORM_DOSAGE_R)", measure);
    }
    /* a triangle has a pair from two rows on; a rectangle from one row on either side */
    if (!rc && (square ? n_a != 0 && n_b != 0 : n_a >= 2)) {
        storm_hip_ctx_t* ctx = NULL;
        const storm_hip_matrix_t *ma = NULL, *mb = NULL;
        rc = storm_dosage_operands(a, square ? b : NULL, &ctx, &ma, &mb);
        if (!rc) rc = pairs_run(ctx, ma, mb, square, stat, measure, a->n_samples, out, out_ld, device);
    }
    return storm_host_end(rc);
}

int STORM_dosage_pairw_dot(STORM_dosage_t* h, uint32_t* out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_pairs(h, NULL, 0, DOT, 0, out, out_rows, out_ld, 0, "STORM_dosage_pairw_dot");
}
int STORM_dosage_pairw_dot_device(STORM_dosage_t* h, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_pairs(h, NULL, 0, DOT, 0, d_out, out_rows, out_ld, 1, "STORM_dosage_pairw_dot_device");
}
int STORM_dosage_pairw_corr(STORM_dosage_t* h, int measure, float* out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_pairs(h, NULL, 0, CORR, measure, out, out_rows, out_ld, 0, "STORM_dosage_pairw_corr");
}
int STORM_dosage_pairw_corr_device(STORM_dosage_t* h, int measure, float* d_out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_pairs(h, NULL, 0, CORR, measure, d_out, out_rows, out_ld, 1, "STORM_dosage_pairw_corr_device");
}
int STORM_dosage_pairw_nobs(STORM_dosage_t* h, uint32_t* out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_pairs(h, NULL, 0, NOBS, 0, out, out_rows, out_ld, 0, "STORM_dosage_pairw_nobs");
}
int STORM_dosage_pairw_nobs_device(STORM_dosage_t* h, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_pairs(h, NULL, 0, NOBS, 0, d_out, out_rows, out_ld, 1, "STORM_dosage_pairw_nobs_device");
}
int STORM_dosage_pairw_corr_complete(STORM_dosage_t* h, int measure, float* out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_pairs(h, NULL, 0, CORR_COMPLETE, measure, out, out_rows, out_ld, 0, "STORM_dosage_pairw_corr_complete");
}
int STORM_dosage_pairw_corr_complete_device(STORM_dosage_t* h, int measure, float* d_out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_pairs(h, NULL, 0, CORR_COMPLETE, measure, d_out, out_rows, out_ld, 1, "STORM_dosage_pairw_corr_complete_device");
}

int STORM_dosage_square_dot(STORM_dosage_t* a, STORM_dosage_t* b, uint32_t* out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_pairs(a, b, 1, DOT, 0, out, out_rows, out_ld, 0, "STORM_dosage_square_dot");
}
int STORM_dosage_square_dot_device(STORM_dosage_t* a, STORM_dosage_t* b, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_pairs(a, b, 1, DOT, 0, d_out, out_rows, out_ld, 1, "STORM_dosage_square_dot_device");
}
int STORM_dosage_square_corr(STORM_dosage_t* a, STORM_dosage_t* b, int measure, float* out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_pairs(a, b, 1, CORR, measure, out, out_rows, out_ld, 0, "STORM_dosage_square_corr");
}
int STORM_dosage_square_corr_device(STORM_dosage_t* a, STORM_dosage_t* b, int measure, float* d_out, uint64_t out_rows,
                                    uint64_t out_ld) {
    return dosage_pairs(a, b, 1, CORR, measure, d_out, out_rows, out_ld, 1, "STORM_dosage_square_corr_device");
}
int STORM_dosage_square_nobs(STORM_dosage_t* a, STORM_dosage_t* b, uint32_t* out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_pairs(a, b, 1, NOBS, 0, out, out_rows, out_ld, 0, "STORM_dosage_square_nobs");
}
int STORM_dosage_square_nobs_device(STORM_dosage_t* a, STORM_dosage_t* b, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld) {
    return dosage_pairs(a, b, 1, NOBS, 0, d_out, out_rows, out_ld, 1, "STORM_dosage_square_nobs_device");
}
int STORM_dosage_square_corr_complete(STORM_dosage_t* a, STORM_dosage_t* b, int measure, float* out, uint64_t out_rows,
                                      uint64_t out_ld) {
    return dosage_pairs(a, b, 1, CORR_COMPLETE, measure, out, out_rows, out_ld, 0, "STORM_dosage_square_corr_complete");
}
int STORM_dosage_square_corr_complete_device(STORM_dosage_t* a, STORM_dosage_t* b, int measure, float* d_out, uint64_t out_rows,
                                             uint64_t out_ld) {
    return dosage_pairs(a, b, 1, CORR_COMPLETE, measure, d_out, out_rows, out_ld, 1, "STORM_dosage_square_corr_complete_device");
}
