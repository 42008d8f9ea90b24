/* storm_lag.c — the per-pair matrices of one container for the pairs within max_lag rows of each other (storm.h:
 * STORM_contig_pairw_lag_matrix, STORM_pairw_lag_matrix, their similarity and _device forms): row i against the next L rows,
 * an n x L matrix in the lag layout (storm_hip.h: storm_hip_pairw_lag_matrix_device).
 *
 * On storm_host.c's locked paths without adding to them, like storm_square.c: the handle's device copy is kept exactly as
 * for STORM_pairw_matrix. A STORM_t always runs on its dense replica (built here when the handle has only its arena or its
 * row lists: there is no list-join form of the lag layout). One device slot and one process, host forms too. */
#include <stdint.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"

/* what = op (measure < 0) or the measure; the arguments as the shim takes them: 0, or -3 with the reason */
static int lag_args(const char* who, int op, int measure, uint64_t* n_bits, uint64_t n_bits_default, uint64_t max_lag) {
    if (max_lag == 0) return storm_host_refuse(who, "max_lag must be at least 1");
    if (measure < 0) return op >= 0 && op <= 2 ? 0 : storm_host_refuse(who, "op must be 0 (and), 1 (or) or 2 (xor)");
    if (measure > STORM_SIM_LD_R2)
        return storm_host_refuse(who, "measure must be 0 (Jaccard), 1 (cosine), 2 (LD D) or 3 (LD r^2)");
    if (measure < STORM_SIM_LD_D) { /* Jaccard and cosine do not read n_bits */
        *n_bits = 1;
        return 0;
    }
    return storm_host_ld_n_bits(who, n_bits, n_bits_default);
}

/* the shim call on the dense operand `m`: 0 or -3 */
static int lag_run(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int op, int measure, uint64_t n_bits, uint64_t max_lag,
                   void* out, uint64_t out_ld, int device) {
    int rc;
    if (measure < 0)
        rc = device ? storm_hip_pairw_lag_matrix_device(ctx, m, op, max_lag, 0, ~0ull, (uint32_t*)out, out_ld)
                    : storm_hip_pairw_lag_matrix(ctx, m, op, max_lag, (uint32_t*)out, out_ld);
    else
        rc = device ? storm_hip_pairw_lag_similarity_device(ctx, m, measure, n_bits, max_lag, (float*)out, out_ld)
                    : storm_hip_pairw_lag_similarity(ctx, m, measure, n_bits, max_lag, (float*)out, out_ld);
    return storm_host_shim_result(ctx, rc, 0, measure < 0 ? "storm_hip_pairw_lag_matrix" : "storm_hip_pairw_lag_similarity");
}

/* out_rows >= n and out_ld >= L = min(max_lag, n - 1) */
static int lag_fits(uint64_t n, uint64_t max_lag, uint64_t out_rows, uint64_t out_ld) {
    const uint64_t lag = n ? (max_lag < n - 1 ? max_lag : n - 1) : 0;
    return out_rows >= n && out_ld >= lag;
}

/* exactly one of c and s is the caller's handle, which may be NULL. measure < 0: counts under op */
static int lag_call(STORM_contiguous_t* c, STORM_t* s, int op, int measure, uint64_t n_bits, uint64_t max_lag, void* out,
                    uint64_t out_rows, uint64_t out_ld, int device, const char* who) {
    if (!c && !s) return -1;
    if (!out) return -2;
    int rc = storm_host_begin(who);
    const uint64_t n = c ? c->n_data : s->n_conts;
    if (!rc && max_lag != 0 && !lag_fits(n, max_lag, out_rows, out_ld)) rc = -4;
    if (!rc) rc = lag_args(who, op, measure, &n_bits, c ? c->vector_length : 0, max_lag);
    if (!rc && n >= 2) {
        storm_hip_ctx_t* ctx = NULL;
        const storm_hip_matrix_t* m = NULL;
        rc = c ? storm_host_contig_operand(c, &ctx, &m) : storm_host_dense_operand(s, &ctx, &m);
        if (!rc) rc = lag_run(ctx, m, op, measure, n_bits, max_lag, out, out_ld, device);
    }
    return storm_host_end(rc);
}

int STORM_contig_pairw_lag_matrix(STORM_contiguous_t* h, int op, uint64_t max_lag, uint32_t* out, uint64_t out_rows,
                                  uint64_t out_ld) {
    return lag_call(h, NULL, op, -1, 0, max_lag, out, out_rows, out_ld, 0, "STORM_contig_pairw_lag_matrix");
}
int STORM_contig_pairw_lag_matrix_device(STORM_contiguous_t* h, int op, uint64_t max_lag, uint32_t* d_out, uint64_t out_rows,
                                         uint64_t out_ld) {
    return lag_call(h, NULL, op, -1, 0, max_lag, d_out, out_rows, out_ld, 1, "STORM_contig_pairw_lag_matrix_device");
}
int STORM_contig_pairw_lag_similarity(STORM_contiguous_t* h, int measure, uint64_t n_bits, uint64_t max_lag, float* out,
                                      uint64_t out_rows, uint64_t out_ld) {
    return lag_call(h, NULL, 0, measure < 0 ? STORM_SIM_LD_R2 + 1 : measure, n_bits, max_lag, out, out_rows, out_ld, 0,
                    "STORM_contig_pairw_lag_similarity");
}
int STORM_contig_pairw_lag_similarity_device(STORM_contiguous_t* h, int measure, uint64_t n_bits, uint64_t max_lag, float* d_out,
                                             uint64_t out_rows, uint64_t out_ld) {
    return lag_call(h, NULL, 0, measure < 0 ? STORM_SIM_LD_R2 + 1 : measure, n_bits, max_lag, d_out, out_rows, out_ld, 1,
                      "STORM_contig_pairw_lag_similarity_device");
}
int STORM_pairw_lag_matrix(STORM_t* h, int op, uint64_t max_lag, uint32_t* out, uint64_t out_rows, uint64_t out_ld) {
    return lag_call(NULL, h, op, -1, 0, max_lag, out, out_rows, out_ld, 0, "STORM_pairw_lag_matrix");
}
int STORM_pairw_lag_matrix_device(STORM_t* h, int op, uint64_t max_lag, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld) {
    return lag_call(NULL, h, op, -1, 0, max_lag, d_out, out_rows, out_ld, 1, "STORM_pairw_lag_matrix_device");
}
int STORM_pairw_lag_similarity(STORM_t* h, int measure, uint64_t n_bits, uint64_t max_lag, float* out, uint64_t out_rows,
                               uint64_t out_ld) {
    return lag_call(NULL, h, 0, measure < 0 ? STORM_SIM_LD_R2 + 1 : measure, n_bits, max_lag, out, out_rows, out_ld, 0,
                     "STORM_pairw_lag_similarity");
}
int STORM_pairw_lag_similarity_device(STORM_t* h, int measure, uint64_t n_bits, uint64_t max_lag, float* d_out, uint64_t out_rows,
                                      uint64_t out_ld) {
    return lag_call(NULL, h, 0, measure < 0 ? STORM_SIM_LD_R2 + 1 : measure, n_bits, max_lag, d_out, out_rows, out_ld, 1,
                     "STORM_pairw_lag_similarity_device");
}
