/* storm_lag.c — the per-pair matrices of one container for the pairs within max_lag rows of each other (storm.h:
 * STORM_contig_pairw_lag_matrix, STORM_pairw_lag_matrix, their similarity and _device forms): row i against the next L rows,
 * an n x L matrix in the lag layout (storm_hip.h: storm_hip_pairw_lag_matrix_device).
 *
 * On storm_host.c's locked paths without adding to them, like storm_square.c: the handle's device copy is kept exactly as
 * for STORM_pairw_matrix. A STORM_t always runs on its dense replica (built here when the handle has only its arena or its
 * row lists: there is no list-join form of the lag layout). One device slot and one process, host forms too. */
#include <stdint.h>
#include <stdio.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"

/* what = op (measure < 0) or the measure; the arguments as the shim takes them: 0, or -3 with the reason */
static int lag_args(const char* who, int op, int measure, uint64_t* n_bits, uint64_t n_bits_default, uint64_t max_lag) {
    char msg[200];
    if (max_lag == 0) {
        snprintf(msg, sizeof(msg), "%s: max_lag must be at least 1", who);
        storm_host_error(msg);
        return -3;
    }
    if (measure < 0) {
        if (op >= 0 && op <= 2) return 0;
        snprintf(msg, sizeof(msg), "%s: op must be 0 (and), 1 (or) or 2 (xor)", who);
        storm_host_error(msg);
        return -3;
    }
    if (measure > STORM_SIM_LD_R2) {
        snprintf(msg, sizeof(msg), "%s: measure must be 0 (Jaccard), 1 (cosine), 2 (LD D) or 3 (LD r^2)", who);
        storm_host_error(msg);
        return -3;
    }
    if (measure < STORM_SIM_LD_D) { /* Jaccard and cosine do not read n_bits */
        *n_bits = 1;
        return 0;
    }
    if (*n_bits == 0) *n_bits = n_bits_default;
    if (*n_bits == 0 || *n_bits > (1ull << 32)) {
        snprintf(msg, sizeof(msg), "%s: the LD measures need n_bits, the size of the universe, in [1, 2^32]%s", who,
                 n_bits_default ? "" : " (a STORM_t declares none: 0 is refused)");
        storm_host_error(msg);
        return -3;
    }
    return 0;
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
    if (rc != STORM_HIP_OK) {
        storm_host_device_error(measure < 0 ? "storm_hip_pairw_lag_matrix" : "storm_hip_pairw_lag_similarity");
        return -3;
    }
    return 0;
}

/* out_rows >= n and out_ld >= L = min(max_lag, n - 1) */
static int lag_fits(uint64_t n, uint64_t max_lag, uint64_t out_rows, uint64_t out_ld) {
    const uint64_t lag = n ? (max_lag < n - 1 ? max_lag : n - 1) : 0;
    return out_rows >= n && out_ld >= lag;
}

/* measure < 0: counts under op */
static int contig_lag(STORM_contiguous_t* h, int op, int measure, uint64_t n_bits, uint64_t max_lag, void* out,
                      uint64_t out_rows, uint64_t out_ld, int device, const char* who) {
    if (!h) return -1;
    if (!out) return -2;
    storm_host_lock();
    int rc = storm_host_one_slot_or_refuse(who);
    const uint64_t n = h->n_data;
    if (!rc && max_lag != 0 && !lag_fits(n, max_lag, out_rows, out_ld)) rc = -4;
    if (!rc) rc = lag_args(who, op, measure, &n_bits, h->vector_length, max_lag);
    if (!rc && n >= 2) {
        const storm_hip_matrix_t* m = storm_host_contig_matrix(h);
        storm_hip_ctx_t* ctx = m ? storm_host_ctx() : NULL;
        rc = ctx ? lag_run(ctx, m, op, measure, n_bits, max_lag, out, out_ld, device) : -3;
    }
    storm_host_unlock();
    return rc;
}

static int storm_lag(STORM_t* h, int op, int measure, uint64_t n_bits, uint64_t max_lag, void* out, uint64_t out_rows,
                     uint64_t out_ld, int device, const char* who) {
    if (!h) return -1;
    if (!out) return -2;
    storm_host_lock();
    int rc = storm_host_one_slot_or_refuse(who);
    const uint64_t n = h->n_conts;
    if (!rc && max_lag != 0 && !lag_fits(n, max_lag, out_rows, out_ld)) rc = -4;
    if (!rc) rc = lag_args(who, op, measure, &n_bits, 0, max_lag);
    if (!rc && n >= 2) {
        storm_hip_ctx_t* ctx = storm_host_ctx();
        /* the handle's state checked against the container as it is now; its dense replica, whatever else it keeps */
        sparse_state_t* st = ctx ? storm_host_checked_state(h) : NULL;
        if (!st || (!st->have_dense && storm_host_build(h, st, 1, NULL, 0))) rc = -3;
        else rc = lag_run(ctx, st->m[storm_host_slot()], op, measure, n_bits, max_lag, out, out_ld, device);
    }
    storm_host_unlock();
    return rc;
}

int STORM_contig_pairw_lag_matrix(STORM_contiguous_t* h, int op, uint64_t max_lag, uint32_t* out, uint64_t out_rows,
                                  uint64_t out_ld) {
    return contig_lag(h, op, -1, 0, max_lag, out, out_rows, out_ld, 0, "STORM_contig_pairw_lag_matrix");
}
int STORM_contig_pairw_lag_matrix_device(STORM_contiguous_t* h, int op, uint64_t max_lag, uint32_t* d_out, uint64_t out_rows,
                                         uint64_t out_ld) {
    return contig_lag(h, op, -1, 0, max_lag, d_out, out_rows, out_ld, 1, "STORM_contig_pairw_lag_matrix_device");
}
int STORM_contig_pairw_lag_similarity(STORM_contiguous_t* h, int measure, uint64_t n_bits, uint64_t max_lag, float* out,
                                      uint64_t out_rows, uint64_t out_ld) {
    return contig_lag(h, 0, measure < 0 ? STORM_SIM_LD_R2 + 1 : measure, n_bits, max_lag, out, out_rows, out_ld, 0,
                      "STORM_contig_pairw_lag_similarity");
}
int STORM_contig_pairw_lag_similarity_device(STORM_contiguous_t* h, int measure, uint64_t n_bits, uint64_t max_lag, float* d_out,
                                             uint64_t out_rows, uint64_t out_ld) {
    return contig_lag(h, 0, measure < 0 ? STORM_SIM_LD_R2 + 1 : measure, n_bits, max_lag, d_out, out_rows, out_ld, 1,
                      "STORM_contig_pairw_lag_similarity_device");
}
int STORM_pairw_lag_matrix(STORM_t* h, int op, uint64_t max_lag, uint32_t* out, uint64_t out_rows, uint64_t out_ld) {
    return storm_lag(h, op, -1, 0, max_lag, out, out_rows, out_ld, 0, "STORM_pairw_lag_matrix");
}
int STORM_pairw_lag_matrix_device(STORM_t* h, int op, uint64_t max_lag, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld) {
    return storm_lag(h, op, -1, 0, max_lag, d_out, out_rows, out_ld, 1, "STORM_pairw_lag_matrix_device");
}
int STORM_pairw_lag_similarity(STORM_t* h, int measure, uint64_t n_bits, uint64_t max_lag, float* out, uint64_t out_rows,
                               uint64_t out_ld) {
    return storm_lag(h, 0, measure < 0 ? STORM_SIM_LD_R2 + 1 : measure, n_bits, max_lag, out, out_rows, out_ld, 0,
                     "STORM_pairw_lag_similarity");
}
int STORM_pairw_lag_similarity_device(STORM_t* h, int measure, uint64_t n_bits, uint64_t max_lag, float* d_out, uint64_t out_rows,
                                      uint64_t out_ld) {
    return storm_lag(h, 0, measure < 0 ? STORM_SIM_LD_R2 + 1 : measure, n_bits, max_lag, d_out, out_rows, out_ld, 1,
                     "STORM_pairw_lag_similarity_device");
}
