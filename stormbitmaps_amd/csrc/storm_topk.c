/* storm_topk.c — for each row of a container its k most similar rows, selected on the device (storm.h:
 * STORM_contig_pairw_topk, STORM_pairw_topk, STORM_square_topk and their _device forms; storm_hip.h: storm_hip_pairw_topk,
 * storm_hip_cross_dense_topk).
 *
 * On storm_host.c's locked paths without adding to them, like storm_lag.c: the handle's device copy is kept exactly as for
 * STORM_pairw_matrix. A STORM_t always runs on its dense replica (built here when the handle has only its arena or its row
 * lists), two of them at their common width as in storm_square.c: there is no list-join form of the selection. One
 * device slot and one process, host forms too. */
#include <stdint.h>
#include <stdio.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"

/* the arguments as the shim takes them: 0, or -3 with the reason. n_bits_default: what 0 stands for (0: refused) */
static int topk_args(const char* who, int score, uint64_t* n_bits, uint64_t n_bits_default, uint64_t k, uint64_t panel_rows) {
    char msg[220];
    if (score < STORM_SIM_JACCARD || score > STORM_TOPK_COUNT) {
        snprintf(msg, sizeof(msg), "%s: score must be 0 (Jaccard), 1 (cosine), 2 (LD D), 3 (LD r^2) or 4 (the AND count)", who);
        storm_host_error(msg);
        return -3;
    }
    if (k == 0 || k > STORM_TOPK_MAX) {
        snprintf(msg, sizeof(msg), "%s: k must be in [1, %d]", who, STORM_TOPK_MAX);
        storm_host_error(msg);
        return -3;
    }
    if (panel_rows % 256u != 0) {
        snprintf(msg, sizeof(msg), "%s: panel_rows must be 0 (chosen by the library) or a multiple of 256", who);
        storm_host_error(msg);
        return -3;
    }
    if (score != STORM_SIM_LD_D && score != STORM_SIM_LD_R2) { /* only the LD measures read n_bits */
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

/* the shim call on dense operands (b == NULL: the rows of `a` among themselves): 0 or -3 */
static int topk_run(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int score, uint64_t n_bits,
                    uint64_t k, uint64_t panel_rows, uint32_t* idx, void* val, uint64_t out_ld, int device) {
    int rc;
    if (!b)
        rc = device ? storm_hip_pairw_topk_device(ctx, a, score, n_bits, k, panel_rows, idx, val, out_ld)
                    : storm_hip_pairw_topk(ctx, a, score, n_bits, k, panel_rows, idx, val, out_ld);
    else
        rc = device ? storm_hip_cross_dense_topk_device(ctx, a, b, score, n_bits, k, panel_rows, idx, val, out_ld)
                    : storm_hip_cross_dense_topk(ctx, a, b, score, n_bits, k, panel_rows, idx, val, out_ld);
    if (rc != STORM_HIP_OK) {
        storm_host_device_error(b ? "storm_hip_cross_dense_topk" : "storm_hip_pairw_topk");
        return -3;
    }
    return 0;
}

static int contig_topk(STORM_contiguous_t* h, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* idx,
                       void* val, uint64_t out_rows, uint64_t out_ld, int device, const char* who) {
    if (!h) return -1;
    if (!idx || !val) return -2;
    storm_host_lock();
    int rc = storm_host_one_slot_or_refuse(who);
    const uint64_t n = h->n_data;
    if (!rc && (out_rows < n || out_ld < k)) rc = -4;
    if (!rc) rc = topk_args(who, score, &n_bits, h->vector_length, k, panel_rows);
    if (!rc && n != 0) {
        const storm_hip_matrix_t* m = storm_host_contig_matrix(h);
        storm_hip_ctx_t* ctx = m ? storm_host_ctx() : NULL;
        rc = ctx ? topk_run(ctx, m, NULL, score, n_bits, k, panel_rows, idx, val, out_ld, device) : -3;
    }
    storm_host_unlock();
    return rc;
}

static int storm_topk(STORM_t* h, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* idx, void* val,
                      uint64_t out_rows, uint64_t out_ld, int device, const char* who) {
    if (!h) return -1;
    if (!idx || !val) return -2;
    storm_host_lock();
    int rc = storm_host_one_slot_or_refuse(who);
    const uint64_t n = h->n_conts;
    if (!rc && (out_rows < n || out_ld < k)) rc = -4;
    if (!rc) rc = topk_args(who, score, &n_bits, 0, k, panel_rows);
    if (!rc && n != 0) {
        storm_hip_ctx_t* ctx = storm_host_ctx();
        /* the handle's state checked against the container as it is now; its dense replica, whatever else it keeps */
        sparse_state_t* st = ctx ? storm_host_checked_state(h) : NULL;
        if (!st || (!st->have_dense && storm_host_build(h, st, 1, NULL, 0))) rc = -3;
        else rc = topk_run(ctx, st->m[storm_host_slot()], NULL, score, n_bits, k, panel_rows, idx, val, out_ld, device);
    }
    storm_host_unlock();
    return rc;
}

/* a's rows against b's */
static int square_topk(STORM_t* a, STORM_t* b, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* idx,
                       void* val, uint64_t out_rows, uint64_t out_ld, int device, const char* who) {
    if (!a || !b) return -1;
    if (!idx || !val) return -2;
    storm_host_lock();
    int rc = storm_host_one_slot_or_refuse(who);
    if (!rc && (out_rows < a->n_conts || out_ld < k)) rc = -4;
    if (!rc) rc = topk_args(who, score, &n_bits, 0, k, panel_rows);
    if (!rc && a->n_conts != 0) {
        storm_hip_ctx_t* ctx = storm_host_ctx();
        const int slot = storm_host_slot();
        sparse_state_t* sa = ctx ? storm_host_checked_state(a) : NULL;
        if (!sa) rc = -3;
        else if (b->n_conts == 0) { /* nothing to list: every row of `a` is k paddings, against an empty matrix of a's width */
            storm_hip_matrix_t* none = NULL;
            if (!sa->have_dense && storm_host_build(a, sa, 1, NULL, 0)) rc = -3;
            else if (storm_hip_matrix_create(ctx, 0, storm_hip_matrix_words(sa->m[slot]), &none) != STORM_HIP_OK) {
                storm_host_device_error("storm_hip_matrix_create");
                rc = -3;
            } else {
                rc = topk_run(ctx, sa->m[slot], none, score, n_bits, k, panel_rows, idx, val, out_ld, device);
                storm_hip_matrix_destroy(ctx, none);
            }
        } else {
            sparse_state_t* sb = b != a ? storm_host_checked_state(b) : sa;
            if (!sb || storm_host_common_dense(a, sa, b, sb, slot)) rc = -3;
            else rc = topk_run(ctx, sa->m[slot], sb->m[slot], score, n_bits, k, panel_rows, idx, val, out_ld, device);
        }
    }
    storm_host_unlock();
    return rc;
}

int STORM_contig_pairw_topk(STORM_contiguous_t* h, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* idx,
                            void* val, uint64_t out_rows, uint64_t out_ld) {
    return contig_topk(h, score, n_bits, k, panel_rows, idx, val, out_rows, out_ld, 0, "STORM_contig_pairw_topk");
}
int STORM_contig_pairw_topk_device(STORM_contiguous_t* h, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows,
                                   uint32_t* d_idx, void* d_val, uint64_t out_rows, uint64_t out_ld) {
    return contig_topk(h, score, n_bits, k, panel_rows, d_idx, d_val, out_rows, out_ld, 1, "STORM_contig_pairw_topk_device");
}
int STORM_pairw_topk(STORM_t* h, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* idx, void* val,
                     uint64_t out_rows, uint64_t out_ld) {
    return storm_topk(h, score, n_bits, k, panel_rows, idx, val, out_rows, out_ld, 0, "STORM_pairw_topk");
}
int STORM_pairw_topk_device(STORM_t* h, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* d_idx, void* d_val,
                            uint64_t out_rows, uint64_t out_ld) {
    return storm_topk(h, score, n_bits, k, panel_rows, d_idx, d_val, out_rows, out_ld, 1, "STORM_pairw_topk_device");
}
int STORM_square_topk(STORM_t* a, STORM_t* b, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* idx,
                      void* val, uint64_t out_rows, uint64_t out_ld) {
    return square_topk(a, b, score, n_bits, k, panel_rows, idx, val, out_rows, out_ld, 0, "STORM_square_topk");
}
int STORM_square_topk_device(STORM_t* a, STORM_t* b, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* d_idx,
                             void* d_val, uint64_t out_rows, uint64_t out_ld) {
    return square_topk(a, b, score, n_bits, k, panel_rows, d_idx, d_val, out_rows, out_ld, 1, "STORM_square_topk_device");
}
