/* storm_topk.c — for each row of a container its k most similar rows, selected on the device (storm.h:
 * STORM_contig_pairw_topk, STORM_pairw_topk, STORM_square_topk and their _device forms; storm_hip.h: storm_hip_pairw_topk,
 * storm_hip_cross_dense_topk).
 *
 * On storm_host.c's locked paths without adding to them, like storm_lag.c: the handle's device copy is kept exactly as for
 * STORM_pairw_matrix. A STORM_t always runs on its dense replica (built here when the handle has only its arena or its row
 * lists), two of them at their common width as in storm_square.c: there is no list-join form of the selection. One
 * device slot and one process, host forms too. */
#include <stdint.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"

/* the arguments as the shim takes them: 0, or -3 with the reason. n_bits_default: what 0 stands for (0: refused) */
static int topk_args(const char* who, int score, uint64_t* n_bits, uint64_t n_bits_default, uint64_t k, uint64_t panel_rows) {
    if (score < STORM_SIM_JACCARD || score > STORM_TOPK_COUNT)
        return storm_host_refuse(who, "score must be 0 (Jaccard), 1 (cosine), 2 (LD D), 3 (LD r^2) or 4 (the AND count)");
    if (k == 0 || k > STORM_TOPK_MAX) return storm_host_refuse(who, "k must be in [1, %d]", STORM_TOPK_MAX);
    if (panel_rows % 256u != 0)
        return storm_host_refuse(who, "panel_rows must be 0 (chosen by the library) or a multiple of 256");
    if (score != STORM_SIM_LD_D && score != STORM_SIM_LD_R2) { /* only the LD measures read n_bits */
        *n_bits = 1;
        return 0;
    }
    return storm_host_ld_n_bits(who, n_bits, n_bits_default);
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
    return storm_host_shim_result(ctx, rc, 0, b ? "storm_hip_cross_dense_topk" : "storm_hip_pairw_topk");
}

/* the rows of one container among themselves: exactly one of c and s is the caller's handle, which may be NULL */
static int pairw_topk(STORM_contiguous_t* c, STORM_t* s, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* idx,
                      void* val, uint64_t out_rows, uint64_t out_ld, int device, const char* who) {
    if (!c && !s) return -1;
    if (!idx || !val) return -2;
    int rc = storm_host_begin(who);
    const uint64_t n = c ? c->n_data : s->n_conts;
    if (!rc && (out_rows < n || out_ld < k)) rc = -4;
    if (!rc) rc = topk_args(who, score, &n_bits, c ? c->vector_length : 0, k, panel_rows);
    if (!rc && n != 0) {
        storm_hip_ctx_t* ctx = NULL;
        const storm_hip_matrix_t* m = NULL;
        rc = c ? storm_host_contig_operand(c, &ctx, &m) : storm_host_dense_operand(s, &ctx, &m);
        if (!rc) rc = topk_run(ctx, m, NULL, score, n_bits, k, panel_rows, idx, val, out_ld, device);
    }
    return storm_host_end(rc);
}

/* a's rows against b's */
static int square_topk(STORM_t* a, STORM_t* b, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* idx,
                       void* val, uint64_t out_rows, uint64_t out_ld, int device, const char* who) {
    if (!a || !b) return -1;
    if (!idx || !val) return -2;
    int rc = storm_host_begin(who);
    if (!rc && (out_rows < a->n_conts || out_ld < k)) rc = -4;
    if (!rc) rc = topk_args(who, score, &n_bits, 0, k, panel_rows);
    storm_hip_ctx_t* ctx = NULL;
    const storm_hip_matrix_t* ma = NULL;
    if (!rc && a->n_conts != 0 && b->n_conts == 0) {
        /* nothing to list: every row of `a` is k paddings, against an empty matrix of a's width */
        storm_hip_matrix_t* none = NULL;
        rc = storm_host_dense_operand(a, &ctx, &ma);
        if (!rc)
            rc = storm_host_shim_result(ctx, storm_hip_matrix_create(ctx, 0, storm_hip_matrix_words(ma), &none), 0,
                                        "storm_hip_matrix_create");
        if (!rc) {
            rc = topk_run(ctx, ma, none, score, n_bits, k, panel_rows, idx, val, out_ld, device);
            storm_hip_matrix_destroy(ctx, none);
        }
    } else if (!rc && a->n_conts != 0) {
        const int slot = storm_host_slot();
        sparse_state_t* sa = (ctx = storm_host_ctx()) ? storm_host_checked_state(a) : NULL;
        sparse_state_t* sb = sa && b != a ? storm_host_checked_state(b) : sa;
        if (!sb || storm_host_common_dense(a, sa, b, sb, slot)) rc = -3;
        else rc = topk_run(ctx, sa->m[slot], sb->m[slot], score, n_bits, k, panel_rows, idx, val, out_ld, device);
    }
    return storm_host_end(rc);
}

int STORM_contig_pairw_topk(STORM_contiguous_t* h, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* idx,
                            void* val, uint64_t out_rows, uint64_t out_ld) {
    return pairw_topk(h, NULL, score, n_bits, k, panel_rows, idx, val, out_rows, out_ld, 0, "STORM_contig_pairw_topk");
}
int STORM_contig_pairw_topk_device(STORM_contiguous_t* h, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows,
                                   uint32_t* d_idx, void* d_val, uint64_t out_rows, uint64_t out_ld) {
    return pairw_topk(h, NULL, score, n_bits, k, panel_rows, d_idx, d_val, out_rows, out_ld, 1, "STORM_contig_pairw_topk_device");
}
int STORM_pairw_topk(STORM_t* h, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* idx, void* val,
                     uint64_t out_rows, uint64_t out_ld) {
    return pairw_topk(NULL, h, score, n_bits, k, panel_rows, idx, val, out_rows, out_ld, 0, "STORM_pairw_topk");
}
int STORM_pairw_topk_device(STORM_t* h, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* d_idx, void* d_val,
                            uint64_t out_rows, uint64_t out_ld) {
    return pairw_topk(NULL, h, score, n_bits, k, panel_rows, d_idx, d_val, out_rows, out_ld, 1, "STORM_pairw_topk_device");
}
int STORM_square_topk(STORM_t* a, STORM_t* b, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* idx,
                      void* val, uint64_t out_rows, uint64_t out_ld) {
    return square_topk(a, b, score, n_bits, k, panel_rows, idx, val, out_rows, out_ld, 0, "STORM_square_topk");
}
int STORM_square_topk_device(STORM_t* a, STORM_t* b, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* d_idx,
                             void* d_val, uint64_t out_rows, uint64_t out_ld) {
    return square_topk(a, b, score, n_bits, k, panel_rows, d_idx, d_val, out_rows, out_ld, 1, "STORM_square_topk_device");
}
