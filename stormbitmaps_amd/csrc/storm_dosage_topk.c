/* storm_dosage_topk.c — for each row of a dosage container its k best rows by r^2, r or the dot product, selected on the
 * device (storm.h: STORM_dosage_pairw_topk, STORM_dosage_square_topk, their _complete and _device forms; storm_hip.h:
 * storm_hip_pairw_dosage_topk, storm_hip_square_dosage_topk). The container, its device copy and the locked paths are
 * storm_dosage.c's, as in storm_dosage_pairs.c; arguments and return codes are those of STORM_dosage_square_corr and
 * STORM_square_topk. Every refusal comes before the device is touched. No CPU fallback. */
#include <stdint.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"
#include "storm_dosage_internal.h"

/* the arguments as the shim takes them: 0, or -3 with the reason */
static int topk_args(const char* who, int score, int complete, uint64_t k, uint64_t panel_rows) {
    if (score != STORM_DOSAGE_R2 && score != STORM_DOSAGE_R && (complete || score != STORM_DOSAGE_TOPK_DOT))
        return storm_host_refuse(who, "score must be 0 (STORM_DOSAGE_R2)%s",
                                 complete ? " or 1 (STORM_DOSAGE_R): the dot product has no pairwise-complete form"
                                          : ", 1 (STORM_DOSAGE_R) or 2 (STORM_DOSAGE_TOPK_DOT)");
    if (k == 0 || k > STORM_TOPK_MAX) return storm_host_refuse(who, "k must be in [1, %d]", STORM_TOPK_MAX);
    if (panel_rows % 256u != 0)
        return storm_host_refuse(who, "panel_rows must be 0 (chosen by the library) or a multiple of 256");
    return 0;
}

/* b == NULL: the rows of `a` among themselves. An empty b travels as its (empty) device copy: every row of a is k paddings. */
static int dosage_topk(STORM_dosage_t* a, STORM_dosage_t* b, int have_b, int complete, int score, uint64_t k, uint64_t panel_rows,
                       uint32_t* idx, void* val, uint64_t out_rows, uint64_t out_ld, int device, const char* who) {
    if (!a || (have_b && !b)) return -1;
    if (!idx || !val) return -2;
    int rc = storm_host_begin(who);
    if (!rc && (out_rows < a->n_rows || out_ld < k)) rc = -4;
    if (!rc) rc = topk_args(who, score, complete, k, panel_rows);
    if (!rc && have_b) rc = storm_dosage_samples_refusal(who, a, b);
    if (!rc && a->n_rows != 0) {
        storm_hip_ctx_t* ctx = NULL;
        const storm_hip_matrix_t *ma = NULL, *mb = NULL;
        const uint64_t S = a->n_samples;
        rc = storm_dosage_operands(a, b, &ctx, &ma, &mb);
        if (!rc) {
            int hrc;
            const char* name;
            if (!have_b) {
                name = complete ? "storm_hip_pairw_dosage_topk_complete" : "storm_hip_pairw_dosage_topk";
                if (complete)
                    hrc = device ? storm_hip_pairw_dosage_topk_complete_device(ctx, ma, score, S, k, panel_rows, idx, val, out_ld)
                                 : storm_hip_pairw_dosage_topk_complete(ctx, ma, score, S, k, panel_rows, idx, val, out_ld);
                else
                    hrc = device ? storm_hip_pairw_dosage_topk_device(ctx, ma, score, S, k, panel_rows, idx, val, out_ld)
                                 : storm_hip_pairw_dosage_topk(ctx, ma, score, S, k, panel_rows, idx, val, out_ld);
            } else {
                name = complete ? "storm_hip_square_dosage_topk_complete" : "storm_hip_square_dosage_topk";
                if (complete)
                    hrc = device ? storm_hip_square_dosage_topk_complete_device(ctx, ma, mb, score, S, k, panel_rows, idx, val, out_ld)
                                 : storm_hip_square_dosage_topk_complete(ctx, ma, mb, score, S, k, panel_rows, idx, val, out_ld);
                else
                    hrc = device ? storm_hip_square_dosage_topk_device(ctx, ma, mb, score, S, k, panel_rows, idx, val, out_ld)
                                 : storm_hip_square_dosage_topk(ctx, ma, mb, score, S, k, panel_rows, idx, val, out_ld);
            }
            rc = storm_host_shim_result(ctx, hrc, 0, name);
        }
    }
    return storm_host_end(rc);
}

int STORM_dosage_pairw_topk(STORM_dosage_t* h, int score, uint64_t k, uint64_t panel_rows, uint32_t* idx, void* val,
                            uint64_t out_rows, uint64_t out_ld) {
    return dosage_topk(h, NULL, 0, 0, score, k, panel_rows, idx, val, out_rows, out_ld, 0, "STORM_dosage_pairw_topk");
}
int STORM_dosage_pairw_topk_device(STORM_dosage_t* h, int score, uint64_t k, uint64_t panel_rows, uint32_t* d_idx, void* d_val,
                                   uint64_t out_rows, uint64_t out_ld) {
    return dosage_topk(h, NULL, 0, 0, score, k, panel_rows, d_idx, d_val, out_rows, out_ld, 1, "STORM_dosage_pairw_topk_device");
}
int STORM_dosage_pairw_topk_complete(STORM_dosage_t* h, int score, uint64_t k, uint64_t panel_rows, uint32_t* idx, void* val,
                                     uint64_t out_rows, uint64_t out_ld) {
    return dosage_topk(h, NULL, 0, 1, score, k, panel_rows, idx, val, out_rows, out_ld, 0, "STORM_dosage_pairw_topk_complete");
}
int STORM_dosage_pairw_topk_complete_device(STORM_dosage_t* h, int score, uint64_t k, uint64_t panel_rows, uint32_t* d_idx,
                                            void* d_val, uint64_t out_rows, uint64_t out_ld) {
    return dosage_topk(h, NULL, 0, 1, score, k, panel_rows, d_idx, d_val, out_rows, out_ld, 1,
                       "STORM_dosage_pairw_topk_complete_device");
}
int STORM_dosage_square_topk(STORM_dosage_t* a, STORM_dosage_t* b, int score, uint64_t k, uint64_t panel_rows, uint32_t* idx,
                             void* val, uint64_t out_rows, uint64_t out_ld) {
    return dosage_topk(a, b, 1, 0, score, k, panel_rows, idx, val, out_rows, out_ld, 0, "STORM_dosage_square_topk");
}
int STORM_dosage_square_topk_device(STORM_dosage_t* a, STORM_dosage_t* b, int score, uint64_t k, uint64_t panel_rows,
                                    uint32_t* d_idx, void* d_val, uint64_t out_rows, uint64_t out_ld) {
    return dosage_topk(a, b, 1, 0, score, k, panel_rows, d_idx, d_val, out_rows, out_ld, 1, "STORM_dosage_square_topk_device");
}
int STORM_dosage_square_topk_complete(STORM_dosage_t* a, STORM_dosage_t* b, int score, uint64_t k, uint64_t panel_rows,
                                      uint32_t* idx, void* val, uint64_t out_rows, uint64_t out_ld) {
    return dosage_topk(a, b, 1, 1, score, k, panel_rows, idx, val, out_rows, out_ld, 0, "STORM_dosage_square_topk_complete");
}
int STORM_dosage_square_topk_complete_device(STORM_dosage_t* a, STORM_dosage_t* b, int score, uint64_t k, uint64_t panel_rows,
                                             uint32_t* d_idx, void* d_val, uint64_t out_rows, uint64_t out_ld) {
    return dosage_topk(a, b, 1, 1, score, k, panel_rows, d_idx, d_val, out_rows, out_ld, 1,
                       "STORM_dosage_square_topk_complete_device");
}
