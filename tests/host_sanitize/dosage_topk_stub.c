/* dosage_topk_stub.c — TEST ONLY. The dosage top-k entry points of the device library for dosage_topk_driver.c, beside
 * device_stub.c (whose matrix is host memory), dosage_complete_stub.c and dosage_band_stub.c: every call forms each entry
 * from the words that reached it, sample by sample on the CPU, ranks a row by insertion — value descending, then row
 * ascending, NaN no candidate — and writes exactly what the real call writes: columns [0, k) of the rows of `a`, padded
 * with idx 0xFFFFFFFF and val NaN (0 for the dot product). Never linked into the product. */
#include <string.h>

#include "stub_dosage.h"

#define NAN_BITS 0x7FC00000u

/* one entry: its value for the order, and the 32 bits the call writes; 0: no candidate */
static int entry(const storm_hip_matrix_t* a, uint64_t i, const storm_hip_matrix_t* b, uint64_t j, int score, int complete,
                 uint64_t n_samples, double* value, uint32_t* bits) {
    double N = 0, P = 0, sx = 0, sy = 0, qx = 0, qy = 0;
    for (uint64_t s = 0; s < n_samples; ++s) {
        const unsigned x = value_at(a, i, s), y = value_at(b, j, s);
        if (complete && (x == 3u || y == 3u)) continue;
        N += 1, P += x * y, sx += x, sy += y, qx += x * x, qy += y * y;
    }
    if (score == STORM_HIP_DOSAGE_TOPK_DOT) {
        *value = P;
        *bits = (uint32_t)P;
        return 1;
    }
    const double num = N * P - sx * sy, dx = N * qx - sx * sx, dy = N * qy - sy * sy;
    if (dx == 0 || dy == 0) return 0;
    const float f = (float)(score == STORM_HIP_DOSAGE_R2 ? num * num / (dx * dy) : num / sqrt(dx * dy));
    *value = f;
    memcpy(bits, &f, sizeof(*bits));
    return 1;
}

static int topk_call(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int self, int complete, int score,
                     uint64_t n_samples, uint64_t k, uint64_t panel_rows, uint32_t* idx, void* val_, uint64_t ld_k) {
    uint32_t* val = (uint32_t*)val_;
    if (!ctx || !a || !b || !idx || !val) return STORM_HIP_EINVAL;
    if (a->n_words != b->n_words || (n_samples + 31) / 32 != a->n_words || n_samples == 0) return STORM_HIP_EINVAL;
    if (score < 0 || score > (complete ? STORM_HIP_DOSAGE_R : STORM_HIP_DOSAGE_TOPK_DOT)) return STORM_HIP_EINVAL;
    if (k == 0 || k > STORM_HIP_TOPK_MAX || ld_k < k || panel_rows % 256u != 0) return STORM_HIP_EINVAL;
    double best[STORM_HIP_TOPK_MAX];
    for (uint64_t i = 0; i < a->n_rows; ++i) {
        uint32_t* const ri = idx + i * ld_k;
        uint32_t* const rv = val + i * ld_k;
        uint64_t have = 0;
        for (uint64_t j = 0; j < b->n_rows; ++j) {
            double v;
            uint32_t bits;
            if ((self && j == i) || !entry(a, i, b, j, score, complete, n_samples, &v, &bits)) continue;
            uint64_t at = have;                       /* behind every entry that is no worse: j ascends, so ties keep their order */
            while (at > 0 && best[at - 1] < v) --at;
            if (at >= k) continue;
            const uint64_t last = have < k ? have : k - 1;
            for (uint64_t t = last; t > at; --t) best[t] = best[t - 1], ri[t] = ri[t - 1], rv[t] = rv[t - 1];
            best[at] = v, ri[at] = (uint32_t)j, rv[at] = bits;
            if (have < k) ++have;
        }
        for (uint64_t t = have; t < k; ++t) ri[t] = 0xFFFFFFFFu, rv[t] = score == STORM_HIP_DOSAGE_TOPK_DOT ? 0u : NAN_BITS;
    }
    return STORM_HIP_OK;
}

#define FORMS(name, complete)                                                                                                         \
    int storm_hip_pairw_##name##_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int score, uint64_t n_samples, uint64_t k,  \
                                        uint64_t panel_rows, uint32_t* d_idx, void* d_val, uint64_t ld_k) {                            \
        return topk_call(ctx, m, m, 1, complete, score, n_samples, k, panel_rows, d_idx, d_val, ld_k);                                 \
    }                                                                                                                                  \
    int storm_hip_pairw_##name(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int score, uint64_t n_samples, uint64_t k,           \
                               uint64_t panel_rows, uint32_t* h_idx, void* h_val, uint64_t ld_k) {                                     \
        return topk_call(ctx, m, m, 1, complete, score, n_samples, k, panel_rows, h_idx, h_val, ld_k);                                 \
    }                                                                                                                                  \
    int storm_hip_square_##name##_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int score,    \
                                         uint64_t n_samples, uint64_t k, uint64_t panel_rows, uint32_t* d_idx, void* d_val,            \
                                         uint64_t ld_k) {                                                                              \
        return topk_call(ctx, a, b, 0, complete, score, n_samples, k, panel_rows, d_idx, d_val, ld_k);                                 \
    }                                                                                                                                  \
    int storm_hip_square_##name(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int score,             \
                                uint64_t n_samples, uint64_t k, uint64_t panel_rows, uint32_t* h_idx, void* h_val, uint64_t ld_k) {    \
        return topk_call(ctx, a, b, 0, complete, score, n_samples, k, panel_rows, h_idx, h_val, ld_k);                                 \
    }
FORMS(dosage_topk, 0)
FORMS(dosage_topk_complete, 1)
