/* dosage_complete_stub.c — TEST ONLY. The dosage entry points of the device library for dosage_complete_driver.c, beside
 * device_stub.c (whose matrix is host memory): every call computes its result from the words that reached it, sample by
 * sample on the CPU, and writes exactly the window the real call writes. Here the row sums and the triangle's dot products
 * and correlations (the five calls dosage_driver.c answers itself); the rectangle and the calls that read 3 as "missing"
 * are dosage_pairs_stub.c's. Never linked into the product. */

#include "stub_dosage.h"

static uint32_t dot(const storm_hip_matrix_t* a, uint64_t i, const storm_hip_matrix_t* b, uint64_t j) {
    uint32_t p = 0;
    for (uint64_t s = 0; s < (uint64_t)a->n_words * 32; ++s) p += value_at(a, i, s) * value_at(b, j, s);
    return p;
}

int storm_hip_dosage_row_sums(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint32_t* h_sum, uint32_t* h_sum_sq) {
    (void)ctx;
    for (uint64_t i = 0; i < m->n_rows; ++i) {
        h_sum[i] = h_sum_sq[i] = 0;
        for (uint64_t s = 0; s < (uint64_t)m->n_words * 32; ++s) {
            h_sum[i] += value_at(m, i, s);
            h_sum_sq[i] += value_at(m, i, s) * value_at(m, i, s);
        }
    }
    return STORM_HIP_OK;
}
int storm_hip_pairw_dosage_matrix_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint32_t* d_out, uint64_t ld) {
    (void)ctx;
    if (ld < m->n_rows) return STORM_HIP_EINVAL;
    for (uint64_t i = 0; i < m->n_rows; ++i)
        for (uint64_t j = i + 1; j < m->n_rows; ++j) d_out[i * ld + j] = dot(m, i, m, j);
    return STORM_HIP_OK;
}
int storm_hip_pairw_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint32_t* h_out, uint64_t ld) {
    for (uint64_t i = 0; i < m->n_rows; ++i)
        for (uint64_t j = 0; j < m->n_rows; ++j) h_out[i * ld + j] = 0;
    return storm_hip_pairw_dosage_matrix_device(ctx, m, h_out, ld);
}
int storm_hip_pairw_dosage_corr_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                       float* d_out, uint64_t ld) {
    (void)ctx;
    if (ld < m->n_rows || (n_samples + 31) / 32 != m->n_words || measure < 0 || measure > 1) return STORM_HIP_EINVAL;
    for (uint64_t i = 0; i < m->n_rows; ++i) /* (touches the window the real call writes) */
        for (uint64_t j = i + 1; j < m->n_rows; ++j) d_out[i * ld + j] = 0.5f;
    return STORM_HIP_OK;
}
int storm_hip_pairw_dosage_corr(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples, float* h_out,
                                uint64_t ld) {
    for (uint64_t i = 0; i < m->n_rows; ++i)
        for (uint64_t j = 0; j < m->n_rows; ++j) h_out[i * ld + j] = 0.0f;
    return storm_hip_pairw_dosage_corr_device(ctx, m, measure, n_samples, h_out, ld);
}
