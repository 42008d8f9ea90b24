/* dosage_pairs_stub.c — TEST ONLY. The dosage entry points of the device library that storm_dosage_pairs.c and
 * STORM_dosage_row_missing call beyond the five dosage_complete_stub.c (or dosage_driver.c, with its own) answers: the
 * rectangle of two matrices and the calls that read 3 as "missing", beside device_stub.c (whose matrix is host memory).
 * Every call computes its result from the words that reached it, sample by sample on the CPU, and writes exactly the window
 * the real call writes. Never linked into the product. */
#include "stub_dosage.h"

/* row i of a against row j of b: the dot product, the samples neither of which is missing, and r^2 or r */
static uint32_t dot(const storm_hip_matrix_t* a, uint64_t i, const storm_hip_matrix_t* b, uint64_t j) {
    uint32_t p = 0;
    for (uint64_t s = 0; s < (uint64_t)a->n_words * 32; ++s) p += value_at(a, i, s) * value_at(b, j, s);
    return p;
}
static uint32_t shared(const storm_hip_matrix_t* a, uint64_t i, const storm_hip_matrix_t* b, uint64_t j, uint64_t n_samples) {
    uint32_t n = 0;
    for (uint64_t s = 0; s < n_samples; ++s) n += value_at(a, i, s) != 3u && value_at(b, j, s) != 3u;
    return n;
}
static float corr(const storm_hip_matrix_t* a, uint64_t i, const storm_hip_matrix_t* b, uint64_t j, int measure, int missing,
                  uint64_t n_samples) {
    double N = 0, P = 0, sx = 0, sy = 0, qx = 0, qy = 0;
    for (uint64_t s = 0; s < n_samples; ++s) {
        const unsigned x = value_at(a, i, s), y = value_at(b, j, s);
        if (missing && (x == 3u || y == 3u)) continue;
        N += 1, P += x * y, sx += x, sy += y, qx += x * x, qy += y * y;
    }
    const double num = N * P - sx * sy, dx = N * qx - sx * sx, dy = N * qy - sy * sy;
    return dx == 0 || dy == 0 ? NAN : (float)(measure == 0 ? num * num / (dx * dy) : num / sqrt(dx * dy));
}
static int square_refusal(const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, uint64_t n_samples, uint64_t ld) {
    return a->n_words != b->n_words || ld < b->n_rows || (n_samples + 31) / 32 != a->n_words;
}

/* ---- the rectangle: the whole n_a x n_b window, host and _device forms alike ---- */
int storm_hip_square_dosage_matrix_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,
                                          uint32_t* d_out, uint64_t ld) {
    (void)ctx;
    if (a->n_words != b->n_words || ld < b->n_rows) return STORM_HIP_EINVAL;
    for (uint64_t i = 0; i < a->n_rows; ++i)
        for (uint64_t j = 0; j < b->n_rows; ++j) d_out[i * ld + j] = dot(a, i, b, j);
    return STORM_HIP_OK;
}
int storm_hip_square_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, uint32_t* h_out,
                                   uint64_t ld) {
    return storm_hip_square_dosage_matrix_device(ctx, a, b, h_out, ld);
}
int storm_hip_square_dosage_nobs_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,
                                        uint64_t n_samples, uint32_t* d_out, uint64_t ld) {
    (void)ctx;
    if (square_refusal(a, b, n_samples, ld)) return STORM_HIP_EINVAL;
    for (uint64_t i = 0; i < a->n_rows; ++i)
        for (uint64_t j = 0; j < b->n_rows; ++j) d_out[i * ld + j] = shared(a, i, b, j, n_samples);
    return STORM_HIP_OK;
}
int storm_hip_square_dosage_nobs(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, uint64_t n_samples,
                                 uint32_t* h_out, uint64_t ld) {
    return storm_hip_square_dosage_nobs_device(ctx, a, b, n_samples, h_out, ld);
}
static int square_corr(const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int measure, int missing, uint64_t n_samples,
                       float* out, uint64_t ld) {
    if (square_refusal(a, b, n_samples, ld) || measure < 0 || measure > 1) return STORM_HIP_EINVAL;
    for (uint64_t i = 0; i < a->n_rows; ++i)
        for (uint64_t j = 0; j < b->n_rows; ++j) out[i * ld + j] = corr(a, i, b, j, measure, missing, n_samples);
    return STORM_HIP_OK;
}
#define SQUARE_CORR_ENTRY(name, missing)                                                                                       \
    int name(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int measure, uint64_t n_samples,  \
             float* out, uint64_t ld) {                                                                                        \
        (void)ctx;                                                                                                             \
        return square_corr(a, b, measure, missing, n_samples, out, ld);                                                       \
    }
SQUARE_CORR_ENTRY(storm_hip_square_dosage_corr_device, 0)
SQUARE_CORR_ENTRY(storm_hip_square_dosage_corr, 0)
SQUARE_CORR_ENTRY(storm_hip_square_dosage_corr_complete_device, 1)
SQUARE_CORR_ENTRY(storm_hip_square_dosage_corr_complete, 1)

/* ---- one matrix, 3 read as "missing": the triangle above the diagonal, a host form's zeros below it ---- */
int storm_hip_dosage_row_missing(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint32_t* h_missing) {
    (void)ctx;
    if ((n_samples + 31) / 32 != m->n_words) return STORM_HIP_EINVAL;
    for (uint64_t i = 0; i < m->n_rows; ++i) {
        h_missing[i] = 0;
        for (uint64_t s = 0; s < n_samples; ++s) h_missing[i] += value_at(m, i, s) == 3u;
    }
    return STORM_HIP_OK;
}
int storm_hip_pairw_dosage_nobs_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint32_t* d_out,
                                       uint64_t ld) {
    (void)ctx;
    if (ld < m->n_rows || (n_samples + 31) / 32 != m->n_words) return STORM_HIP_EINVAL;
    for (uint64_t i = 0; i < m->n_rows; ++i)
        for (uint64_t j = i + 1; j < m->n_rows; ++j) d_out[i * ld + j] = shared(m, i, m, j, n_samples);
    return STORM_HIP_OK;
}
int storm_hip_pairw_dosage_nobs(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint32_t* h_out, uint64_t ld) {
    if (ld < m->n_rows) return STORM_HIP_EINVAL;
    for (uint64_t i = 0; i < m->n_rows; ++i)
        for (uint64_t j = 0; j < m->n_rows; ++j) h_out[i * ld + j] = 0;
    return storm_hip_pairw_dosage_nobs_device(ctx, m, n_samples, h_out, ld);
}
int storm_hip_pairw_dosage_corr_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                                float* d_out, uint64_t ld) {
    (void)ctx;
    if (ld < m->n_rows || (n_samples + 31) / 32 != m->n_words || measure < 0 || measure > 1) return STORM_HIP_EINVAL;
    for (uint64_t i = 0; i < m->n_rows; ++i)
        for (uint64_t j = i + 1; j < m->n_rows; ++j) d_out[i * ld + j] = corr(m, i, m, j, measure, 1, n_samples);
    return STORM_HIP_OK;
}
int storm_hip_pairw_dosage_corr_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                         float* h_out, uint64_t ld) {
    if (ld < m->n_rows) return STORM_HIP_EINVAL;
    for (uint64_t i = 0; i < m->n_rows; ++i)
        for (uint64_t j = 0; j < m->n_rows; ++j) h_out[i * ld + j] = 0.0f;
    return storm_hip_pairw_dosage_corr_complete_device(ctx, m, measure, n_samples, h_out, ld);
}
