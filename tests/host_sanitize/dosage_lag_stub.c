/* dosage_lag_stub.c — TEST ONLY. The lag-layout dosage entry points of the device library for dosage_lag_driver.c, beside
 * device_stub.c (whose matrix is host memory) and dosage_complete_stub.c: every call computes its result from the words that
 * reached it, sample by sample on the CPU, and writes exactly what the real call writes — the pairs (i, i + 1 + d), d < L,
 * i + 1 + d < n, and in the host forms 0 in the corner. Never linked into the product. */
#include <string.h>

#include "stub_dosage.h"

enum { DOT, CORR, NOBS, COMPLETE };

/* one entry as 32 bits: `missing` reads 3 as "no call" */
static uint32_t entry(const storm_hip_matrix_t* m, uint64_t i, uint64_t j, int what, int measure, uint64_t n_samples) {
    double N = 0, P = 0, sx = 0, sy = 0, qx = 0, qy = 0;
    const int missing = what == NOBS || what == COMPLETE;
    const uint64_t S = what == DOT ? (uint64_t)m->n_words * 32 : n_samples;
    for (uint64_t s = 0; s < S; ++s) {
        const unsigned x = value_at(m, i, s), y = value_at(m, j, s);
        if (missing && (x == 3u || y == 3u)) continue;
        N += 1, P += x * y, sx += x, sy += y, qx += x * x, qy += y * y;
    }
    if (what == DOT) return (uint32_t)P;
    if (what == NOBS) return (uint32_t)N;
    const double num = N * P - sx * sy, dx = N * qx - sx * sx, dy = N * qy - sy * sy;
    const float f = dx == 0 || dy == 0 ? NAN : (float)(measure == 0 ? num * num / (dx * dy) : num / sqrt(dx * dy));
    uint32_t bits;
    memcpy(&bits, &f, sizeof(bits));
    return bits;
}

static int lag_call(const storm_hip_matrix_t* m, int what, int measure, uint64_t n_samples, uint64_t max_lag, uint64_t row0,
                    uint64_t n_band_rows, uint32_t* out, uint64_t ld, int host) {
    if (!m || !out || max_lag == 0) return STORM_HIP_EINVAL;
    const uint64_t n = m->n_rows, lag = n ? (max_lag < n - 1 ? max_lag : n - 1) : 0;
    if (ld < lag) return STORM_HIP_EINVAL;
    if (what != DOT && (n_samples + 31) / 32 != m->n_words) return STORM_HIP_EINVAL;
    if ((what == CORR || what == COMPLETE) && (measure < 0 || measure > 1)) return STORM_HIP_EINVAL;
    if (n_band_rows == ~0ull && row0 <= n) n_band_rows = n - row0;
    if (row0 > n || n_band_rows > n - row0) return STORM_HIP_EINVAL;
    if (n < 2) return STORM_HIP_OK;
    for (uint64_t i = row0; i < row0 + n_band_rows; ++i)
        for (uint64_t d = 0; d < lag; ++d) {
            if (i + 1 + d < n) out[(i - row0) * ld + d] = entry(m, i, i + 1 + d, what, measure, n_samples);
            else if (host) out[(i - row0) * ld + d] = 0;
        }
    return STORM_HIP_OK;
}

int storm_hip_pairw_lag_dosage_matrix_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t max_lag, uint64_t row0,
                                             uint64_t n_band_rows, uint32_t* d_out, uint64_t ld) {
    (void)ctx;
    return lag_call(m, DOT, 0, 0, max_lag, row0, n_band_rows, d_out, ld, 0);
}
int storm_hip_pairw_lag_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t max_lag, uint32_t* h_out,
                                      uint64_t ld) {
    (void)ctx;
    return lag_call(m, DOT, 0, 0, max_lag, 0, ~0ull, h_out, ld, 1);
}
int storm_hip_pairw_lag_dosage_corr_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                           uint64_t max_lag, float* d_out, uint64_t ld) {
    (void)ctx;
    return lag_call(m, CORR, measure, n_samples, max_lag, 0, ~0ull, (uint32_t*)d_out, ld, 0);
}
int storm_hip_pairw_lag_dosage_corr(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                    uint64_t max_lag, float* h_out, uint64_t ld) {
    (void)ctx;
    return lag_call(m, CORR, measure, n_samples, max_lag, 0, ~0ull, (uint32_t*)h_out, ld, 1);
}
int storm_hip_pairw_lag_dosage_nobs_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                           uint32_t* d_out, uint64_t ld) {
    (void)ctx;
    return lag_call(m, NOBS, 0, n_samples, max_lag, 0, ~0ull, d_out, ld, 0);
}
int storm_hip_pairw_lag_dosage_nobs(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                    uint32_t* h_out, uint64_t ld) {
    (void)ctx;
    return lag_call(m, NOBS, 0, n_samples, max_lag, 0, ~0ull, h_out, ld, 1);
}
int storm_hip_pairw_lag_dosage_corr_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure,
                                                    uint64_t n_samples, uint64_t max_lag, float* d_out, uint64_t ld) {
    (void)ctx;
    return lag_call(m, COMPLETE, measure, n_samples, max_lag, 0, ~0ull, (uint32_t*)d_out, ld, 0);
}
int storm_hip_pairw_lag_dosage_corr_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                             uint64_t max_lag, float* h_out, uint64_t ld) {
    (void)ctx;
    return lag_call(m, COMPLETE, measure, n_samples, max_lag, 0, ~0ull, (uint32_t*)h_out, ld, 1);
}
