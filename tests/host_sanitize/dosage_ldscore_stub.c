/* dosage_ldscore_stub.c — TEST ONLY. The LD-score entry points of the device library for dosage_ldscore_driver.c, beside
 * device_stub.c (whose matrix is host memory) and dosage_complete_stub.c: every call computes its result from the words that
 * reached it, sample by sample on the CPU, in host memory, and writes exactly what the real call writes — elements [0, n)
 * of score and, where given, of n_pairs. Never linked into the product. */
#include <math.h>
#include <stdint.h>

#include "storm_hip.h"

struct storm_hip_matrix_s { uint64_t n_rows; uint32_t n_words; uint64_t* rows; }; /* device_stub.c's */

static unsigned value_at(const storm_hip_matrix_t* m, uint64_t row, uint64_t s) {
    return (unsigned)(m->rows[row * m->n_words + s / 32] >> (2 * (s % 32))) & 3u;
}

/* the pair's r^2 as the corr call's float and the samples behind it; `missing` reads 3 as "no call" */
static float pair_r2(const storm_hip_matrix_t* m, uint64_t i, uint64_t j, int missing, uint64_t n_samples, uint64_t* n_obs) {
    double N = 0, P = 0, sx = 0, sy = 0, qx = 0, qy = 0;
    for (uint64_t s = 0; s < n_samples; ++s) {
        const unsigned x = value_at(m, i, s), y = value_at(m, j, s);
        if (missing && (x == 3u || y == 3u)) continue;
        N += 1, P += x * y, sx += x, sy += y, qx += x * x, qy += y * y;
    }
    *n_obs = (uint64_t)N;
    const double num = N * P - sx * sy, dx = N * qx - sx * sx, dy = N * qy - sy * sy;
    return dx == 0 || dy == 0 ? NAN : (float)(num * num / (dx * dy));
}

int storm_hip_ctx_synchronize(storm_hip_ctx_t* ctx) { return ctx ? STORM_HIP_OK : STORM_HIP_EINVAL; }

static int ldscore_call(const storm_hip_matrix_t* m, int stat, uint64_t n_samples, uint64_t max_lag, int missing, float* score,
                        uint32_t* n_pairs) {
    if (!m || !score || max_lag == 0) return STORM_HIP_EINVAL;
    if (stat != STORM_HIP_LDSCORE_R2 && stat != STORM_HIP_LDSCORE_R2_ADJ) return STORM_HIP_EINVAL;
    if ((n_samples + 31) / 32 != m->n_words) return STORM_HIP_EINVAL;
    const uint64_t n = m->n_rows;
    if (n < 2) return STORM_HIP_OK;
    const uint64_t lag = max_lag < n - 1 ? max_lag : n - 1;
    for (uint64_t i = 0; i < n; ++i) {
        double sum = 0;
        uint32_t pairs = 0;
        for (uint64_t j = i > lag ? i - lag : 0; j < n && j <= i + lag; ++j) {
            if (j == i) continue;
            uint64_t n_obs = 0;
            const float rho = j < i ? pair_r2(m, j, i, missing, n_samples, &n_obs) : pair_r2(m, i, j, missing, n_samples, &n_obs);
            if (isnan(rho) || (stat == STORM_HIP_LDSCORE_R2_ADJ && n_obs < 3)) continue;
            sum += stat == STORM_HIP_LDSCORE_R2_ADJ ? (double)rho - (1.0 - (double)rho) / (double)(n_obs - 2) : (double)rho;
            ++pairs;
        }
        score[i] = (float)sum;
        if (n_pairs) n_pairs[i] = pairs;
    }
    return STORM_HIP_OK;
}

int storm_hip_lag_dosage_ldscore_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                        uint64_t max_lag, float* d_score, uint32_t* d_n_pairs) {
    (void)ctx;
    return ldscore_call(m, stat, n_samples, max_lag, 0, d_score, d_n_pairs);
}
int storm_hip_lag_dosage_ldscore(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples, uint64_t max_lag,
                                 float* h_score, uint32_t* h_n_pairs) {
    (void)ctx;
    return ldscore_call(m, stat, n_samples, max_lag, 0, h_score, h_n_pairs);
}
int storm_hip_lag_dosage_ldscore_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                                 uint64_t max_lag, float* d_score, uint32_t* d_n_pairs) {
    (void)ctx;
    return ldscore_call(m, stat, n_samples, max_lag, 1, d_score, d_n_pairs);
}
int storm_hip_lag_dosage_ldscore_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                          uint64_t max_lag, float* h_score, uint32_t* h_n_pairs) {
    (void)ctx;
    return ldscore_call(m, stat, n_samples, max_lag, 1, h_score, h_n_pairs);
}
