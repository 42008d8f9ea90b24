/* dosage_ldscore_annot_stub.c — TEST ONLY. The stratified LD-score entry points of the device library for
 * dosage_ldscore_annot_driver.c, beside device_stub.c (whose matrix is host memory), dosage_complete_stub.c and
 * dosage_ldscore_stub.c (storm_hip_ctx_synchronize): every call computes its result from the words that reached it, sample
 * by sample on the CPU, in host memory, and writes exactly what the real call writes — columns [0, n_annot) of rows [0, n)
 * of score and, where given, elements [0, n) of n_pairs. Never linked into the product. */
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

static int annot_call(const storm_hip_matrix_t* m, int stat, uint64_t n_samples, uint64_t max_lag, int missing, const uint32_t* lo,
                      const uint32_t* hi, const float* annot, uint64_t annot_ld, uint64_t n_annot, float* score, uint64_t score_ld,
                      uint32_t* n_pairs) {
    if (!m || !score || max_lag == 0) return STORM_HIP_EINVAL;
    if (stat != STORM_HIP_LDSCORE_R2 && stat != STORM_HIP_LDSCORE_R2_ADJ) return STORM_HIP_EINVAL;
    if ((n_samples + 31) / 32 != m->n_words) return STORM_HIP_EINVAL;
    if (!annot || n_annot < 1 || n_annot > 1024 || annot_ld < n_annot || score_ld < n_annot || !lo != !hi) return STORM_HIP_EINVAL;
    const uint64_t n = m->n_rows;
    if (n < 2) return STORM_HIP_OK;
    const uint64_t lag = max_lag < n - 1 ? max_lag : n - 1;
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t pairs = 0;
        for (uint64_t c = 0; c < n_annot; ++c) {
            double sum = 0;
            pairs = 0;
            for (uint64_t j = i > lag ? i - lag : 0; j < n && j <= i + lag; ++j) {
                if (j == i || (lo && (j < lo[i] || j > hi[i]))) continue;
                uint64_t n_obs = 0;
                const float rho = j < i ? pair_r2(m, j, i, missing, n_samples, &n_obs) : pair_r2(m, i, j, missing, n_samples, &n_obs);
                if (isnan(rho) || (stat == STORM_HIP_LDSCORE_R2_ADJ && n_obs < 3)) continue;
                const double t = stat == STORM_HIP_LDSCORE_R2_ADJ ? (double)rho - (1.0 - (double)rho) / (double)(n_obs - 2) : (double)rho;
                sum = fma(t, (double)annot[j * annot_ld + c], sum);
                ++pairs;
            }
            score[i * score_ld + c] = (float)sum;
        }
        if (n_pairs) n_pairs[i] = pairs;
    }
    return STORM_HIP_OK;
}

int storm_hip_lag_dosage_ldscore_annot_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                              uint64_t max_lag, const uint32_t* h_lo, const uint32_t* h_hi, const float* d_annot,
                                              uint64_t annot_ld, uint64_t n_annot, float* d_score, uint64_t score_ld,
                                              uint32_t* d_n_pairs) {
    (void)ctx;
    return annot_call(m, stat, n_samples, max_lag, 0, h_lo, h_hi, d_annot, annot_ld, n_annot, d_score, score_ld, d_n_pairs);
}
int storm_hip_lag_dosage_ldscore_annot(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                       uint64_t max_lag, const uint32_t* h_lo, const uint32_t* h_hi, const float* h_annot,
                                       uint64_t annot_ld, uint64_t n_annot, float* h_score, uint64_t score_ld, uint32_t* h_n_pairs) {
    (void)ctx;
    return annot_call(m, stat, n_samples, max_lag, 0, h_lo, h_hi, h_annot, annot_ld, n_annot, h_score, score_ld, h_n_pairs);
}
int storm_hip_lag_dosage_ldscore_annot_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat,
                                                       uint64_t n_samples, uint64_t max_lag, const uint32_t* h_lo,
                                                       const uint32_t* h_hi, const float* d_annot, uint64_t annot_ld,
                                                       uint64_t n_annot, float* d_score, uint64_t score_ld, uint32_t* d_n_pairs) {
    (void)ctx;
    return annot_call(m, stat, n_samples, max_lag, 1, h_lo, h_hi, d_annot, annot_ld, n_annot, d_score, score_ld, d_n_pairs);
}
int storm_hip_lag_dosage_ldscore_annot_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                                uint64_t max_lag, const uint32_t* h_lo, const uint32_t* h_hi, const float* h_annot,
                                                uint64_t annot_ld, uint64_t n_annot, float* h_score, uint64_t score_ld,
                                                uint32_t* h_n_pairs) {
    (void)ctx;
    return annot_call(m, stat, n_samples, max_lag, 1, h_lo, h_hi, h_annot, annot_ld, n_annot, h_score, score_ld, h_n_pairs);
}
