/* dosage_prune_stub.c — TEST ONLY. The prune / clump entry points of the device library for dosage_prune_driver.c, beside
 * device_stub.c (whose matrix is host memory), dosage_complete_stub.c and dosage_ldscore_stub.c (storm_hip_ctx_synchronize):
 * the "device" is host memory running the plain greedy over the pairs' r^2, computed sample by sample on the CPU from the
 * words that reached it, and it writes exactly what the real call writes — elements [0, n) of keep and, where given, of
 * owner. Never linked into the product. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "storm_hip.h"

struct storm_hip_matrix_s { uint64_t n_rows; uint32_t n_words; uint64_t* rows; }; /* device_stub.c's */

static unsigned value_at(const storm_hip_matrix_t* m, uint64_t row, uint64_t s) {
    return (unsigned)(m->rows[row * m->n_words + s / 32] >> (2 * (s % 32))) & 3u;
}

/* the pair's r^2 as the corr call's float; `missing` reads 3 as "no call" */
static float pair_r2(const storm_hip_matrix_t* m, uint64_t i, uint64_t j, int missing, uint64_t n_samples) {
    double N = 0, P = 0, sx = 0, sy = 0, qx = 0, qy = 0;
    for (uint64_t s = 0; s < n_samples; ++s) {
        const unsigned x = value_at(m, i, s), y = value_at(m, j, s);
        if (missing && (x == 3u || y == 3u)) continue;
        N += 1, P += x * y, sx += x, sy += y, qx += x * x, qy += y * y;
    }
    const double num = N * P - sx * sy, dx = N * qx - sx * sx, dy = N * qy - sy * sy;
    return dx == 0 || dy == 0 ? NAN : (float)(num * num / (dx * dy));
}

static int prune_call(const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag, float min_r2, int missing,
                      const uint32_t* lo, const uint32_t* hi, const uint32_t* order, uint8_t* keep, uint32_t* owner) {
    if (!m || !keep || max_lag == 0) return STORM_HIP_EINVAL;
    if ((n_samples + 31) / 32 != m->n_words) return STORM_HIP_EINVAL;
    if (!lo != !hi || m->n_rows > (1u << 20) || isnan(min_r2)) return STORM_HIP_EINVAL;
    const uint64_t n = m->n_rows;
    if (n == 0) return STORM_HIP_OK;
    const uint64_t lag = max_lag < n - 1 ? max_lag : n - 1;
    uint8_t* marked = (uint8_t*)calloc(n, 1);
    if (!marked) return STORM_HIP_ENOMEM;
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t v = order ? order[k] : k;
        if (marked[v]) {
            keep[v] = 0;
            continue;
        }
        keep[v] = 1;
        if (owner) owner[v] = (uint32_t)v;
        for (uint64_t j = v > lag ? v - lag : 0; j < n && j <= v + lag; ++j) {
            if (j == v || marked[j]) continue;
            const uint64_t a = j < v ? j : v, b = j < v ? v : j;
            if (lo && !(b <= hi[a] && a >= lo[b])) continue;
            if (pair_r2(m, a, b, missing, n_samples) > min_r2) {   /* (a row kept earlier is never adjacent: v would be marked) */
                marked[j] = 1;
                if (owner) owner[j] = (uint32_t)v;
            }
        }
    }
    free(marked);
    return STORM_HIP_OK;
}

int storm_hip_lag_dosage_prune_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                      float min_r2, const uint32_t* h_lo, const uint32_t* h_hi, const uint32_t* h_order,
                                      uint8_t* d_keep, uint32_t* d_owner) {
    (void)ctx;
    return prune_call(m, n_samples, max_lag, min_r2, 0, h_lo, h_hi, h_order, d_keep, d_owner);
}
int storm_hip_lag_dosage_prune(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag, float min_r2,
                               const uint32_t* h_lo, const uint32_t* h_hi, const uint32_t* h_order, uint8_t* h_keep,
                               uint32_t* h_owner) {
    (void)ctx;
    return prune_call(m, n_samples, max_lag, min_r2, 0, h_lo, h_hi, h_order, h_keep, h_owner);
}
int storm_hip_lag_dosage_prune_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples,
                                               uint64_t max_lag, float min_r2, const uint32_t* h_lo, const uint32_t* h_hi,
                                               const uint32_t* h_order, uint8_t* d_keep, uint32_t* d_owner) {
    (void)ctx;
    return prune_call(m, n_samples, max_lag, min_r2, 1, h_lo, h_hi, h_order, d_keep, d_owner);
}
int storm_hip_lag_dosage_prune_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                        float min_r2, const uint32_t* h_lo, const uint32_t* h_hi, const uint32_t* h_order,
                                        uint8_t* h_keep, uint32_t* h_owner) {
    (void)ctx;
    return prune_call(m, n_samples, max_lag, min_r2, 1, h_lo, h_hi, h_order, h_keep, h_owner);
}
