/* dosage_lag_sparse_stub.c — TEST ONLY. The entry points of the device library that list the pairs of the band of r^2 above a
 * threshold (storm_hip.h: storm_hip_lag_dosage_corr_sparse[_complete][_device]), for dosage_lag_sparse_driver.c, beside
 * device_stub.c (whose matrix is host memory) and dosage_band_stub.c (the wait): every call computes its list from the words
 * that reached it, sample by sample on the CPU, in host memory, and writes exactly what the real call writes — elements
 * [0, n] of row_start, the total, and of col / val the host forms exactly `total` entries (none where the capacity is below
 * it: STORM_HIP_EINVAL), the _device forms the first `capacity` ones. Never linked into the product. */
#include "stub_dosage.h"

static int sparse_call(const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag, float min_r2, int missing, const uint32_t* lo,
                       const uint32_t* hi, uint64_t* row_start, uint32_t* col, float* val, uint64_t capacity, uint64_t* n_pairs,
                       int host) {
    if (!m || !row_start || max_lag == 0 || (n_samples + 31) / 32 != m->n_words) return STORM_HIP_EINVAL;
    if (!lo != !hi || !col != !val || (!col && capacity) || isnan(min_r2)) return STORM_HIP_EINVAL;
    const uint64_t n = m->n_rows;
    const uint64_t lag = n ? (max_lag < n - 1 ? max_lag : n - 1) : 0;
    for (int pass = 0; pass < 2; ++pass) {   /* the offsets and the total, then the entries */
        uint64_t total = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (!pass) row_start[i] = total;
            for (uint64_t j = i + 1; j < n && j <= i + lag; ++j) {
                uint64_t n_obs = 0;
                if (lo && !(j <= hi[i] && i >= lo[j])) continue;
                const float rho = pair_r2(m, i, j, missing, n_samples, &n_obs);
                if (!(rho > min_r2)) continue;
                if (pass && col && total < capacity) col[total] = (uint32_t)j, val[total] = rho;
                ++total;
            }
        }
        if (!pass) {
            row_start[n] = total;
            if (n_pairs) *n_pairs = total;
            if (host && col && total > capacity) return STORM_HIP_EINVAL;
        }
    }
    return STORM_HIP_OK;
}

#define SPARSE_DEVICE_ENTRY(name, missing)                                                                                    \
    int name(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag, float min_r2,            \
             const uint32_t* h_lo, const uint32_t* h_hi, uint64_t* row_start, uint32_t* col, float* val, uint64_t capacity) { \
        (void)ctx;                                                                                                            \
        return sparse_call(m, n_samples, max_lag, min_r2, missing, h_lo, h_hi, row_start, col, val, capacity, NULL, 0);       \
    }
#define SPARSE_HOST_ENTRY(name, missing)                                                                                     \
    int name(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag, float min_r2,           \
             const uint32_t* h_lo, const uint32_t* h_hi, uint64_t* row_start, uint32_t* col, float* val, uint64_t capacity,  \
             uint64_t* n_pairs) {                                                                                            \
        (void)ctx;                                                                                                           \
        return sparse_call(m, n_samples, max_lag, min_r2, missing, h_lo, h_hi, row_start, col, val, capacity, n_pairs, 1);   \
    }
SPARSE_DEVICE_ENTRY(storm_hip_lag_dosage_corr_sparse_device, 0)
SPARSE_HOST_ENTRY(storm_hip_lag_dosage_corr_sparse, 0)
SPARSE_DEVICE_ENTRY(storm_hip_lag_dosage_corr_sparse_complete_device, 1)
SPARSE_HOST_ENTRY(storm_hip_lag_dosage_corr_sparse_complete, 1)
