// storm_ldscore_math.h — the arithmetic of one pair of lag_band_sums_kernel (storm_hip_ldscore.hip), and where the kernel
// finds the pair's N: what an entry of a float matrix in the lag layout adds to the sum of its two rows (storm.h:
// STORM_dosage_lag_ldscore) — in a header of its own so that a host compiler can build the very same lines:
// tests/test_ldscore_math.py restates the whole reduction on them in plain C and compares it with numpy without a device.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define STORM_LDSCORE_FN __host__ __device__ __forceinline__
#else
#define STORM_LDSCORE_FN static inline
#endif

namespace storm {

constexpr int kLdscoreR2 = 0;      // STORM_LDSCORE_R2: the entry itself
constexpr int kLdscoreR2Adj = 1;   // STORM_LDSCORE_R2_ADJ: r^2 - (1 - r^2) / (N - 2)

// One pair: rho = the float of the matrix, N = the samples behind it (read for kLdscoreR2Adj alone). false: the pair is
// not summed — rho is NaN, or the correction has no N - 2 to divide by (N < 3). Otherwise *term is the pair's term in
// double: rho widened (exact), and for the adjusted statistic three correctly rounded operations on it (no product: there
// is nothing a compiler could contract).
STORM_LDSCORE_FN bool ldscore_term(float rho, int stat, uint64_t N, double* term) {
    if (rho != rho) return false;
    const double r = (double)rho;
    if (stat == kLdscoreR2) {
        *term = r;
        return true;
    }
    if (N < 3u) return false;
    *term = r - (1.0 - r) / (double)(N - 2u);
    return true;
}

// The samples behind entry (i, d) where they come from a strided view of a uint32 matrix: N(i, d) at
// nobs[i * row_pitch + d * col_stride] (the pairwise-complete call: row 3 i + 2, column 3 d + 2 of its sums).
STORM_LDSCORE_FN uint64_t ldscore_nobs_at(const uint32_t* nobs, uint64_t row_pitch, uint64_t col_stride, uint64_t i, uint64_t d) {
    return (uint64_t)nobs[i * row_pitch + d * col_stride];
}

// One pair in one column of the stratified scores (lag_band_annot_sums_kernel, storm_hip_ldscore_annot.hip): the pair's
// term times the annotation of the OTHER row, added to the column's sum by one explicit fused multiply-add — one rounding,
// whatever -ffp-contract says, on the device and in the host restatement of tests/test_ldscore_annot_math.py alike. A pair
// that is not summed enters as term +0.0 and leaves the sum's bits as they are for every finite a.
STORM_LDSCORE_FN double ldscore_annot_add(double sum, double term, float a) { return __builtin_fma(term, (double)a, sum); }

}  // namespace storm
