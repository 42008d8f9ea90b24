// storm_dosage_math.h — the arithmetic of one entry of dosage_finish_kernel (storm_hip_dosage.hip): the Pearson
// correlation of two rows of 2-bit values (genotype dosages), in a header of its own so that a host compiler can build
// the very same lines: tests/test_dosage_math.py checks them against exactly rounded rationals without a device.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define STORM_DOSAGE_FN __host__ __device__ __forceinline__
#else
#define STORM_DOSAGE_FN static inline
#endif

namespace storm {

constexpr uint32_t kDosageNaN = 0x7FC00000u;   // "undefined": the one quiet-NaN pattern (storm_hip.h)

// One entry: P = sum v_i v_j, s = sum v, q = sum v^2 of either row, S = samples per row (1 .. 2^24, values 0 .. 3).
//   num = S P - s_i s_j and d = S q - s^2 are formed exactly in 64-bit integers (every term is below 9 x 2^48; the sign
//   of num is kept aside; d >= 0 by Cauchy-Schwarz and 0 exactly for a constant row),
//   measure 0 (r^2): num^2 / (d_i d_j),   measure 1 (r): +-num / sqrt(d_i d_j),
// in double — the integers convert exactly (below 2^53), three correctly rounded operations carry 3.4e-16 of relative
// error against a float's half-ulp of 6e-8 — and rounded once to float: at most one float away from the correctly
// rounded rational (r: from the correctly rounded real). NaN when either row is constant.
STORM_DOSAGE_FN uint32_t dosage_corr_bits(uint32_t P, uint32_t s_i, uint32_t q_i, uint32_t s_j, uint32_t q_j, int measure,
                                          uint64_t S) {
    const uint64_t d_i = S * q_i - (uint64_t)s_i * s_i, d_j = S * q_j - (uint64_t)s_j * s_j;
    if (d_i == 0 || d_j == 0) return kDosageNaN;
    const uint64_t x = S * P, y = (uint64_t)s_i * s_j;
    const bool negative = x < y;
    const double num = (double)(negative ? y - x : x - y);
    const double den = (double)d_i * (double)d_j;
    double v;
    if (measure == 0 /* STORM_HIP_DOSAGE_R2 */) {
        v = (num * num) / den;
    } else {
        v = num / sqrt(den);
        if (negative) v = -v;
    }
    const float f = (float)v;
    uint32_t bits;
    memcpy(&bits, &f, sizeof(bits));
    return bits;
}

}  // namespace storm
