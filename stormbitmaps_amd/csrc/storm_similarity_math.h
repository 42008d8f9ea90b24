// storm_similarity_math.h — the arithmetic of one entry of similarity_finish_kernel (storm_hip_similarity.hip), in a
// header of its own so that a host compiler can build the very same lines: tests/test_similarity_math.py checks them
// against exactly rounded rationals without a device.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#ifdef __HIPCC__
#define STORM_SIM_FN __host__ __device__ __forceinline__
#else
#define STORM_SIM_FN static inline
#endif

namespace storm {

constexpr uint32_t kSimNaN = 0x7FC00000u;   // "undefined": the one quiet-NaN pattern (storm_hip.h)

// One entry: c = |A_i & B_j|, a = |A_i|, b = |B_j|, M = bits of the universe. M c - a b is formed exactly in 64-bit
// integers (M <= 2^32 and a, b, c < 2^32: either product fits; the sign is kept aside), the rest in double, rounded
// once to float: a handful of f64 operations carry 1e-15 of relative error against a float's half-ulp of 6e-8, so the
// result is at most one float away from the correctly rounded rational.
STORM_SIM_FN uint32_t similarity_bits(uint32_t c, uint32_t a, uint32_t b, int measure, uint64_t M) {
    double v;
    if (measure == 0 /* STORM_HIP_SIM_JACCARD */) {
        const uint64_t u = (uint64_t)a + b - c;
        if (u == 0) return kSimNaN;
        v = (double)c / (double)u;
    } else if (measure == 1 /* STORM_HIP_SIM_COSINE */) {
        const uint64_t p = (uint64_t)a * b;
        if (p == 0) return kSimNaN;
        v = (double)c / sqrt((double)p);
    } else {
        const uint64_t x = M * c, y = (uint64_t)a * b;
        const bool negative = x < y;
        const double d = (double)(negative ? y - x : x - y);
        if (measure == 2 /* STORM_HIP_SIM_LD_D */) {
            const double m = (double)M;
            v = d / (m * m);
            if (negative) v = -v;
        } else {
            if (a == 0 || a >= M || b == 0 || b >= M) return kSimNaN;
            v = (d * d) / ((double)(a * (M - a)) * (double)(b * (M - b)));
        }
    }
    const float f = (float)v;
    uint32_t bits;
    memcpy(&bits, &f, sizeof(bits));
    return bits;
}

}  // namespace storm
