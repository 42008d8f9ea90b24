// storm_prune_math.h — the edge predicate of LD pruning and clumping (storm.h: STORM_dosage_lag_prune;
// lag_band_threshold_kernel of storm_hip_prune.hip): when an entry of a float matrix in the lag layout joins the two rows of
// its pair — in a header of its own so that a host compiler can build the very same line (tests/test_prune_math.py).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define STORM_PRUNE_FN __host__ __device__ __forceinline__
#else
#define STORM_PRUNE_FN static inline
#endif

namespace storm {

// One pair: rho = the float of the matrix, min_r2 = the threshold (never NaN: the calls refuse it). An edge exactly when
// rho > min_r2 as floats: a NaN rho fails the comparison (never an edge), a pair exactly at the threshold is not an edge,
// and -0.0f equals +0.0f on either side.
STORM_PRUNE_FN bool prune_edge(float rho, float min_r2) { return rho > min_r2; }

// The mask of row v covers rows v - L .. v + L, aligned to ABSOLUTE row numbers: word k holds rows base + 32 k .. + 31,
// bit b of it row base + 32 k + b.
STORM_PRUNE_FN uint64_t prune_mask_base(uint64_t v, uint64_t L) { return (v > L ? v - L : 0u) / 32u * 32u; }
STORM_PRUNE_FN uint64_t prune_mask_pitch(uint64_t L) { return 2u * ((L + 31u) / 32u) + 2u; }

}  // namespace storm
