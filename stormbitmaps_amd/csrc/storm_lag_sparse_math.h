// storm_lag_sparse_math.h — the index arithmetic of the sparse pair list taken from a float matrix in the lag layout
// (storm.h: STORM_dosage_lag_corr_sparse; the kernels of storm_hip_lag_sparse.hip): the pitch of a row's forward mask, the
// slot of a set bit in the list and the block plan of the scan of the rows' counts — in a header of its own so that a host
// compiler can build the very same lines (tests/test_lag_sparse_math.py). The edge predicate is pruning's: prune_edge.
#pragma once
#include <stdint.h>

#include "storm_prune_math.h"

namespace storm {

// The forward mask of row i: bit d of the row (bit d % 64 of word d / 64) is the pair (i, i + 1 + d), d < L. 64-bit words,
// one per __ballot of a wave; every word of the pitch is written.
STORM_PRUNE_FN uint64_t sparse_mask_pitch(uint64_t L) { return (L + 63u) / 64u; }

// bits of `word` below bit `lane` (lane < 64): what mbcnt gives the lane on the device
STORM_PRUNE_FN uint32_t sparse_bits_below(uint64_t word, uint32_t lane) {
    const uint64_t below = word & ((1ull << lane) - 1ull);
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t)__popcll(below);
#else
    return (uint32_t)__builtin_popcountll(below);
#endif
}

// The slot of the set bit `lane` of a mask word in the list: the row's first slot, the row's bits in the words before this
// one, the bits of this word below the lane. Ascending in (word, lane), so a row's columns ascend.
STORM_PRUNE_FN uint64_t sparse_slot(uint64_t row_start, uint64_t bits_before, uint64_t word, uint32_t lane) {
    return row_start + bits_before + sparse_bits_below(word, lane);
}

// The scan of the n counts into n + 1 offsets, reduce-then-scan: block b owns the rows [b R, min(n, (b + 1) R)), R =
// kSparseScanRows = kSparseScanThreads threads x kSparseScanPerThread consecutive rows each.
constexpr uint32_t kSparseScanThreads = 256;
constexpr uint32_t kSparseScanPerThread = 4;
constexpr uint32_t kSparseScanRows = kSparseScanThreads * kSparseScanPerThread;   // 1024
STORM_PRUNE_FN uint64_t sparse_scan_blocks(uint64_t n) { return (n + kSparseScanRows - 1u) / kSparseScanRows; }
STORM_PRUNE_FN uint64_t sparse_scan_block_of(uint64_t row) { return row / kSparseScanRows; }
STORM_PRUNE_FN uint64_t sparse_scan_block_rows(uint64_t n, uint64_t b) {   // rows of block b (0 behind the last block)
    const uint64_t r0 = b * kSparseScanRows;
    return r0 >= n ? 0u : (n - r0 < kSparseScanRows ? n - r0 : (uint64_t)kSparseScanRows);
}

// 32-bit words of device scratch of the pass, from an 8-byte aligned base: the masks (64-bit), the blocks' sums (64-bit),
// then the counts and, with windows, lo and hi
STORM_PRUNE_FN uint64_t sparse_scratch_words(uint64_t n, uint64_t L, bool windows) {
    return 2u * (n * sparse_mask_pitch(L) + sparse_scan_blocks(n)) + n + (windows ? 2u * n : 0u);
}

}  // namespace storm
