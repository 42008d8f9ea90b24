// storm_topk_math.h — the order topk_rows_kernel (storm_hip_topk.hip) selects by, in a header of its own so that a host
// compiler can build the very same lines: tests/test_topk_math.py checks them against numpy's sort without a device.
//
// An entry (value bits, column j) becomes one 64-bit key: the value mapped monotonically to an unsigned integer in the
// high word, 0xFFFFFFFF - j in the low word. The largest key is the best neighbour: value descending, then column
// ascending, and no two keys of a row are equal (their columns differ). A candidate's key is never 0 (j <= 2^32 - 2),
// so 0 stands for "no entry".
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define STORM_TOPK_FN __host__ __device__ __forceinline__
#else
#define STORM_TOPK_FN static inline
#endif

namespace storm {

constexpr uint32_t kTopkNaN = 0x7FC00000u;      // "undefined" (storm_similarity_math.h: kSimNaN): not a candidate
constexpr uint32_t kTopkNoIndex = 0xFFFFFFFFu;  // idx of a padding entry

// false exactly for the one NaN pattern the similarity measures write; the key of a non-candidate is never formed
STORM_TOPK_FN bool topk_is_candidate(uint32_t value_bits) { return value_bits != kTopkNaN; }

// float bits -> unsigned, so that float order is unsigned order (the sign-flip map); -0 like +0
STORM_TOPK_FN uint32_t topk_float_to_ordered(uint32_t bits) {
    if (bits == 0x80000000u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
STORM_TOPK_FN uint32_t topk_ordered_to_float(uint32_t ordered) {
    return (ordered & 0x80000000u) ? (ordered & 0x7FFFFFFFu) : ~ordered;
}

// is_count: the value is an AND count and is used as it is; else float bits
STORM_TOPK_FN uint64_t topk_key(uint32_t value_bits, uint32_t j, bool is_count) {
    const uint32_t hi = is_count ? value_bits : topk_float_to_ordered(value_bits);
    return ((uint64_t)hi << 32) | (uint64_t)(0xFFFFFFFFu - j);
}
STORM_TOPK_FN uint32_t topk_key_index(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }
STORM_TOPK_FN uint32_t topk_key_value(uint64_t key, bool is_count) {
    const uint32_t hi = (uint32_t)(key >> 32);
    return is_count ? hi : topk_ordered_to_float(hi);
}

}  // namespace storm
