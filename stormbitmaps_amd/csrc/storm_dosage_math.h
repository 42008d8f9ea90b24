// storm_dosage_math.h — the arithmetic of one entry of dosage_finish_kernel and dosage_complete_finish_kernel
// (storm_hip_dosage.hip): the Pearson correlation of two rows of 2-bit values (genotype dosages), over all samples or
// over the samples both rows have, and the word logic of dosage_split_missing_kernel — in a header of its own so that a
// host compiler can build the very same lines: tests/test_dosage_math.py and tests/test_dosage_complete_math.py check
// them against exactly rounded rationals and a per-sample loop without a device.
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

// ---- rows with missing genotypes (code 3 = missing): pairwise-complete statistics ----
constexpr uint64_t kDosageLowBits = 0x5555555555555555ull;   // the low bit of each of a word's 32 values

// The low bits of the values of word `word` of a row that are samples: all 32 below the last word, the first
// n_samples % 32 (0: all) in the last one, none in the pad words behind it.
STORM_DOSAGE_FN uint64_t dosage_valid_mask(uint64_t word, uint32_t n_words, uint64_t n_samples) {
    if (word + 1u < n_words) return kDosageLowBits;
    if (word >= n_words) return 0ull;
    const uint32_t tail = (uint32_t)(n_samples % 32u);
    return tail ? kDosageLowBits & ((1ull << (2u * tail)) - 1ull) : kDosageLowBits;
}

// One word of a row split into three words of 2-bit values: g = the value with 3 -> 0, h = 1 where the value is 2
// (so that g^2 = g + 2 h), m = 1 where a sample is present (`valid`: dosage_valid_mask of the word).
STORM_DOSAGE_FN void dosage_split_word(uint64_t w, uint64_t valid, uint64_t* g, uint64_t* h, uint64_t* m) {
    const uint64_t lo = w & kDosageLowBits, hi = (w >> 1) & kDosageLowBits;
    const uint64_t both = lo & hi;
    *g = w & ~(3ull * both);
    *h = hi & ~lo;
    *m = ~both & kDosageLowBits & valid;
}

// Word w of row r of the INTERLEAVED split of a matrix X (n_rows rows of stride_words words, n_words of them data): row
// 3 i is G_i, row 3 i + 1 is H_i, row 3 i + 2 is M_i — one matrix of 3 n_rows rows whose lag layout at lag 3 L + 2 holds
// every product of G, H, M of two rows within L of each other (dosage_split_interleaved_kernel). Rows behind 3 n_rows
// and the words behind n_words are zero.
STORM_DOSAGE_FN uint64_t dosage_interleaved_word(const uint64_t* X, uint64_t stride_words, uint64_t n_rows, uint32_t n_words,
                                                 uint64_t n_samples, uint64_t r, uint64_t w) {
    const uint64_t row = r / 3u;
    if (row >= n_rows || w >= n_words) return 0ull;
    uint64_t g, h, m;
    dosage_split_word(X[row * stride_words + w], dosage_valid_mask(w, n_words, n_samples), &g, &h, &m);
    const uint32_t which = (uint32_t)(r % 3u);
    return which == 0u ? g : which == 1u ? h : m;
}

// One entry over the samples BOTH rows have: N = their number, P = sum g_i g_j, sx = sum g_i m_j, sy = sum m_i g_j,
// qx = sum g_i^2 m_j, qy = sum m_i g_j^2 (g: the value, 0 where missing; m: 1 where present; values 0 .. 2, at most 2^24
// samples: every term below 2^51).
//   num = N P - sx sy, dx = N qx - sx^2, dy = N qy - sy^2 exactly in 64-bit integers (dx, dy >= 0 by Cauchy-Schwarz over
//   the shared samples), then dosage_corr_bits' scheme line for line: on rows without a missing sample (N = S,
//   sx = s_i, ...) the result is the same bits. NaN when dx or dy is 0: no or one shared sample, or a row that is
//   constant on the shared samples.
STORM_DOSAGE_FN uint32_t dosage_corr_complete_bits(uint32_t P, uint32_t N, uint32_t sx, uint32_t sy, uint32_t qx, uint32_t qy,
                                                   int measure) {
    const uint64_t d_i = (uint64_t)N * qx - (uint64_t)sx * sx, d_j = (uint64_t)N * qy - (uint64_t)sy * sy;
    if (d_i == 0 || d_j == 0) return kDosageNaN;
    const uint64_t x = (uint64_t)N * P, y = (uint64_t)sx * sy;
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

// Where the six sums of the pair (i, i + 1 + d) lie in the lag layout (lag 3 L + 2) of the interleaved split, and what
// entry (i, d) of the caller's matrix is made of (g_row, h_row, m_row: rows 3 i, 3 i + 1, 3 i + 2 of that layout):
//   row 3 i     : P = G_i G_j at 3 d + 2, Sx = G_i M_j at 3 d + 4
//   row 3 i + 1 : H_i M_j at 3 d + 3                      (Qx = Sx + 2 H_i M_j)
//   row 3 i + 2 : Sy = M_i G_j at 3 d, M_i H_j at 3 d + 1 (Qy = Sy + 2 M_i H_j), N = M_i M_j at 3 d + 2
// (rows 3 i + a and 3 j + b are 3 (d + 1) + b - a apart: column 3 d + 2 + b - a, at most 3 L + 1.)
STORM_DOSAGE_FN uint32_t dosage_interleaved_entry_bits(const uint32_t* g_row, const uint32_t* h_row, const uint32_t* m_row,
                                                       uint32_t d, int measure) {
    const uint32_t c = 3u * d;
    const uint32_t sx = g_row[c + 4u], sy = m_row[c];
    return dosage_corr_complete_bits(g_row[c + 2u], m_row[c + 2u], sx, sy, sx + 2u * h_row[c + 3u], sy + 2u * m_row[c + 1u],
                                     measure);
}

}  // namespace storm
