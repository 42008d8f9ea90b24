// storm_hip_dosage.hip — rows of 2-bit VALUES (genotype dosages 0 / 1 / 2; 3 is an ordinary value) instead of bits: value s
// of a row in bits 2 (s % 32), 2 (s % 32) + 1 of word s / 32 of an ordinary storm_hip_matrix_t. The dot products of all row
// pairs come from K2h in its dosage form (tile128_kernel<false, 2>, storm_hip_mfma.hip: launch_pairw_dosage_matrix); this
// file holds what stands around it — the rows' sums and sums of squares, and DosageStat, the policy under which the shared
// in-place uint32 -> float pass (finish_tiles_kernel.inc; the triangle: finish_tiles_kernel<DosageStat, true>) turns a dot
// product into PLINK's --r / --r2, the (squared) Pearson correlation of two dosage vectors — and the C-ABI of the form. Plain vector code; the formulas are storm_dosage_math.h.
// Missing genotypes (the *_complete, *_nobs and *_row_missing calls only: code 3 = missing there, an ordinary value in
// every other call): dosage_split_missing_kernel splits the rows into three matrices of 2-bit rows — G (3 -> 0), H (1 where
// the value is 2) and M (1 where present) — K2h multiplies the triangles of G and of M and the rectangle [G ; H] x M, and
// dosage_complete_finish_kernel turns the five sums of a pair into r / r^2 over the samples both rows have (DESIGN.md §4,
// "K2h, dosage form with missing genotypes").
// The rectangle of two matrices (the *_square_dosage_* calls): K2h over n_a x n_b; for r / r^2 both matrices' row sums and
// finish_tiles_kernel<DosageStat, false>, or both matrices' splits, six products in three launches and
// dosage_square_complete_finish_kernel ("K2h, dosage form: the rectangle of two containers").
// The lag layout (the *_lag_dosage_* calls: the pairs within max_lag rows of each other, an n x L matrix): K2h in its lag and
// dosage form (tile128_kernel<true, 2>: launch_pairw_lag_dosage_matrix), finish_lag_tiles_kernel<DosageStat> over it, and for missing
// genotypes dosage_split_interleaved_kernel — G, H and M as ONE matrix of 3 n rows — one launch at lag 3 L + 2 into a scratch
// matrix of 3 n x (3 L + 2) words and dosage_complete_finish_lag_kernel from there into the caller's matrix: O(n L)
// throughout ("K2h, dosage form in the lag layout").
#include "storm_hip_internal.h"
#include "storm_dosage_math.h"

namespace storm {

constexpr uint64_t kDosageMaxSamples = 1ull << 24;

// One wave per row: lo = the values' low bits, hi = their high bits; sum v = pc(lo) + 2 pc(hi),
// sum v^2 = pc(lo) + 4 pc(hi) + 4 pc(lo & hi). Four rows per workgroup.
__global__ __launch_bounds__(kThreads) void dosage_row_sums_kernel(const uint64_t* __restrict__ X, uint64_t stride_words,
                                                                   uint64_t n_rows, uint32_t n_words,
                                                                   uint32_t* __restrict__ sum, uint32_t* __restrict__ sum_sq) {
    const uint64_t row = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (row >= n_rows) return;
    const uint64_t* const x = X + row * stride_words;
    uint32_t n_lo = 0, n_hi = 0, n_both = 0;
    for (uint32_t w = lane; w < n_words; w += kLanes) {
        const uint64_t v = x[w];
        const uint64_t lo = v & 0x5555555555555555ull, hi = (v >> 1) & 0x5555555555555555ull;
        n_lo += (uint32_t)__popcll(lo);
        n_hi += (uint32_t)__popcll(hi);
        n_both += (uint32_t)__popcll(lo & hi);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n_lo += __shfl_down(n_lo, off, kLanes);
        n_hi += __shfl_down(n_hi, off, kLanes);
        n_both += __shfl_down(n_both, off, kLanes);
    }
    if (lane == 0) {
        sum[row] = n_lo + 2u * n_hi;
        sum_sq[row] = n_lo + 4u * n_hi + 4u * n_both;
    }
}

// r / r^2 as finish_tiles_kernel.inc takes them — the finishing pass over a matrix of dot products in place, shared with the
// bit statistics (storm_hip_similarity.hip) — two words per row: its sum and its sum of squares
struct DosageStat {
    static constexpr int W = 2;
    static __device__ __forceinline__ uint32_t bits(uint32_t P, const uint32_t (&a)[2], const uint32_t (&b)[2], int measure,
                                                    uint64_t n_samples) {
        return dosage_corr_bits(P, a[0], a[1], b[0], b[1], measure, n_samples);
    }
    static int check(const char* who, int measure, uint64_t n_samples) {
        if (measure != STORM_HIP_DOSAGE_R2 && measure != STORM_HIP_DOSAGE_R) {
            set_error("%s: unknown measure %d (0 r^2, 1 r)", who, measure);
            return STORM_HIP_EINVAL;
        }
        if (n_samples == 0 || n_samples > kDosageMaxSamples) {
            set_error("%s: n_samples %llu is not in [1, 2^24]", who, (unsigned long long)n_samples);
            return STORM_HIP_EINVAL;
        }
        return STORM_HIP_OK;
    }
};

#include "finish_tiles_kernel.inc"

// ---- rows with missing genotypes ----
// One word per thread: word w of row `row` of X into the same word of G, H and M (rows of `stride_words` words each,
// rows_pad rows: the rows behind n_rows and the words behind n_words — the pad up to the stride and the 512-bit chunk — come
// out zero in all three, and so do M's tail samples of the last word).
__global__ __launch_bounds__(256) void dosage_split_missing_kernel(const uint64_t* __restrict__ X, uint64_t stride_words,
                                                                   uint64_t n_rows, uint64_t rows_pad, uint32_t n_words,
                                                                   uint64_t n_samples, uint64_t* __restrict__ G,
                                                                   uint64_t* __restrict__ H, uint64_t* __restrict__ M) {
    const uint64_t w = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t row = blockIdx.y;
    if (w >= stride_words || row >= rows_pad) return;
    const bool data = row < n_rows && w < n_words;
    const uint64_t x = data ? X[row * stride_words + w] : 0ull;
    uint64_t g, h, m;
    dosage_split_word(x, data ? dosage_valid_mask(w, n_words, n_samples) : 0ull, &g, &h, &m);
    const uint64_t at = row * stride_words + w;
    G[at] = g;
    H[at] = h;
    M[at] = m;
}

// One wave per row: the samples of a row that are missing (code 3 below n_samples). Four rows per workgroup.
__global__ __launch_bounds__(kThreads) void dosage_row_missing_kernel(const uint64_t* __restrict__ X, uint64_t stride_words,
                                                                      uint64_t n_rows, uint32_t n_words, uint64_t n_samples,
                                                                      uint32_t* __restrict__ missing) {
    const uint64_t row = (uint64_t)blockIdx.x * kWaves + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (row >= n_rows) return;
    const uint64_t* const x = X + row * stride_words;
    uint32_t present = 0;
    for (uint32_t w = lane; w < n_words; w += kLanes) {
        uint64_t g, h, m;
        dosage_split_word(x[w], dosage_valid_mask(w, n_words, n_samples), &g, &h, &m);
        present += (uint32_t)__popcll(m);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) present += __shfl_down(present, off, kLanes);
    if (lane == 0) missing[row] = (uint32_t)n_samples - present;
}

constexpr int kDosCompleteTile = 64;   // a workgroup finishes 64 x 64 entries: wave w rows w, w + 4, ..., lane = column

// The finishing pass of the pairwise-complete correlation over the upper triangle of an n x n matrix of dot products P, in
// place (uint32 -> float). Entry (i, j) needs N(i, j) (`nobs`), sx = GM(i, j), qx = sx + 2 HM(i, j) and — from the
// TRANSPOSED position — sy = GM(j, i), qy = sy + 2 HM(j, i) (`gm`, `hm`: n x n each, pitch lds, like nobs). The block
// GM / HM [col0 .. + 63][row0 .. + 63] is read by rows (one 256-byte run per wave instruction) into the LDS at a pitch
// of 65 words and read back down its columns without a bank conflict. Grid (column tiles, row tiles); a tile wholly at or
// below the diagonal exits at once; entries i >= j, the pitch columns and rows beyond n are neither read nor written.
__global__ __launch_bounds__(256) void dosage_complete_finish_kernel(uint32_t* __restrict__ io, uint64_t ld, uint64_t n,
                                                                     const uint32_t* __restrict__ nobs,
                                                                     const uint32_t* __restrict__ gm,
                                                                     const uint32_t* __restrict__ hm, uint64_t lds, int measure) {
    const uint64_t row0 = (uint64_t)blockIdx.y * kDosCompleteTile, col0 = (uint64_t)blockIdx.x * kDosCompleteTile;
    if (col0 + kDosCompleteTile <= row0 + 1) return;   // the tile's last column is not beyond its first row
    __shared__ uint32_t t_gm[kDosCompleteTile][kDosCompleteTile + 1], t_hm[kDosCompleteTile][kDosCompleteTile + 1];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    for (uint32_t r = wave; r < kDosCompleteTile; r += 4) {   // row col0 + r of GM / HM, its columns row0 .. row0 + 63
        const bool in = col0 + r < n && row0 + lane < n;
        const uint64_t at = (col0 + r) * lds + row0 + lane;
        t_gm[r][lane] = in ? gm[at] : 0u;
        t_hm[r][lane] = in ? hm[at] : 0u;
    }
    __syncthreads();
    const uint64_t j = col0 + lane;
    for (uint32_t a = wave; a < kDosCompleteTile; a += 4) {
        const uint64_t i = row0 + a;
        if (i >= n || j >= n || j <= i) continue;
        const uint64_t at = i * lds + j;
        const uint32_t sx = gm[at], sy = t_gm[lane][a];
        const uint32_t qx = sx + 2u * hm[at], qy = sy + 2u * t_hm[lane][a];
        io[i * ld + j] = dosage_corr_complete_bits(io[i * ld + j], nobs[at], sx, sy, qx, qy, measure);
    }
}

// ---- the lag layout ("K2h, dosage form in the lag layout") ----
// One word per thread of the INTERLEAVED split of X (dosage_interleaved_word: row 3 i = G_i, 3 i + 1 = H_i, 3 i + 2 = M_i):
// rows_out rows of stride_words words, zero behind row 3 n_rows and behind word n_words. Grid (rows, word tiles).
__global__ __launch_bounds__(256) void dosage_split_interleaved_kernel(const uint64_t* __restrict__ X, uint64_t stride_words,
                                                                       uint64_t n_rows, uint64_t rows_out, uint32_t n_words,
                                                                       uint64_t n_samples, uint64_t* __restrict__ T) {
    const uint64_t w = (uint64_t)blockIdx.y * 256u + threadIdx.x;
    const uint64_t r = blockIdx.x;
    if (w >= stride_words || r >= rows_out) return;
    T[r * stride_words + w] = dosage_interleaved_word(X, stride_words, n_rows, n_words, n_samples, r, w);
}

constexpr uint32_t kDosLagTile = 64;                     // a workgroup finishes 64 rows x 64 lags ...
constexpr uint32_t kDosLagPass = 8;                      // ... 8 rows at a time: wave w rows w and w + 4 of a pass
constexpr uint32_t kDosLagRun = 3u * kDosLagTile + 2u;   // the columns of a scratch row that 64 lags read
constexpr uint32_t kDosLagPitch = kDosLagRun + 2u;

// The finishing pass of the pairwise-complete correlation in the lag layout. `sums` is the lag layout (lag 3 lag + 2, pitch
// lds) of the dot products of the interleaved split (3 n rows): the six sums of entry (i, d) sit in its rows 3 i, 3 i + 1 and
// 3 i + 2 at columns 3 d .. 3 d + 4 (dosage_interleaved_entry_bits). A wave reads the run [3 col0, 3 col0 + 194) of each of
// the three rows of a row i — consecutive lanes, consecutive words — into the LDS, and lane l takes its six words from
// there at a stride of 3 words (no bank conflict). Writes out[i * ld + d] for d < lag, i + 1 + d < n, nothing else; reads
// nothing of `sums` beyond column lds of a row (what lies in its own corner is read into the LDS and never used).
__global__ __launch_bounds__(256) void dosage_complete_finish_lag_kernel(const uint32_t* __restrict__ sums, uint64_t lds,
                                                                         uint32_t* __restrict__ out, uint64_t ld, uint64_t n,
                                                                         uint64_t lag, int measure) {
    const uint64_t i0 = (uint64_t)blockIdx.y * kDosLagTile, col0 = (uint64_t)blockIdx.x * kDosLagTile;
    if (i0 + 1 + col0 >= n) return;   // the tile's first pair is already in the corner
    __shared__ uint32_t t[kDosLagPass][3][kDosLagPitch];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t d = col0 + lane;
    for (uint32_t pass = 0; pass < kDosLagTile / kDosLagPass; ++pass) {
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t k = wave + 4u * h;
            const uint64_t i = i0 + pass * kDosLagPass + k;
#pragma unroll
            for (uint32_t a = 0; a < 3; ++a) {
                const uint32_t* const row = sums + (3u * i + a) * lds + 3u * col0;
                for (uint32_t c = lane; c < kDosLagRun; c += 64u) t[k][a][c] = (i < n && 3u * col0 + c < lds) ? row[c] : 0u;
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t k = wave + 4u * h;
            const uint64_t i = i0 + pass * kDosLagPass + k;
            if (i < n && d < lag && i + 1 + d < n)
                out[i * ld + d] = dosage_interleaved_entry_bits(t[k][0], t[k][1], t[k][2], lane, measure);
        }
        __syncthreads();
    }
}

// the rows' sums into the context's row-count scratch: sum at [0, n), sum of squares at [n, 2 n); queued
static int dosage_sums_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m) {
    const uint64_t n = m->n_rows;
    if (int rc = ctx->d_counts.ensure(2 * n * sizeof(uint32_t), "dosage: the row-sum scratch")) return rc;
    hipLaunchKernelGGL(dosage_row_sums_kernel, dim3((uint32_t)((n + kWaves - 1) / kWaves)), dim3(kThreads), 0, ctx->stream, m->d,
                       m->stride_words, n, m->n_words, ctx->d_counts.d, ctx->d_counts.d + n);
    STORM_HIP_TRY(hipGetLastError());
    return STORM_HIP_OK;
}

// dot products at d_io (pitch ld), the rows' sums, then the finish: all queued
static int dosage_corr_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, int measure, uint64_t n_samples, uint32_t* d_io,
                              uint64_t ld) {
    const uint64_t n = m->n_rows;
    if (int rc = launch_pairw_dosage_matrix(ctx, m, d_io, ld)) return rc;
    if (int rc = dosage_sums_queued(ctx, m)) return rc;
    if (!finish_tiles_fit(n, n)) {
        set_error("pairw_dosage_corr: %llu rows exceed the finishing pass's launch grid", (unsigned long long)n);
        return STORM_HIP_EINVAL;
    }
    const StatWords<2> sums{{ctx->d_counts.d, ctx->d_counts.d + n}};
    return launch_finish_tiles<DosageStat>(ctx, "pairw_dosage_corr", d_io, ld, n, n, sums, sums, true, measure, n_samples);
}

// The split operands of a matrix with missing genotypes, in ctx->d_dosage_rows: G, H and M as matrices of rows128 =
// n_rows up to the next multiple of 128 rows each (zero rows behind n_rows), G and H adjacent so that [G ; H] is one matrix
// of rows128 + n_rows rows. Queued.
// (struct DosageSplit: storm_hip_internal.h — the top-k calls take panels of its matrices)
// the words of one matrix of the split (rows128 rows of the source's stride); refuses what the split's launch grid cannot hold
static int dosage_split_words(const storm_hip_matrix_s* x, uint64_t* words) {
    const uint64_t rows128 = (x->n_rows + kThTile - 1) / kThTile * kThTile;
    if (rows128 > 65535u) {
        set_error("dosage rows with missing genotypes: %llu rows exceed the split's launch grid", (unsigned long long)x->n_rows);
        return STORM_HIP_EINVAL;
    }
    *words = rows128 * x->stride_words;
    return STORM_HIP_OK;
}
// the split of x at G (3 x dosage_split_words words of ctx->d_dosage_rows, already there), queued
static int dosage_split_at(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* x, uint64_t n_samples, uint64_t* G, DosageSplit* out) {
    const uint64_t n = x->n_rows, rows128 = (n + kThTile - 1) / kThTile * kThTile, stride = x->stride_words;
    const uint64_t words = rows128 * stride;
    hipLaunchKernelGGL(dosage_split_missing_kernel, dim3((uint32_t)((stride + 255u) / 256u), (uint32_t)rows128), dim3(256), 0,
                       ctx->stream, x->d, stride, n, rows128, x->n_words, n_samples, G, G + words, G + 2 * words);
    STORM_HIP_TRY(hipGetLastError());
    auto view = [&](uint64_t* d, uint64_t rows, uint64_t rows_pad) {
        storm_hip_matrix_s v;
        v.d = d;
        v.n_rows = rows;
        v.n_rows_pad = rows_pad;
        v.n_words = x->n_words;
        v.stride_words = stride;
        return v;
    };
    out->rows128 = rows128;
    out->g = view(G, n, rows128);
    out->gh = view(G, rows128 + n, 2 * rows128);
    out->ghm = view(G, 2 * rows128 + n, 3 * rows128);   // (the rectangle of two containers: [G ; H ; M] as ONE operand)
    out->m = view(G + 2 * words, n, rows128);
    return STORM_HIP_OK;
}
static int dosage_split_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* x, uint64_t n_samples, DosageSplit* out) {
    uint64_t words = 0;
    if (int rc = dosage_split_words(x, &words)) return rc;
    if (int rc = ctx->d_dosage_rows.ensure(3 * words * sizeof(uint64_t), "dosage rows with missing genotypes: the split operands G, H, M"))
        return rc;
    return dosage_split_at(ctx, x, n_samples, ctx->d_dosage_rows.d, out);
}

// N(i, j) for i < j at d_out (pitch ld): the split, then the triangle of M. Queued.
static int dosage_nobs_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, uint64_t n_samples, uint32_t* d_out, uint64_t ld) {
    DosageSplit sp;
    if (int rc = dosage_split_queued(ctx, m, n_samples, &sp)) return rc;
    return launch_pairw_dosage_matrix(ctx, &sp.m, d_out, ld);
}

// The pairwise-complete correlation at d_io (pitch ld): the split; P = the triangle of G straight into d_io; N = the
// triangle of M and [G ; H] x M (rows [0, n): G M^T, rows [rows128, rows128 + n): H M^T) into ctx->d_dosage_sums — 3 n^2
// row-pair products on the matrix cores; then the finish in place. Scratch: about 3 n^2 uint32 of sums (n + rows128 + n rows
// of n up to the next multiple of 4 columns) and 3 rows128 rows of operands. All queued.
static int dosage_corr_complete_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, int measure, uint64_t n_samples,
                                       uint32_t* d_io, uint64_t ld) {
    const uint64_t n = m->n_rows;
    DosageSplit sp;
    if (int rc = dosage_split_queued(ctx, m, n_samples, &sp)) return rc;
    const uint64_t lds = (n + 3u) / 4u * 4u;
    if (int rc = ctx->d_dosage_sums.ensure((2 * n + sp.rows128) * lds * sizeof(uint32_t),
                                           "pairw_dosage_corr_complete: the sums N, G M^T and H M^T"))
        return rc;
    uint32_t* const d_nobs = ctx->d_dosage_sums.d;
    uint32_t* const d_gm = d_nobs + n * lds;
    uint32_t* const d_hm = d_gm + sp.rows128 * lds;
    // (the two triangles are planned alike: the second one launches from the first one's list)
    if (int rc = launch_pairw_dosage_matrix(ctx, &sp.g, d_io, ld)) return rc;
    if (int rc = launch_pairw_dosage_matrix(ctx, &sp.m, d_nobs, lds)) return rc;
    if (int rc = launch_square_dosage_matrix(ctx, &sp.gh, &sp.m, d_gm, lds)) return rc;
    const uint64_t tiles = (n + kDosCompleteTile - 1) / kDosCompleteTile;
    if (tiles > 65535u) {
        set_error("pairw_dosage_corr_complete: %llu rows exceed the finishing pass's launch grid", (unsigned long long)n);
        return STORM_HIP_EINVAL;
    }
    hipLaunchKernelGGL(dosage_complete_finish_kernel, dim3((uint32_t)tiles, (uint32_t)tiles), dim3(256), 0, ctx->stream, d_io, ld, n,
                       d_nobs, d_gm, d_hm, lds, measure);
    STORM_HIP_TRY(hipGetLastError());
    ctx->pass_report[0] = STORM_HIP_RAN_TILES_OUT | STORM_HIP_RAN_SIMILARITY;
    ctx->pass_report[1] = 3 * n * n * m->n_words;
    return STORM_HIP_OK;
}

// what every dosage call refuses alike
static int check_dosage(const char* who, const storm_hip_matrix_s* m, const void* out, uint64_t ld) {
    if (!m || !out) {
        set_error("%s: NULL argument", who);
        return STORM_HIP_EINVAL;
    }
    if (ld < m->n_rows) {
        set_error("%s: leading dimension %llu < rows %llu", who, (unsigned long long)ld, (unsigned long long)m->n_rows);
        return STORM_HIP_EINVAL;
    }
    if ((uint64_t)m->n_words * 32u > kDosageMaxSamples) {
        set_error("%s: rows of %u words hold more than 2^24 values", who, m->n_words);
        return STORM_HIP_EINVAL;
    }
    return STORM_HIP_OK;
}
int check_samples(const char* who, const storm_hip_matrix_s* m, uint64_t n_samples) {
    if (n_samples == 0 || (n_samples + 31u) / 32u != m->n_words) {
        set_error("%s: %llu samples do not fill rows of %u words (32 values per word)", who, (unsigned long long)n_samples,
                  m->n_words);
        return STORM_HIP_EINVAL;
    }
    return STORM_HIP_OK;
}
static int check_corr(const char* who, const storm_hip_matrix_s* m, int measure, uint64_t n_samples) {
    if (measure != STORM_HIP_DOSAGE_R2 && measure != STORM_HIP_DOSAGE_R) {
        set_error("%s: unknown measure %d (0 r^2, 1 r)", who, measure);
        return STORM_HIP_EINVAL;
    }
    return check_samples(who, m, n_samples);
}
// the rectangle of two dosage matrices: rows of the same width
int check_square(const char* who, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, const void* out, uint64_t ld) {
    if (!a || !b || !out) {
        set_error("%s: NULL argument", who);
        return STORM_HIP_EINVAL;
    }
    if (a->n_words != b->n_words || a->stride_words != b->stride_words) {
        set_error("%s: rows of %u and of %u words (both matrices must hold the same number of samples)", who, a->n_words,
                  b->n_words);
        return STORM_HIP_EINVAL;
    }
    if (ld < b->n_rows) {
        set_error("%s: leading dimension %llu < B's rows %llu", who, (unsigned long long)ld, (unsigned long long)b->n_rows);
        return STORM_HIP_EINVAL;
    }
    if ((uint64_t)a->n_words * 32u > kDosageMaxSamples) {
        set_error("%s: rows of %u words hold more than 2^24 values", who, a->n_words);
        return STORM_HIP_EINVAL;
    }
    return STORM_HIP_OK;
}

// ---- the rectangle of two matrices: r / r^2 and N of every row of A against every row of B ("K2h, dosage
// form: the rectangle of two containers") ----
// The finishing pass of the pairwise-complete correlation over an n_a x n_b matrix of dot products P = G_a G_b^T, in place
// (uint32 -> float). All six sums of entry (i, j) lie at (i, j) of their matrices — `ghm` = [G_a ; H_a] x M_b (pitch ld_ghm:
// sx at row i, H_a M_b at row h_row0 + i) and `mghm` = M_a x [G_b ; H_b ; M_b] (pitch ld_mghm: sy at column j, M_a H_b at
// h_col0 + j, N at m_col0 + j) — so there is no transposed tile and no LDS: wave w takes rows w, w + 4, ... of a 64 x 64
// tile, lane = column, every read one run along j. Entries outside the n_a x n_b window are neither read nor written.
__global__ __launch_bounds__(256) void dosage_square_complete_finish_kernel(uint32_t* __restrict__ io, uint64_t ld, uint64_t n_a,
                                                                            uint64_t n_b, const uint32_t* __restrict__ ghm,
                                                                            uint64_t ld_ghm, uint64_t h_row0,
                                                                            const uint32_t* __restrict__ mghm, uint64_t ld_mghm,
                                                                            uint64_t h_col0, uint64_t m_col0, int measure) {
    const uint64_t row0 = (uint64_t)blockIdx.y * kDosCompleteTile, j = (uint64_t)blockIdx.x * kDosCompleteTile + (threadIdx.x & 63u);
    if (j >= n_b) return;
    for (uint32_t a = threadIdx.x >> 6; a < kDosCompleteTile; a += 4 * kFinishUnroll) {
        uint32_t P[kFinishUnroll], N[kFinishUnroll], sx[kFinishUnroll], sy[kFinishUnroll], hx[kFinishUnroll], hy[kFinishUnroll];
#pragma unroll
        for (int u = 0; u < kFinishUnroll; ++u) {   // the loads of kFinishUnroll rows leave before the first divide
            const uint64_t i = row0 + a + 4u * u;
            if (i >= n_a) continue;
            const uint32_t* const mrow = mghm + i * ld_mghm;
            P[u] = io[i * ld + j];
            sx[u] = ghm[i * ld_ghm + j];
            hx[u] = ghm[(h_row0 + i) * ld_ghm + j];
            sy[u] = mrow[j];
            hy[u] = mrow[h_col0 + j];
            N[u] = mrow[m_col0 + j];
        }
#pragma unroll
        for (int u = 0; u < kFinishUnroll; ++u) {
            const uint64_t i = row0 + a + 4u * u;
            if (i < n_a) io[i * ld + j] = dosage_corr_complete_bits(P[u], N[u], sx[u], sy[u], sx[u] + 2u * hx[u], sy[u] + 2u * hy[u], measure);
        }
    }
}

// the sums of both matrices' rows into the context's row-count scratch, 2 (n_a + n_b) words: A's s and q, then B's; queued
// (struct SquareSums: storm_hip_internal.h)
int dosage_square_sums_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, SquareSums* out) {
    const uint64_t na = a->n_rows, nb = b->n_rows;
    if (int rc = ctx->d_counts.ensure(2 * (na + nb) * sizeof(uint32_t), "square_dosage_corr: the row-sum scratch")) return rc;
    uint32_t* const d = ctx->d_counts.d;
    hipLaunchKernelGGL(dosage_row_sums_kernel, dim3((uint32_t)((na + kWaves - 1) / kWaves)), dim3(kThreads), 0, ctx->stream, a->d,
                       a->stride_words, na, a->n_words, d, d + na);
    hipLaunchKernelGGL(dosage_row_sums_kernel, dim3((uint32_t)((nb + kWaves - 1) / kWaves)), dim3(kThreads), 0, ctx->stream, b->d,
                       b->stride_words, nb, b->n_words, d + 2 * na, d + 2 * na + nb);
    STORM_HIP_TRY(hipGetLastError());
    *out = SquareSums{d, d + na, d + 2 * na, d + 2 * na + nb};
    return STORM_HIP_OK;
}

// r / r^2 of every row of A against every row of B at d_io (pitch ld), 3 an ordinary value: the dot products, both
// matrices' row sums, then the finish in place. All queued.
static int square_dosage_corr_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, int measure,
                                     uint64_t n_samples, uint32_t* d_io, uint64_t ld) {
    const uint64_t na = a->n_rows, nb = b->n_rows;
    if (!finish_tiles_fit(na, nb)) {   // (before anything is queued)
        set_error("square_dosage_corr: %llu x %llu entries exceed the finishing pass's launch grid", (unsigned long long)na,
                  (unsigned long long)nb);
        return STORM_HIP_EINVAL;
    }
    if (int rc = launch_square_dosage_matrix(ctx, a, b, d_io, ld)) return rc;
    SquareSums s;
    if (int rc = dosage_square_sums_queued(ctx, a, b, &s)) return rc;
    // (the report's [1]: n_a n_b n_words, the launch's own)
    return launch_finish_tiles<DosageStat>(ctx, "square_dosage_corr", d_io, ld, na, nb, {{s.a_sum, s.a_sq}}, {{s.b_sum, s.b_sq}}, false,
                                           measure, n_samples);
}

// The splits of both matrices side by side in ctx->d_dosage_rows (A's three matrices, then B's; one split when b is a),
// queued. The buffer is sized for both before either kernel starts: growing it drops what it held.
int dosage_split_pair_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, uint64_t n_samples,
                             DosageSplit* sa, DosageSplit* sb) {
    uint64_t words_a = 0, words_b = 0;
    if (int rc = dosage_split_words(a, &words_a)) return rc;
    if (b != a)
        if (int rc = dosage_split_words(b, &words_b)) return rc;
    if (int rc = ctx->d_dosage_rows.ensure(3 * (words_a + words_b) * sizeof(uint64_t),
                                           "dosage rows with missing genotypes: the split operands G, H, M of two matrices"))
        return rc;
    if (int rc = dosage_split_at(ctx, a, n_samples, ctx->d_dosage_rows.d, sa)) return rc;
    if (b == a) {
        *sb = *sa;
        return STORM_HIP_OK;
    }
    return dosage_split_at(ctx, b, n_samples, ctx->d_dosage_rows.d + 3 * words_a, sb);
}

// N(i, j) of every row of A against every row of B at d_out (pitch ld): the splits, then M_a x M_b. Queued.
static int square_dosage_nobs_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, uint64_t n_samples,
                                     uint32_t* d_out, uint64_t ld) {
    DosageSplit sa, sb;
    if (int rc = dosage_split_pair_queued(ctx, a, b, n_samples, &sa, &sb)) return rc;
    return launch_square_dosage_matrix(ctx, &sa.m, &sb.m, d_out, ld);   // ([1]: n_a n_b n_words)
}

// The pairwise-complete correlation of every row of A against every row of B at d_io (pitch ld): the splits; six n_a x n_b
// products on K2h in three launches — P = G_a x G_b straight into d_io, [G_a ; H_a] x M_b (rows [0, n_a): sx, rows
// [rows128_a, rows128_a + n_a): H_a M_b) and M_a x [G_b ; H_b ; M_b] (columns [0, n_b): sy, from rows128_b: M_a H_b, from
// 2 rows128_b: N; the operand's zero rows between the three cost up to 127 columns each) into ctx->d_dosage_sums — then the
// finish in place. Scratch: about 5 n_a n_b uint32 of sums and both splits. All queued.
static int square_dosage_corr_complete_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b,
                                              int measure, uint64_t n_samples, uint32_t* d_io, uint64_t ld) {
    const uint64_t na = a->n_rows, nb = b->n_rows;
    const uint64_t tiles_x = (nb + kDosCompleteTile - 1) / kDosCompleteTile, tiles_y = (na + kDosCompleteTile - 1) / kDosCompleteTile;
    if (tiles_y > 65535u || tiles_x > 0x7fffffffu) {
        set_error("square_dosage_corr_complete: %llu x %llu entries exceed the finishing pass's launch grid", (unsigned long long)na,
                  (unsigned long long)nb);
        return STORM_HIP_EINVAL;
    }
    DosageSplit sa, sb;
    if (int rc = dosage_split_pair_queued(ctx, a, b, n_samples, &sa, &sb)) return rc;
    const uint64_t ld_ghm = (nb + 3u) / 4u * 4u, ld_mghm = 2 * sb.rows128 + ld_ghm;
    const uint64_t ghm_words = (sa.rows128 + na) * ld_ghm;
    if (int rc = ctx->d_dosage_sums.ensure((ghm_words + na * ld_mghm) * sizeof(uint32_t),
                                           "square_dosage_corr_complete: the sums [G_a ; H_a] M_b^T and M_a [G_b ; H_b ; M_b]^T"))
        return rc;
    uint32_t* const d_ghm = ctx->d_dosage_sums.d;
    uint32_t* const d_mghm = d_ghm + ghm_words;
    if (int rc = launch_square_dosage_matrix(ctx, &sa.g, &sb.g, d_io, ld)) return rc;
    if (int rc = launch_square_dosage_matrix(ctx, &sa.gh, &sb.m, d_ghm, ld_ghm)) return rc;
    if (int rc = launch_square_dosage_matrix(ctx, &sa.m, &sb.ghm, d_mghm, ld_mghm)) return rc;
    hipLaunchKernelGGL(dosage_square_complete_finish_kernel, dim3((uint32_t)tiles_x, (uint32_t)tiles_y), dim3(256), 0, ctx->stream, d_io,
                       ld, na, nb, d_ghm, ld_ghm, sa.rows128, d_mghm, ld_mghm, sb.rows128, 2 * sb.rows128, measure);
    STORM_HIP_TRY(hipGetLastError());
    ctx->pass_report[0] = STORM_HIP_RAN_TILES_OUT | STORM_HIP_RAN_SIMILARITY;
    ctx->pass_report[1] = 6 * na * nb * a->n_words;
    return STORM_HIP_OK;
}

// ---- the lag layout ----
// what the lag calls of the dosage form refuse alike (check_lag, and check_dosage's width test); *lag = L
static int check_lag_dosage(const char* who, const storm_hip_matrix_s* m, const void* out, uint64_t max_lag, uint64_t ld,
                            uint64_t* lag) {
    if (int rc = check_lag(who, m, out, max_lag, ld, lag)) return rc;
    if ((uint64_t)m->n_words * 32u > kDosageMaxSamples) {
        set_error("%s: rows of %u words hold more than 2^24 values", who, m->n_words);
        return STORM_HIP_EINVAL;
    }
    return STORM_HIP_OK;
}

// r / r^2 over a matrix of dot products in the lag layout, asynchronous (the checks of storm_hip_dosage_finish_lag_device)
static int launch_dosage_finish_lag(storm_hip_ctx_t* ctx, void* d_io, uint64_t ld, uint64_t n_rows, uint64_t row0,
                                    uint64_t n_band_rows, uint64_t max_lag, const uint32_t* d_sum, const uint32_t* d_sum_sq,
                                    int measure, uint64_t n_samples) {
    return launch_finish_lag_tiles<DosageStat>(ctx, "dosage_finish_lag", d_io, ld, n_rows, row0, n_band_rows, max_lag,
                                               {{d_sum, d_sum_sq}}, measure, n_samples);
}

// dot products in the lag layout at d_io (pitch ld), the rows' sums, then the finish: all queued
static int lag_dosage_corr_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, int measure, uint64_t n_samples,
                                  uint64_t max_lag, uint32_t* d_io, uint64_t ld) {
    const uint64_t n = m->n_rows;
    if (int rc = launch_pairw_lag_dosage_matrix(ctx, m, max_lag, 0, n, d_io, ld)) return rc;
    if (int rc = dosage_sums_queued(ctx, m)) return rc;
    return launch_dosage_finish_lag(ctx, d_io, ld, n, 0, n, max_lag, ctx->d_counts.d, ctx->d_counts.d + n, measure, n_samples);
}

// The interleaved split of a matrix with missing genotypes, in ctx->d_dosage_rows: one matrix of 3 n rows (G_i, H_i, M_i at
// rows 3 i, 3 i + 1, 3 i + 2) of the source's stride, zero rows up to the next multiple of 128 (and two more: M's view
// below ends a row pitch behind its last row). `m`: the M rows alone, a view of every third row. Queued.
struct DosageInterleaved {
    storm_hip_matrix_s all, m;   // views into the scratch (never destroyed)
};
static int dosage_interleave_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* x, uint64_t n_samples, DosageInterleaved* out) {
    const uint64_t n = x->n_rows, stride = x->stride_words;
    const uint64_t rows128 = (3 * n + kThTile - 1) / kThTile * kThTile, rows_out = rows128 + 2;
    if (rows_out > 0x7fffffffu) {
        set_error("dosage rows with missing genotypes: %llu rows exceed the split's launch grid", (unsigned long long)n);
        return STORM_HIP_EINVAL;
    }
    if (int rc = ctx->d_dosage_rows.ensure(rows_out * stride * sizeof(uint64_t),
                                           "dosage rows with missing genotypes: the interleaved operand G, H, M"))
        return rc;
    uint64_t* const T = ctx->d_dosage_rows.d;
    hipLaunchKernelGGL(dosage_split_interleaved_kernel, dim3((uint32_t)rows_out, (uint32_t)((stride + 255u) / 256u)), dim3(256), 0,
                       ctx->stream, x->d, stride, n, rows_out, x->n_words, n_samples, T);
    STORM_HIP_TRY(hipGetLastError());
    auto view = [&](uint64_t* d, uint64_t rows, uint64_t rows_pad, uint64_t stride_words) {
        storm_hip_matrix_s v;
        v.d = d;
        v.n_rows = rows;
        v.n_rows_pad = rows_pad;
        v.n_words = x->n_words;
        v.stride_words = stride_words;
        return v;
    };
    out->all = view(T, 3 * n, rows128, stride);
    out->m = view(T + 2 * stride, n, n, 3 * stride);
    return STORM_HIP_OK;
}

// N(i, i + 1 + d) in the lag layout at d_out (pitch ld): the split, then the lag form on the M rows. Queued.
static int lag_dosage_nobs_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, uint64_t n_samples, uint64_t max_lag,
                                  uint32_t* d_out, uint64_t ld) {
    DosageInterleaved sp;
    if (int rc = dosage_interleave_queued(ctx, m, n_samples, &sp)) return rc;
    return launch_pairw_lag_dosage_matrix(ctx, &sp.m, max_lag, 0, m->n_rows, d_out, ld);
}

// The pitch of the scratch matrix of sums below (lag_dosage_r2_band_queued hands N out of it to the LD-score calls): 3 L + 2 columns up to the next
// multiple of 4.
static inline uint64_t lag_complete_pitch(uint64_t L) { return (3 * L + 2 + 3u) / 4u * 4u; }

// The pairwise-complete correlation in the lag layout at d_out (pitch ld): the interleaved split; ONE launch of K2h in its
// lag and dosage form over its 3 n rows at lag 3 L + 2 into ctx->d_dosage_sums — every product of G, H, M of two rows within
// L of each other: 9 per row pair where the finish reads 6 — then the finish into d_out. Scratch: 3 n x (3 L + 2 up to the
// next multiple of 4) uint32 of sums and 3 n rows of operands: O(n L), nothing of n^2. All queued.
static int lag_dosage_corr_complete_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, int measure, uint64_t n_samples,
                                           uint64_t max_lag, uint32_t* d_out, uint64_t ld) {
    const uint64_t n = m->n_rows, L = std::min<uint64_t>(max_lag, n - 1);
    const uint64_t lag3 = 3 * L + 2, lds = lag_complete_pitch(L);
    const uint64_t tiles_x = (L + kDosLagTile - 1) / kDosLagTile, tiles_y = (n + kDosLagTile - 1) / kDosLagTile;
    if (tiles_y > 65535u || tiles_x > 0x7fffffffu) {
        set_error("pairw_lag_dosage_corr_complete: %llu rows exceed the finishing pass's launch grid", (unsigned long long)n);
        return STORM_HIP_EINVAL;
    }
    DosageInterleaved sp;
    if (int rc = dosage_interleave_queued(ctx, m, n_samples, &sp)) return rc;
    if (int rc = ctx->d_dosage_sums.ensure(3 * n * lds * sizeof(uint32_t),
                                           "pairw_lag_dosage_corr_complete: the sums of the interleaved rows within the lag"))
        return rc;
    if (int rc = launch_pairw_lag_dosage_matrix(ctx, &sp.all, lag3, 0, 3 * n, ctx->d_dosage_sums.d, lds)) return rc;
    hipLaunchKernelGGL(dosage_complete_finish_lag_kernel, dim3((uint32_t)tiles_x, (uint32_t)tiles_y), dim3(256), 0, ctx->stream,
                       ctx->d_dosage_sums.d, lds, d_out, ld, n, L, measure);
    STORM_HIP_TRY(hipGetLastError());
    ctx->pass_report[0] |= STORM_HIP_RAN_SIMILARITY;   // ([1]: the interleaved rows' pairs within 3 L + 2 x n_words)
    return STORM_HIP_OK;
}

// ---- the band of r^2 in ctx->d_band, as every composed call below starts ----
// r^2 (complete-case or pairwise-complete) of the pairs within the lag in the first n x L floats of the band buffer, and
// `tail_words` words behind them that are the caller's to lay out. `n`: where the pairwise-complete call left N(i, d), row
// 3 i + 2, column 3 d + 2 of ctx->d_dosage_sums (dosage_interleaved_entry_bits): N(i, d) = n[i * n_ld + d * n_step]. NULL
// in the complete-case form, which has no such matrix.
struct LagR2Band {
    uint32_t *band, *tail;
    const uint32_t* n;
    uint64_t n_ld, n_step;
};
// the buffer alone: a caller with arrays to send ahead of the band's kernels queues them between this and the next
static int lag_dosage_r2_band_ensure(storm_hip_ctx_t* ctx, uint64_t n, uint64_t lag, size_t tail_words, const char* what,
                                     LagR2Band* out) {
    const size_t band = (size_t)n * lag;
    if (int rc = ctx->d_band.ensure((band + tail_words) * sizeof(uint32_t), what)) return rc;
    *out = LagR2Band{ctx->d_band.d, ctx->d_band.d + band, nullptr, 0, 0};
    return STORM_HIP_OK;
}
// the band's kernels, queued
static int lag_dosage_r2_band_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, uint64_t n_samples, uint64_t max_lag,
                                     uint64_t lag, bool complete, LagR2Band* b) {
    if (int rc = complete ? lag_dosage_corr_complete_queued(ctx, m, STORM_HIP_DOSAGE_R2, n_samples, max_lag, b->band, lag)
                          : lag_dosage_corr_queued(ctx, m, STORM_HIP_DOSAGE_R2, n_samples, max_lag, b->band, lag))
        return rc;
    const uint64_t lds = lag_complete_pitch(lag);
    b->n = complete ? ctx->d_dosage_sums.d + 2 * lds + 2 : nullptr;
    b->n_ld = 3 * lds;
    b->n_step = 3;
    return STORM_HIP_OK;
}
static int lag_dosage_r2_band(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, uint64_t n_samples, uint64_t max_lag, uint64_t lag,
                              bool complete, size_t tail_words, const char* what, LagR2Band* out) {
    if (int rc = lag_dosage_r2_band_ensure(ctx, m->n_rows, lag, tail_words, what, out)) return rc;
    return lag_dosage_r2_band_queued(ctx, m, n_samples, max_lag, lag, complete, out);
}

static int check_ldscore_stat(const char* who, int stat) {
    if (stat == STORM_HIP_LDSCORE_R2 || stat == STORM_HIP_LDSCORE_R2_ADJ) return STORM_HIP_OK;
    set_error("%s: unknown stat %d (0 r^2, 1 r^2 adjusted)", who, stat);
    return STORM_HIP_EINVAL;
}

// ---- LD scores: the band, then lag_band_sums_kernel (storm_hip_ldscore.hip) over it ----
// Tail, for a host form: the n scores and the n counts on their way back. All queued on ctx->stream; the host form alone
// waits. The adjusted pairwise-complete statistic alone reads N.
static int lag_dosage_ldscore(storm_hip_ctx_t* ctx, const char* who, const storm_hip_matrix_s* m, int stat, uint64_t n_samples,
                              uint64_t max_lag, bool complete, float* score, uint32_t* n_pairs, bool host) {
    uint64_t lag = 0;
    if (int rc = check_lag_dosage(who, m, score, max_lag, ~0ull, &lag)) return rc;
    if (int rc = check_ldscore_stat(who, stat)) return rc;
    if (int rc = check_samples(who, m, n_samples)) return rc;
    const uint64_t n = m->n_rows;
    if (n < 2) return STORM_HIP_OK;
    STORM_HIP_TRY(hipSetDevice(ctx->device));
    LagR2Band b;
    if (int rc = lag_dosage_r2_band(ctx, m, n_samples, max_lag, lag, complete, host ? 2 * n : 0,
                                    "lag_dosage_ldscore: the band of r^2", &b))
        return rc;
    float* const d_score = host ? reinterpret_cast<float*>(b.tail) : score;
    uint32_t* const d_pairs = host ? b.tail + n : n_pairs;
    if (int rc = launch_lag_band_sums(ctx, reinterpret_cast<const float*>(b.band), lag, n, max_lag, stat, n_samples,
                                      stat == STORM_HIP_LDSCORE_R2_ADJ ? b.n : nullptr, b.n_ld, b.n_step, d_score, d_pairs))
        return rc;
    if (!host) return STORM_HIP_OK;
    STORM_HIP_TRY(hipMemcpyAsync(score, d_score, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (n_pairs) STORM_HIP_TRY(hipMemcpyAsync(n_pairs, d_pairs, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    STORM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return STORM_HIP_OK;
}

// ---- stratified LD scores: the band, then lag_band_annot_sums_kernel (storm_hip_ldscore_annot.hip) over it ----
// Tail: the window bounds (h_lo / h_hi are HOST arrays of n entries in every form, both or neither: the planner runs on the
// host) and, for a host form, the n x C annotations on their way in and the n x C scores and n counts on their way back, all
// dense. The bounds and the annotations are queued ahead of the band's kernels. The host form alone waits.
static int lag_dosage_ldscore_annot(storm_hip_ctx_t* ctx, const char* who, const storm_hip_matrix_s* m, int stat, uint64_t n_samples,
                                    uint64_t max_lag, bool complete, const uint32_t* h_lo, const uint32_t* h_hi, const float* annot,
                                    uint64_t annot_ld, uint64_t n_annot, float* score, uint64_t score_ld, uint32_t* n_pairs,
                                    bool host) {
    uint64_t lag = 0;
    if (int rc = check_lag_dosage(who, m, score, max_lag, ~0ull, &lag)) return rc;
    if (int rc = check_ldscore_stat(who, stat)) return rc;
    if (int rc = check_samples(who, m, n_samples)) return rc;
    if (!annot) {
        set_error("%s: NULL annotations", who);
        return STORM_HIP_EINVAL;
    }
    if (n_annot < 1 || n_annot > kLdscoreMaxAnnot) {
        set_error("%s: %llu annotation columns (1 .. %u)", who, (unsigned long long)n_annot, kLdscoreMaxAnnot);
        return STORM_HIP_EINVAL;
    }
    if (annot_ld < n_annot || score_ld < n_annot) {
        set_error("%s: annot_ld %llu or score_ld %llu < %llu annotation columns", who, (unsigned long long)annot_ld,
                  (unsigned long long)score_ld, (unsigned long long)n_annot);
        return STORM_HIP_EINVAL;
    }
    if (!h_lo != !h_hi) {
        set_error("%s: the window bounds lo and hi come together or not at all", who);
        return STORM_HIP_EINVAL;
    }
    const uint64_t n = m->n_rows;
    if (n < 2) return STORM_HIP_OK;
    STORM_HIP_TRY(hipSetDevice(ctx->device));
    const size_t cells = (size_t)n * n_annot;
    LagR2Band b;
    if (int rc = lag_dosage_r2_band_ensure(ctx, n, lag, (h_lo ? 2 * n : 0) + (host ? 2 * cells + n : 0),
                                           "lag_dosage_ldscore_annot: the band of r^2", &b))
        return rc;
    uint32_t* const d_lo = h_lo ? b.tail : nullptr;
    uint32_t* const d_hi = h_lo ? d_lo + n : nullptr;
    uint32_t* const d_io = b.tail + (h_lo ? 2 * n : 0);
    if (h_lo) {
        STORM_HIP_TRY(hipMemcpyAsync(d_lo, h_lo, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        STORM_HIP_TRY(hipMemcpyAsync(d_hi, h_hi, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    if (host)
        STORM_HIP_TRY(hipMemcpy2DAsync(d_io, n_annot * sizeof(float), annot, annot_ld * sizeof(float), n_annot * sizeof(float), n,
                                       hipMemcpyHostToDevice, ctx->stream));
    if (int rc = lag_dosage_r2_band_queued(ctx, m, n_samples, max_lag, lag, complete, &b)) return rc;
    const float* const d_annot = host ? reinterpret_cast<const float*>(d_io) : annot;
    float* const d_score = host ? reinterpret_cast<float*>(d_io + cells) : score;
    uint32_t* const d_pairs = host ? d_io + 2 * cells : n_pairs;
    if (int rc = launch_lag_band_annot_sums(ctx, reinterpret_cast<const float*>(b.band), lag, n, max_lag, stat, n_samples,
                                            stat == STORM_HIP_LDSCORE_R2_ADJ ? b.n : nullptr, b.n_ld, b.n_step, d_lo, d_hi, d_annot,
                                            host ? n_annot : annot_ld, n_annot, d_score, host ? n_annot : score_ld, d_pairs))
        return rc;
    if (!host) return STORM_HIP_OK;
    STORM_HIP_TRY(hipMemcpy2DAsync(score, score_ld * sizeof(float), d_score, n_annot * sizeof(float), n_annot * sizeof(float), n,
                                   hipMemcpyDeviceToHost, ctx->stream));
    if (n_pairs) STORM_HIP_TRY(hipMemcpyAsync(n_pairs, d_pairs, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    STORM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return STORM_HIP_OK;
}

// ---- greedy pruning / clumping: the band, then the kernels of storm_hip_prune.hip over it ----
// Tail: the adjacency masks, the window bounds and the order (h_lo / h_hi / h_order are HOST arrays of n entries in every
// form, or NULL; the launcher lays them out and sends them) and, for a host form, the n owners and the n keep bytes on their
// way back. All queued on ctx->stream; the host form alone waits.
static int lag_dosage_prune(storm_hip_ctx_t* ctx, const char* who, const storm_hip_matrix_s* m, uint64_t n_samples, uint64_t max_lag,
                            float min_r2, bool complete, const uint32_t* h_lo, const uint32_t* h_hi, const uint32_t* h_order,
                            uint8_t* keep, uint32_t* owner, bool host) {
    uint64_t lag = 0;
    if (int rc = check_lag_dosage(who, m, keep, max_lag, ~0ull, &lag)) return rc;
    if (int rc = check_samples(who, m, n_samples)) return rc;
    const uint64_t n = m->n_rows;
    if (int rc = check_lag_band_prune(who, n, h_lo, h_hi, min_r2)) return rc;
    if (n == 0) return STORM_HIP_OK;
    STORM_HIP_TRY(hipSetDevice(ctx->device));
    if (n == 1) {   // a row without any edge is kept and owns itself: no band, no kernel
        if (host) {
            keep[0] = 1;
            if (owner) owner[0] = 0;
            return STORM_HIP_OK;
        }
        STORM_HIP_TRY(hipMemsetAsync(keep, 1, 1, ctx->stream));
        if (owner) STORM_HIP_TRY(hipMemsetAsync(owner, 0, sizeof(uint32_t), ctx->stream));
        return STORM_HIP_OK;
    }
    const size_t scratch = lag_band_prune_scratch_words(n, lag, h_lo != nullptr, h_order != nullptr);
    LagR2Band b;
    if (int rc = lag_dosage_r2_band(ctx, m, n_samples, max_lag, lag, complete, scratch + (host ? n + (n + 3) / 4 : 0),
                                    "lag_dosage_prune: the band of r^2 and the adjacency masks", &b))
        return rc;
    uint32_t* const d_owner = host ? (owner ? b.tail + scratch : nullptr) : owner;
    uint8_t* const d_keep = host ? reinterpret_cast<uint8_t*>(b.tail + scratch + n) : keep;
    if (int rc = launch_lag_band_prune(ctx, who, reinterpret_cast<const float*>(b.band), lag, n, lag, min_r2, h_lo, h_hi, h_order,
                                       d_keep, d_owner, b.tail))
        return rc;
    if (!host) return STORM_HIP_OK;
    STORM_HIP_TRY(hipMemcpyAsync(keep, d_keep, n, hipMemcpyDeviceToHost, ctx->stream));
    if (owner) STORM_HIP_TRY(hipMemcpyAsync(owner, d_owner, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    STORM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return STORM_HIP_OK;
}

// ---- the sparse pair list: the band, then the kernels of storm_hip_lag_sparse.hip over it ----
// Tail, from the next 8-byte boundary (n x lag words can be odd): the forward masks, the blocks' sums, the rows' counts and the
// window bounds (h_lo / h_hi are HOST arrays of n entries in every form, or NULL; the launcher lays them out and sends them)
// and, for a host form, again from an 8-byte boundary, the n + 1 offsets and min(capacity, n x lag) staged (col, val) entries
// on their way back. All queued on ctx->stream; the host form alone waits: it reads the total, refuses a capacity below it
// (row_start and *n_pairs are valid then) and otherwise copies exactly `total` entries of col and val.
static int lag_dosage_corr_sparse(storm_hip_ctx_t* ctx, const char* who, const storm_hip_matrix_s* m, uint64_t n_samples,
                                  uint64_t max_lag, float min_r2, bool complete, const uint32_t* h_lo, const uint32_t* h_hi,
                                  uint64_t* row_start, uint32_t* col, float* val, uint64_t capacity, uint64_t* h_n_pairs, bool host) {
    uint64_t lag = 0;
    if (int rc = check_lag_dosage(who, m, row_start, max_lag, ~0ull, &lag)) return rc;
    if (int rc = check_samples(who, m, n_samples)) return rc;
    const uint64_t n = m->n_rows;
    if (int rc = check_lag_band_sparse(who, n, h_lo, h_hi, min_r2, col, val, capacity)) return rc;
    STORM_HIP_TRY(hipSetDevice(ctx->device));
    if (n < 2) {   // no pair: the offsets alone, n + 1 zeros; no band, no kernel
        if (host) {
            for (uint64_t i = 0; i <= n; ++i) row_start[i] = 0;
            if (h_n_pairs) *h_n_pairs = 0;
            return STORM_HIP_OK;
        }
        STORM_HIP_TRY(hipMemsetAsync(row_start, 0, (n + 1) * sizeof(uint64_t), ctx->stream));
        return STORM_HIP_OK;
    }
    const size_t pad = ((size_t)n * lag) & 1u;
    const size_t scratch = (lag_band_sparse_scratch_words(n, lag, h_lo != nullptr) + 1u) & ~(size_t)1u;
    const uint64_t staged = col ? std::min<uint64_t>(capacity, n * lag) : 0;
    LagR2Band b;
    if (int rc = lag_dosage_r2_band(ctx, m, n_samples, max_lag, lag, complete,
                                    pad + scratch + (host ? 2 * (size_t)(n + 1) + 2 * (size_t)staged : 0),
                                    "lag_dosage_corr_sparse: the band of r^2, the forward masks and the list", &b))
        return rc;
    uint32_t* const d_scratch = b.tail + pad;
    uint64_t* const d_row_start = host ? reinterpret_cast<uint64_t*>(d_scratch + scratch) : row_start;
    uint32_t* const d_col = host ? (col ? d_scratch + scratch + 2 * (size_t)(n + 1) : nullptr) : col;
    float* const d_val = host ? (col ? reinterpret_cast<float*>(d_col + staged) : nullptr) : val;
    if (int rc = launch_lag_band_sparse(ctx, reinterpret_cast<const float*>(b.band), lag, n, lag, min_r2, h_lo, h_hi, d_row_start,
                                        d_col, d_val, host ? staged : capacity, d_scratch))
        return rc;
    if (!host) return STORM_HIP_OK;
    STORM_HIP_TRY(hipMemcpyAsync(row_start, d_row_start, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    STORM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    const uint64_t total = row_start[n];
    if (h_n_pairs) *h_n_pairs = total;
    if (!col) return STORM_HIP_OK;
    if (total > capacity) {
        set_error("%s: %llu pairs are listed, capacity is %llu", who, (unsigned long long)total, (unsigned long long)capacity);
        return STORM_HIP_EINVAL;
    }
    if (total) {
        STORM_HIP_TRY(hipMemcpyAsync(col, d_col, total * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        STORM_HIP_TRY(hipMemcpyAsync(val, d_val, total * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        STORM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return STORM_HIP_OK;
}

// ---- the per-pair matrix calls: one body for the device form and the host form of each (pair_matrix_out, storm_hip_internal.h) ----
// A triangle of n x n entries, cleared in the band buffer (entries i >= j): `queued` where there is a pair. The device form
// returns below two rows without touching its matrix; the host form returns without rows and writes the one zero of a single row.
template <typename Queued>
static int dosage_triangle_out(storm_hip_ctx_t* ctx, const char* what, uint64_t n, void* out, uint64_t ld, bool host, Queued queued) {
    if (host ? n == 0 : n < 2) return STORM_HIP_OK;
    return pair_matrix_out(ctx, what, n, n, out, ld, host, true, true,
                           [&](uint32_t* d, uint64_t d_ld) { return n >= 2 ? queued(d, d_ld) : STORM_HIP_OK; });
}

static int pairw_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, uint32_t* out, uint64_t ld, bool host) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    if (int rc = check_dosage("pairw_dosage_matrix", m, out, ld)) return rc;
    return dosage_triangle_out(ctx, "pairw_dosage_matrix: the output", m->n_rows, out, ld, host,
                               [&](uint32_t* d, uint64_t d_ld) { return launch_pairw_dosage_matrix(ctx, m, d, d_ld); });
}

static int pairw_dosage_corr(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, int measure, uint64_t n_samples, bool complete,
                             float* out, uint64_t ld, bool host) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    const char* const who = complete ? "pairw_dosage_corr_complete" : "pairw_dosage_corr";
    if (int rc = check_dosage(who, m, out, ld)) return rc;
    if (int rc = check_corr(who, m, measure, n_samples)) return rc;
    return dosage_triangle_out(ctx, complete ? "pairw_dosage_corr_complete: the output" : "pairw_dosage_corr: the output", m->n_rows,
                               out, ld, host, [&](uint32_t* d, uint64_t d_ld) {
                                   return complete ? dosage_corr_complete_queued(ctx, m, measure, n_samples, d, d_ld)
                                                   : dosage_corr_queued(ctx, m, measure, n_samples, d, d_ld);
                               });
}

static int pairw_dosage_nobs(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, uint64_t n_samples, uint32_t* out, uint64_t ld,
                             bool host) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    if (int rc = check_dosage("pairw_dosage_nobs", m, out, ld)) return rc;
    if (int rc = check_samples("pairw_dosage_nobs", m, n_samples)) return rc;
    return dosage_triangle_out(ctx, "pairw_dosage_nobs: the output", m->n_rows, out, ld, host,
                               [&](uint32_t* d, uint64_t d_ld) { return dosage_nobs_queued(ctx, m, n_samples, d, d_ld); });
}

// (a rectangle: every entry is written, nothing to clear)
static int square_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, uint32_t* out,
                                uint64_t ld, bool host) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    if (int rc = check_square("square_dosage_matrix", a, b, out, ld)) return rc;
    if (a->n_rows == 0 || b->n_rows == 0) return STORM_HIP_OK;
    return pair_matrix_out(ctx, "square_dosage_matrix: the output", a->n_rows, b->n_rows, out, ld, host, false, true,
                           [&](uint32_t* d, uint64_t d_ld) { return launch_square_dosage_matrix(ctx, a, b, d, d_ld); });
}

// r / r^2 (complete: over the samples both rows have) and N of the rectangle: every entry is written in both forms
static int square_dosage_corr(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, int measure,
                              uint64_t n_samples, bool complete, float* out, uint64_t ld, bool host) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    const char* const who = complete ? "square_dosage_corr_complete" : "square_dosage_corr";
    if (int rc = check_square(who, a, b, out, ld)) return rc;
    if (int rc = check_corr(who, a, measure, n_samples)) return rc;
    if (a->n_rows == 0 || b->n_rows == 0) return STORM_HIP_OK;
    return pair_matrix_out(ctx, complete ? "square_dosage_corr_complete: the output" : "square_dosage_corr: the output", a->n_rows,
                           b->n_rows, out, ld, host, false, true, [&](uint32_t* d, uint64_t d_ld) {
                               return complete ? square_dosage_corr_complete_queued(ctx, a, b, measure, n_samples, d, d_ld)
                                               : square_dosage_corr_queued(ctx, a, b, measure, n_samples, d, d_ld);
                           });
}

static int square_dosage_nobs(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, uint64_t n_samples,
                              uint32_t* out, uint64_t ld, bool host) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    if (int rc = check_square("square_dosage_nobs", a, b, out, ld)) return rc;
    if (int rc = check_samples("square_dosage_nobs", a, n_samples)) return rc;
    if (a->n_rows == 0 || b->n_rows == 0) return STORM_HIP_OK;
    return pair_matrix_out(ctx, "square_dosage_nobs: the output", a->n_rows, b->n_rows, out, ld, host, false, true,
                           [&](uint32_t* d, uint64_t d_ld) { return square_dosage_nobs_queued(ctx, a, b, n_samples, d, d_ld); });
}

// The lag layout, n x L, cleared in the band buffer (the lower-right corner): both forms return below two rows. The dot
// products alone take a band of rows in their device form (the host form: every row).
static int pairw_lag_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, uint64_t max_lag, uint64_t row0,
                                   uint64_t n_band_rows, uint32_t* out, uint64_t ld, bool host) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    uint64_t lag = 0;
    if (int rc = check_lag_dosage("pairw_lag_dosage_matrix", m, out, max_lag, ld, &lag)) return rc;
    if (n_band_rows == ~0ull && row0 <= m->n_rows) n_band_rows = m->n_rows - row0;
    if (row0 > m->n_rows || n_band_rows > m->n_rows - row0) {
        set_error("pairw_lag_dosage_matrix: a band outside the rows");
        return STORM_HIP_EINVAL;
    }
    if (m->n_rows < 2 || n_band_rows == 0) return STORM_HIP_OK;
    return pair_matrix_out(ctx, "pairw_lag_dosage_matrix: the output", n_band_rows, lag, out, ld, host, true, true,
                           [&](uint32_t* d, uint64_t d_ld) {
                               return launch_pairw_lag_dosage_matrix(ctx, m, max_lag, row0, n_band_rows, d, d_ld);
                           });
}

static int pairw_lag_dosage_corr(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, int measure, uint64_t n_samples, uint64_t max_lag,
                                 bool complete, float* out, uint64_t ld, bool host) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    const char* const who = complete ? "pairw_lag_dosage_corr_complete" : "pairw_lag_dosage_corr";
    uint64_t lag = 0;
    if (int rc = check_lag_dosage(who, m, out, max_lag, ld, &lag)) return rc;
    if (int rc = check_corr(who, m, measure, n_samples)) return rc;
    if (m->n_rows < 2) return STORM_HIP_OK;
    return pair_matrix_out(ctx, complete ? "pairw_lag_dosage_corr_complete: the output" : "pairw_lag_dosage_corr: the output",
                           m->n_rows, lag, out, ld, host, true, true, [&](uint32_t* d, uint64_t d_ld) {
                               return complete ? lag_dosage_corr_complete_queued(ctx, m, measure, n_samples, max_lag, d, d_ld)
                                               : lag_dosage_corr_queued(ctx, m, measure, n_samples, max_lag, d, d_ld);
                           });
}

static int pairw_lag_dosage_nobs(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, uint64_t n_samples, uint64_t max_lag,
                                 uint32_t* out, uint64_t ld, bool host) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    uint64_t lag = 0;
    if (int rc = check_lag_dosage("pairw_lag_dosage_nobs", m, out, max_lag, ld, &lag)) return rc;
    if (int rc = check_samples("pairw_lag_dosage_nobs", m, n_samples)) return rc;
    if (m->n_rows < 2) return STORM_HIP_OK;
    return pair_matrix_out(ctx, "pairw_lag_dosage_nobs: the output", m->n_rows, lag, out, ld, host, true, true,
                           [&](uint32_t* d, uint64_t d_ld) { return lag_dosage_nobs_queued(ctx, m, n_samples, max_lag, d, d_ld); });
}

}  // namespace storm

using namespace storm;

extern "C" {

int storm_hip_dosage_row_sums(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint32_t* h_sum, uint32_t* h_sum_sq) {
    return guarded("storm_hip_dosage_row_sums", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        if (!m || !h_sum || !h_sum_sq) {
            set_error("dosage_row_sums: NULL argument");
            return STORM_HIP_EINVAL;
        }
        if ((uint64_t)m->n_words * 32u > kDosageMaxSamples) {
            set_error("dosage_row_sums: rows of %u words hold more than 2^24 values", m->n_words);
            return STORM_HIP_EINVAL;
        }
        const uint64_t n = m->n_rows;
        if (n == 0) return STORM_HIP_OK;
        STORM_HIP_TRY(hipSetDevice(ctx->device));
        if (int rc = dosage_sums_queued(ctx, m)) return rc;
        STORM_HIP_TRY(hipMemcpyAsync(h_sum, ctx->d_counts.d, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        STORM_HIP_TRY(hipMemcpyAsync(h_sum_sq, ctx->d_counts.d + n, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        STORM_HIP_TRY(hipStreamSynchronize(ctx->stream));
        return STORM_HIP_OK;
    });
}

int storm_hip_pairw_dosage_matrix_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint32_t* d_out, uint64_t ld) {
    return guarded("storm_hip_pairw_dosage_matrix_device", [&] { return pairw_dosage_matrix(ctx, m, d_out, ld, false); });
}

int storm_hip_pairw_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint32_t* h_out, uint64_t ld) {
    return guarded("storm_hip_pairw_dosage_matrix", [&] { return pairw_dosage_matrix(ctx, m, h_out, ld, true); });
}

int storm_hip_pairw_dosage_corr_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                       float* d_out, uint64_t ld) {
    return guarded("storm_hip_pairw_dosage_corr_device",
                   [&] { return pairw_dosage_corr(ctx, m, measure, n_samples, false, d_out, ld, false); });
}

int storm_hip_pairw_dosage_corr(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples, float* h_out,
                                uint64_t ld) {
    return guarded("storm_hip_pairw_dosage_corr",
                   [&] { return pairw_dosage_corr(ctx, m, measure, n_samples, false, h_out, ld, true); });
}

int storm_hip_square_dosage_matrix_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,
                                          uint32_t* d_out, uint64_t ld) {
    return guarded("storm_hip_square_dosage_matrix_device", [&] { return square_dosage_matrix(ctx, a, b, d_out, ld, false); });
}

int storm_hip_square_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, uint32_t* h_out,
                                   uint64_t ld) {
    return guarded("storm_hip_square_dosage_matrix", [&] { return square_dosage_matrix(ctx, a, b, h_out, ld, true); });
}

int storm_hip_square_dosage_corr_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int measure,
                                        uint64_t n_samples, float* d_out, uint64_t ld) {
    return guarded("storm_hip_square_dosage_corr_device",
                   [&] { return square_dosage_corr(ctx, a, b, measure, n_samples, false, d_out, ld, false); });
}

int storm_hip_square_dosage_corr(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int measure,
                                 uint64_t n_samples, float* h_out, uint64_t ld) {
    return guarded("storm_hip_square_dosage_corr",
                   [&] { return square_dosage_corr(ctx, a, b, measure, n_samples, false, h_out, ld, true); });
}

int storm_hip_square_dosage_nobs_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,
                                        uint64_t n_samples, uint32_t* d_out, uint64_t ld) {
    return guarded("storm_hip_square_dosage_nobs_device", [&] { return square_dosage_nobs(ctx, a, b, n_samples, d_out, ld, false); });
}

int storm_hip_square_dosage_nobs(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, uint64_t n_samples,
                                 uint32_t* h_out, uint64_t ld) {
    return guarded("storm_hip_square_dosage_nobs", [&] { return square_dosage_nobs(ctx, a, b, n_samples, h_out, ld, true); });
}

int storm_hip_square_dosage_corr_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,
                                                 int measure, uint64_t n_samples, float* d_out, uint64_t ld) {
    return guarded("storm_hip_square_dosage_corr_complete_device",
                   [&] { return square_dosage_corr(ctx, a, b, measure, n_samples, true, d_out, ld, false); });
}

int storm_hip_square_dosage_corr_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int measure,
                                          uint64_t n_samples, float* h_out, uint64_t ld) {
    return guarded("storm_hip_square_dosage_corr_complete",
                   [&] { return square_dosage_corr(ctx, a, b, measure, n_samples, true, h_out, ld, true); });
}

int storm_hip_dosage_row_missing(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint32_t* h_missing) {
    return guarded("storm_hip_dosage_row_missing", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        if (int rc = check_dosage("dosage_row_missing", m, h_missing, m ? m->n_rows : 0)) return rc;
        if (int rc = check_samples("dosage_row_missing", m, n_samples)) return rc;
        const uint64_t n = m->n_rows;
        if (n == 0) return STORM_HIP_OK;
        STORM_HIP_TRY(hipSetDevice(ctx->device));
        if (int rc = ctx->d_counts.ensure(n * sizeof(uint32_t), "dosage_row_missing: the row scratch")) return rc;
        hipLaunchKernelGGL(dosage_row_missing_kernel, dim3((uint32_t)((n + kWaves - 1) / kWaves)), dim3(kThreads), 0, ctx->stream, m->d,
                           m->stride_words, n, m->n_words, n_samples, ctx->d_counts.d);
        STORM_HIP_TRY(hipGetLastError());
        STORM_HIP_TRY(hipMemcpyAsync(h_missing, ctx->d_counts.d, n * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        STORM_HIP_TRY(hipStreamSynchronize(ctx->stream));
        return STORM_HIP_OK;
    });
}

int storm_hip_pairw_dosage_nobs_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint32_t* d_out,
                                       uint64_t ld) {
    return guarded("storm_hip_pairw_dosage_nobs_device", [&] { return pairw_dosage_nobs(ctx, m, n_samples, d_out, ld, false); });
}

int storm_hip_pairw_dosage_nobs(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint32_t* h_out, uint64_t ld) {
    return guarded("storm_hip_pairw_dosage_nobs", [&] { return pairw_dosage_nobs(ctx, m, n_samples, h_out, ld, true); });
}

int storm_hip_pairw_dosage_corr_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                                float* d_out, uint64_t ld) {
    return guarded("storm_hip_pairw_dosage_corr_complete_device",
                   [&] { return pairw_dosage_corr(ctx, m, measure, n_samples, true, d_out, ld, false); });
}

int storm_hip_pairw_dosage_corr_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                         float* h_out, uint64_t ld) {
    return guarded("storm_hip_pairw_dosage_corr_complete",
                   [&] { return pairw_dosage_corr(ctx, m, measure, n_samples, true, h_out, ld, true); });
}

// ---- the lag layout ----
int storm_hip_pairw_lag_dosage_matrix_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t max_lag, uint64_t row0,
                                             uint64_t n_band_rows, uint32_t* d_out, uint64_t ld) {
    return guarded("storm_hip_pairw_lag_dosage_matrix_device",
                   [&] { return pairw_lag_dosage_matrix(ctx, m, max_lag, row0, n_band_rows, d_out, ld, false); });
}

int storm_hip_pairw_lag_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t max_lag, uint32_t* h_out,
                                      uint64_t ld) {
    return guarded("storm_hip_pairw_lag_dosage_matrix",
                   [&] { return pairw_lag_dosage_matrix(ctx, m, max_lag, 0, ~0ull, h_out, ld, true); });
}

int storm_hip_dosage_finish_lag_device(storm_hip_ctx_t* ctx, void* d_io, uint64_t ld, uint64_t n_rows, uint64_t row0,
                                       uint64_t n_band_rows, uint64_t max_lag, const uint32_t* d_sum, const uint32_t* d_sum_sq,
                                       int measure, uint64_t n_samples) {
    return guarded("storm_hip_dosage_finish_lag_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        if (int rc = launch_dosage_finish_lag(ctx, d_io, ld, n_rows, row0, n_band_rows, max_lag, d_sum, d_sum_sq, measure, n_samples))
            return rc;
        // (alone on a caller's matrix: a report of its own, as storm_hip_similarity_finish_lag_device; nothing launched: as it was)
        if (n_rows >= 2 && n_band_rows != 0 && row0 < n_rows) {
            memset(ctx->pass_report, 0, sizeof(ctx->pass_report));
            ctx->pass_report[0] = STORM_HIP_RAN_SIMILARITY;
        }
        return STORM_HIP_OK;
    });
}

int storm_hip_pairw_lag_dosage_corr_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                           uint64_t max_lag, float* d_out, uint64_t ld) {
    return guarded("storm_hip_pairw_lag_dosage_corr_device",
                   [&] { return pairw_lag_dosage_corr(ctx, m, measure, n_samples, max_lag, false, d_out, ld, false); });
}

int storm_hip_pairw_lag_dosage_corr(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                    uint64_t max_lag, float* h_out, uint64_t ld) {
    return guarded("storm_hip_pairw_lag_dosage_corr",
                   [&] { return pairw_lag_dosage_corr(ctx, m, measure, n_samples, max_lag, false, h_out, ld, true); });
}

int storm_hip_pairw_lag_dosage_nobs_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                           uint32_t* d_out, uint64_t ld) {
    return guarded("storm_hip_pairw_lag_dosage_nobs_device",
                   [&] { return pairw_lag_dosage_nobs(ctx, m, n_samples, max_lag, d_out, ld, false); });
}

int storm_hip_pairw_lag_dosage_nobs(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                    uint32_t* h_out, uint64_t ld) {
    return guarded("storm_hip_pairw_lag_dosage_nobs",
                   [&] { return pairw_lag_dosage_nobs(ctx, m, n_samples, max_lag, h_out, ld, true); });
}

int storm_hip_pairw_lag_dosage_corr_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure,
                                                    uint64_t n_samples, uint64_t max_lag, float* d_out, uint64_t ld) {
    return guarded("storm_hip_pairw_lag_dosage_corr_complete_device",
                   [&] { return pairw_lag_dosage_corr(ctx, m, measure, n_samples, max_lag, true, d_out, ld, false); });
}

int storm_hip_pairw_lag_dosage_corr_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                             uint64_t max_lag, float* h_out, uint64_t ld) {
    return guarded("storm_hip_pairw_lag_dosage_corr_complete",
                   [&] { return pairw_lag_dosage_corr(ctx, m, measure, n_samples, max_lag, true, h_out, ld, true); });
}

int storm_hip_lag_dosage_ldscore_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                        uint64_t max_lag, float* d_score, uint32_t* d_n_pairs) {
    return guarded("storm_hip_lag_dosage_ldscore_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return lag_dosage_ldscore(ctx, "lag_dosage_ldscore", m, stat, n_samples, max_lag, false, d_score, d_n_pairs, false);
    });
}

int storm_hip_lag_dosage_ldscore(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples, uint64_t max_lag,
                                 float* h_score, uint32_t* h_n_pairs) {
    return guarded("storm_hip_lag_dosage_ldscore", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return lag_dosage_ldscore(ctx, "lag_dosage_ldscore", m, stat, n_samples, max_lag, false, h_score, h_n_pairs, true);
    });
}

int storm_hip_lag_dosage_ldscore_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                                 uint64_t max_lag, float* d_score, uint32_t* d_n_pairs) {
    return guarded("storm_hip_lag_dosage_ldscore_complete_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return lag_dosage_ldscore(ctx, "lag_dosage_ldscore_complete", m, stat, n_samples, max_lag, true, d_score, d_n_pairs, false);
    });
}

int storm_hip_lag_dosage_ldscore_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                          uint64_t max_lag, float* h_score, uint32_t* h_n_pairs) {
    return guarded("storm_hip_lag_dosage_ldscore_complete", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return lag_dosage_ldscore(ctx, "lag_dosage_ldscore_complete", m, stat, n_samples, max_lag, true, h_score, h_n_pairs, true);
    });
}

int storm_hip_lag_dosage_ldscore_annot_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                              uint64_t max_lag, const uint32_t* h_lo, const uint32_t* h_hi, const float* d_annot,
                                              uint64_t annot_ld, uint64_t n_annot, float* d_score, uint64_t score_ld,
                                              uint32_t* d_n_pairs) {
    return guarded("storm_hip_lag_dosage_ldscore_annot_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return lag_dosage_ldscore_annot(ctx, "lag_dosage_ldscore_annot", m, stat, n_samples, max_lag, false, h_lo, h_hi, d_annot,
                                        annot_ld, n_annot, d_score, score_ld, d_n_pairs, false);
    });
}

int storm_hip_lag_dosage_ldscore_annot(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                       uint64_t max_lag, const uint32_t* h_lo, const uint32_t* h_hi, const float* h_annot,
                                       uint64_t annot_ld, uint64_t n_annot, float* h_score, uint64_t score_ld, uint32_t* h_n_pairs) {
    return guarded("storm_hip_lag_dosage_ldscore_annot", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return lag_dosage_ldscore_annot(ctx, "lag_dosage_ldscore_annot", m, stat, n_samples, max_lag, false, h_lo, h_hi, h_annot,
                                        annot_ld, n_annot, h_score, score_ld, h_n_pairs, true);
    });
}

int storm_hip_lag_dosage_ldscore_annot_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat,
                                                       uint64_t n_samples, uint64_t max_lag, const uint32_t* h_lo,
                                                       const uint32_t* h_hi, const float* d_annot, uint64_t annot_ld,
                                                       uint64_t n_annot, float* d_score, uint64_t score_ld, uint32_t* d_n_pairs) {
    return guarded("storm_hip_lag_dosage_ldscore_annot_complete_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return lag_dosage_ldscore_annot(ctx, "lag_dosage_ldscore_annot_complete", m, stat, n_samples, max_lag, true, h_lo, h_hi,
                                        d_annot, annot_ld, n_annot, d_score, score_ld, d_n_pairs, false);
    });
}

int storm_hip_lag_dosage_ldscore_annot_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                                uint64_t max_lag, const uint32_t* h_lo, const uint32_t* h_hi, const float* h_annot,
                                                uint64_t annot_ld, uint64_t n_annot, float* h_score, uint64_t score_ld,
                                                uint32_t* h_n_pairs) {
    return guarded("storm_hip_lag_dosage_ldscore_annot_complete", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return lag_dosage_ldscore_annot(ctx, "lag_dosage_ldscore_annot_complete", m, stat, n_samples, max_lag, true, h_lo, h_hi,
                                        h_annot, annot_ld, n_annot, h_score, score_ld, h_n_pairs, true);
    });
}

int storm_hip_lag_dosage_prune_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                      float min_r2, const uint32_t* h_lo, const uint32_t* h_hi, const uint32_t* h_order,
                                      uint8_t* d_keep, uint32_t* d_owner) {
    return guarded("storm_hip_lag_dosage_prune_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return lag_dosage_prune(ctx, "lag_dosage_prune", m, n_samples, max_lag, min_r2, false, h_lo, h_hi, h_order, d_keep, d_owner,
                                false);
    });
}

int storm_hip_lag_dosage_prune(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag, float min_r2,
                               const uint32_t* h_lo, const uint32_t* h_hi, const uint32_t* h_order, uint8_t* h_keep,
                               uint32_t* h_owner) {
    return guarded("storm_hip_lag_dosage_prune", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return lag_dosage_prune(ctx, "lag_dosage_prune", m, n_samples, max_lag, min_r2, false, h_lo, h_hi, h_order, h_keep, h_owner,
                                true);
    });
}

int storm_hip_lag_dosage_prune_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples,
                                               uint64_t max_lag, float min_r2, const uint32_t* h_lo, const uint32_t* h_hi,
                                               const uint32_t* h_order, uint8_t* d_keep, uint32_t* d_owner) {
    return guarded("storm_hip_lag_dosage_prune_complete_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return lag_dosage_prune(ctx, "lag_dosage_prune_complete", m, n_samples, max_lag, min_r2, true, h_lo, h_hi, h_order, d_keep,
                                d_owner, false);
    });
}

int storm_hip_lag_dosage_prune_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                        float min_r2, const uint32_t* h_lo, const uint32_t* h_hi, const uint32_t* h_order,
                                        uint8_t* h_keep, uint32_t* h_owner) {
    return guarded("storm_hip_lag_dosage_prune_complete", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return lag_dosage_prune(ctx, "lag_dosage_prune_complete", m, n_samples, max_lag, min_r2, true, h_lo, h_hi, h_order, h_keep,
                                h_owner, true);
    });
}

int storm_hip_lag_dosage_corr_sparse_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                            float min_r2, const uint32_t* h_lo, const uint32_t* h_hi, uint64_t* d_row_start,
                                            uint32_t* d_col, float* d_val, uint64_t capacity) {
    return guarded("storm_hip_lag_dosage_corr_sparse_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return lag_dosage_corr_sparse(ctx, "lag_dosage_corr_sparse", m, n_samples, max_lag, min_r2, false, h_lo, h_hi, d_row_start,
                                      d_col, d_val, capacity, nullptr, false);
    });
}

int storm_hip_lag_dosage_corr_sparse(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                     float min_r2, const uint32_t* h_lo, const uint32_t* h_hi, uint64_t* h_row_start, uint32_t* h_col,
                                     float* h_val, uint64_t capacity, uint64_t* h_n_pairs) {
    return guarded("storm_hip_lag_dosage_corr_sparse", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return lag_dosage_corr_sparse(ctx, "lag_dosage_corr_sparse", m, n_samples, max_lag, min_r2, false, h_lo, h_hi, h_row_start,
                                      h_col, h_val, capacity, h_n_pairs, true);
    });
}

int storm_hip_lag_dosage_corr_sparse_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples,
                                                     uint64_t max_lag, float min_r2, const uint32_t* h_lo, const uint32_t* h_hi,
                                                     uint64_t* d_row_start, uint32_t* d_col, float* d_val, uint64_t capacity) {
    return guarded("storm_hip_lag_dosage_corr_sparse_complete_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return lag_dosage_corr_sparse(ctx, "lag_dosage_corr_sparse_complete", m, n_samples, max_lag, min_r2, true, h_lo, h_hi,
                                      d_row_start, d_col, d_val, capacity, nullptr, false);
    });
}

int storm_hip_lag_dosage_corr_sparse_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                              float min_r2, const uint32_t* h_lo, const uint32_t* h_hi, uint64_t* h_row_start,
                                              uint32_t* h_col, float* h_val, uint64_t capacity, uint64_t* h_n_pairs) {
    return guarded("storm_hip_lag_dosage_corr_sparse_complete", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return lag_dosage_corr_sparse(ctx, "lag_dosage_corr_sparse_complete", m, n_samples, max_lag, min_r2, true, h_lo, h_hi,
                                      h_row_start, h_col, h_val, capacity, h_n_pairs, true);
    });
}

}  // extern "C"
