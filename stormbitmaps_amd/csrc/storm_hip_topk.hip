// storm_hip_topk.hip — for each row its k best columns, selected where the counts lie: topk_rows_kernel reads a complete
// panel of intersection counts (uint32, what the matrix-output paths write), forms every entry's score (the AND count
// itself, or the similarity measure of storm_similarity_math.h: bit-identical to the similarity calls) and keeps the k
// largest keys of storm_topk_math.h per row: value descending, then column ascending. n x k entries leave the device
// instead of n x n. The count panel is read once, 4 bytes per entry, and never written.
//
// The forms above the primitive run in row panels: the AND-count rectangle (panel rows x all columns) into the context's
// band buffer through launch_square_matrix with the kernel choice as it is, then the selection over that panel.
//
// The kernel is a template over a scorer — what turns a panel entry into its value. Besides the bit form there are two for
// rows of 2-bit values (dosages): dot products with the rows' sums into dosage_corr_bits, and the six sums of a pair with
// missing genotypes into dosage_corr_complete_bits (storm_dosage_math.h: the bits of the dosage finish kernels). Their forms
// above the primitive (storm_hip_pairw_dosage_topk, storm_hip_square_dosage_topk and the _complete forms) run in row panels of
// integer sums from K2h in its dosage form; no float matrix is formed ("Top-k rows, dosage form").
#include "storm_hip_internal.h"
#include "storm_similarity_math.h"
#include "storm_dosage_math.h"
#include "storm_topk_math.h"

namespace storm {

constexpr int kTopkThreads = 256;                                // 4 waves: one workgroup per panel row
constexpr int kTopkBest = STORM_HIP_TOPK_MAX;                    // keys [0, 128) of the LDS array: the best so far, descending
constexpr int kTopkKeys = 2048;                                  // the LDS array: best + staging, 16 KiB
constexpr int kTopkStaging = kTopkKeys - kTopkBest;              // 1920 staged keys at most
constexpr int kTopkStep = kTopkThreads * 4;                      // entries of one sweep step: 4 per lane
static_assert(kTopkStep <= kTopkStaging, "an empty staging area takes one whole step");
static_assert((kTopkKeys & (kTopkKeys - 1)) == 0 && kTopkBest <= 256, "the sort runs over powers of two from 256 up");

// a lane's 4 entries of the row from column c0: one 128-bit load where all 4 exist and `vec`, else entry by entry
// (columns at or beyond n_cols are not read)
__device__ __forceinline__ uint4 topk_load4(const uint32_t* __restrict__ row, uint64_t c0, uint64_t n_cols, int vec) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (vec && c0 + 4 <= n_cols) {
        v = *reinterpret_cast<const uint4*>(row + c0);
    } else {
        if (c0 < n_cols) v.x = row[c0];
        if (c0 + 1 < n_cols) v.y = row[c0 + 1];
        if (c0 + 2 < n_cols) v.z = row[c0 + 2];
        if (c0 + 3 < n_cols) v.w = row[c0 + 3];
    }
    return v;
}

// best U staging -> the array sorted descending (bitonic, over the power of two that holds them; 0 = no entry sorts
// last). Entered by the whole workgroup behind a barrier that ends the appends; ends behind a barrier.
__device__ __forceinline__ void topk_flush(uint64_t* s_keys, uint32_t staged) {
    const uint32_t n = kTopkBest + staged;
    uint32_t N = 256u;
    while (N < n) N <<= 1;
    for (uint32_t t = n + threadIdx.x; t < N; t += kTopkThreads) s_keys[t] = 0ull;
    __syncthreads();
    for (uint32_t size = 2u; size <= N; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0u; stride >>= 1) {
            for (uint32_t t = threadIdx.x; t < N / 2u; t += kTopkThreads) {
                const uint32_t i = 2u * t - (t & (stride - 1u)), j = i + stride;
                const uint64_t x = s_keys[i], y = s_keys[j];
                const bool descending = (i & size) == 0u;
                if (descending ? x < y : x > y) {
                    s_keys[i] = y;
                    s_keys[j] = x;
                }
            }
            __syncthreads();
        }
    }
}

// ---- the scorers: what topk_rows_kernel forms an entry's value from. A scorer is built per workgroup from its Args and the
// panel row r (what is uniform per row lies in it), `load` fetches a lane's 4 entries from column c0 (columns at or beyond
// n_cols are not read), `bits` turns entry e of them, column j, into the value's 32 bits; is_count: the value is an unsigned
// integer and every entry a candidate, else float bits with kTopkNaN no candidate. ----
__device__ __forceinline__ uint32_t topk_word(const uint4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// intersection counts of bit rows: the AND count itself or a measure of storm_similarity_math.h
struct TopkBitScorer {
    struct Args {
        const uint32_t *counts, *counts_rows, *counts_cols;
        uint64_t ld, n_bits;
        int score, vec;
    };
    typedef uint4 Raw;
    const uint32_t *row, *counts_cols;
    uint64_t n_bits;
    uint32_t a;
    int score, vec;
    bool is_count;
    __device__ __forceinline__ TopkBitScorer(const Args& g, uint64_t r)
        : row(g.counts + r * g.ld), counts_cols(g.counts_cols), n_bits(g.n_bits), a(g.counts_rows[r]), score(g.score), vec(g.vec),
          is_count(g.score == STORM_HIP_TOPK_COUNT) {}
    __device__ __forceinline__ Raw load(uint64_t c0, uint64_t n_cols) const { return topk_load4(row, c0, n_cols, vec); }
    __device__ __forceinline__ uint32_t bits(const Raw& v, int e, uint64_t j) const {
        const uint32_t c = topk_word(v, e);
        return is_count ? c : similarity_bits(c, a, counts_cols[j], score, n_bits);
    }
};

// dot products of dosage rows, 3 an ordinary value: the dot product itself or dosage_corr_bits from the rows' sums
struct TopkDosageScorer {
    struct Args {
        const uint32_t *dots, *a_sum, *a_sq, *b_sum, *b_sq;
        uint64_t ld, n_samples;
        int score, vec;
    };
    typedef uint4 Raw;
    const uint32_t *row, *b_sum, *b_sq;
    uint64_t n_samples;
    uint32_t s_i, q_i;
    int score, vec;
    bool is_count;
    __device__ __forceinline__ TopkDosageScorer(const Args& g, uint64_t r)
        : row(g.dots + r * g.ld), b_sum(g.b_sum), b_sq(g.b_sq), n_samples(g.n_samples), s_i(g.a_sum[r]), q_i(g.a_sq[r]),
          score(g.score), vec(g.vec), is_count(g.score == STORM_HIP_DOSAGE_TOPK_DOT) {}
    __device__ __forceinline__ Raw load(uint64_t c0, uint64_t n_cols) const { return topk_load4(row, c0, n_cols, vec); }
    __device__ __forceinline__ uint32_t bits(const Raw& v, int e, uint64_t j) const {
        const uint32_t P = topk_word(v, e);
        return is_count ? P : dosage_corr_bits(P, s_i, q_i, b_sum[j], b_sq[j], score, n_samples);
    }
};

// dosage rows with missing genotypes: the six sums of an entry from the panel's planes as dosage_square_complete_finish_kernel
// reads them — P (pitch ld), `ghm` (pitch ld_ghm: sx at row r, H_a M_b at row h_row0 + r) and `mghm` (pitch ld_mghm: sy at
// column j, M_a H_b at h_col0 + j, N at m_col0 + j) — into dosage_corr_complete_bits. vec: every plane's base 16-byte
// aligned, every pitch and both column offsets multiples of 4. Never a count.
struct TopkDosageCompleteScorer {
    struct Args {
        const uint32_t *P, *ghm, *mghm;
        uint64_t ld, ld_ghm, h_row0, ld_mghm, h_col0, m_col0;
        int score, vec;
    };
    struct Raw {
        uint4 P, sx, hx, sy, hy, N;
    };
    const uint32_t *P, *sx, *hx, *sy, *hy, *N;
    int score, vec;
    static constexpr bool is_count = false;
    __device__ __forceinline__ TopkDosageCompleteScorer(const Args& g, uint64_t r)
        : P(g.P + r * g.ld), sx(g.ghm + r * g.ld_ghm), hx(g.ghm + (g.h_row0 + r) * g.ld_ghm), sy(g.mghm + r * g.ld_mghm),
          hy(sy + g.h_col0), N(sy + g.m_col0), score(g.score), vec(g.vec) {}
    __device__ __forceinline__ Raw load(uint64_t c0, uint64_t n_cols) const {
        return {topk_load4(P, c0, n_cols, vec),  topk_load4(sx, c0, n_cols, vec), topk_load4(hx, c0, n_cols, vec),
                topk_load4(sy, c0, n_cols, vec), topk_load4(hy, c0, n_cols, vec), topk_load4(N, c0, n_cols, vec)};
    }
    __device__ __forceinline__ uint32_t bits(const Raw& v, int e, uint64_t) const {
        const uint32_t x = topk_word(v.sx, e), y = topk_word(v.sy, e);
        return dosage_corr_complete_bits(topk_word(v.P, e), topk_word(v.N, e), x, y, x + 2u * topk_word(v.hx, e),
                                         y + 2u * topk_word(v.hy, e), score);
    }
};

// Grid: one workgroup per row of the panel. The lanes sweep the row kTopkStep entries at a time (the next step's load
// leaves before this step's arithmetic); a lane appends a key to the staging area only when it beats the threshold, the
// k-th best key of the last sort (0 before the first). Slots come from an LDS counter per step — three of them in
// rotation, so that the step's total is read behind ONE barrier while the lanes ahead already count the next step in
// another word — and the workgroup sorts best U staging whenever the next step could overflow the staging area. Keys
// are unique within a row, so what is kept does not depend on the order the lanes arrive in. No global atomics.
// One body for the three scorers above (resources per instantiation: DESIGN.md §4, "Top-k rows, dosage form").
template <class Scorer>
__global__ __launch_bounds__(kTopkThreads) void topk_rows_kernel(const typename Scorer::Args args, uint64_t n_cols, uint64_t skip0,
                                                                 uint32_t k, uint32_t* __restrict__ idx, uint32_t* __restrict__ val,
                                                                 uint64_t ld_k) {
    __shared__ uint64_t s_keys[kTopkKeys];
    __shared__ uint32_t s_step[3];
    const uint64_t r = blockIdx.x;
    const Scorer scorer(args, r);
    const bool is_count = scorer.is_count;
    const uint64_t skip = (skip0 == ~0ull || skip0 > ~0ull - r) ? ~0ull : skip0 + r;   // (no column is ~0: n_cols < 2^32)
    if (threadIdx.x < kTopkBest) s_keys[threadIdx.x] = 0ull;
    if (threadIdx.x < 3) s_step[threadIdx.x] = 0u;
    __syncthreads();
    uint64_t threshold = 0ull;
    uint32_t staged = 0u, step = 0u;   // uniform
    typename Scorer::Raw cur = scorer.load((uint64_t)threadIdx.x * 4u, n_cols);
    for (uint64_t base = 0; base < n_cols; base += kTopkStep) {
        const uint64_t c0 = base + (uint64_t)threadIdx.x * 4u;
        typename Scorer::Raw nxt = {};
        if (base + kTopkStep < n_cols) nxt = scorer.load(c0 + kTopkStep, n_cols);
        uint32_t* const counter = &s_step[step % 3u];
        if (threadIdx.x == 0) s_step[(step + 1u) % 3u] = 0u;   // the next step's: last read two barriers ago
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint64_t j = c0 + e;
            if (j >= n_cols || j == skip) continue;
            const uint32_t bits = scorer.bits(cur, e, j);
            if (!is_count && !topk_is_candidate(bits)) continue;
            const uint64_t key = topk_key(bits, (uint32_t)j, is_count);
            if (key > threshold) s_keys[kTopkBest + staged + atomicAdd(counter, 1u)] = key;
        }
        __syncthreads();
        staged += *counter;
        ++step;
        if (staged + kTopkStep > kTopkStaging) {
            topk_flush(s_keys, staged);
            staged = 0u;
            threshold = s_keys[k - 1u];
        }
        cur = nxt;
    }
    if (staged) topk_flush(s_keys, staged);
    if (threadIdx.x < k) {
        const uint64_t key = s_keys[threadIdx.x];
        idx[r * ld_k + threadIdx.x] = key ? topk_key_index(key) : kTopkNoIndex;
        val[r * ld_k + threadIdx.x] = key ? topk_key_value(key, is_count) : (is_count ? 0u : kTopkNaN);
    }
}

// what every top-k call refuses alike, before anything is launched: k and the outputs' pitch; the bit forms' score and n_bits
static int check_topk_k(const char* who, uint64_t k, uint64_t ld_k) {
    if (k == 0 || k > STORM_HIP_TOPK_MAX || ld_k < k) {
        set_error("%s: k %llu is not in [1, %d], or ld_k %llu < k", who, (unsigned long long)k, STORM_HIP_TOPK_MAX,
                  (unsigned long long)ld_k);
        return STORM_HIP_EINVAL;
    }
    return STORM_HIP_OK;
}
static int check_topk(const char* who, int score, uint64_t n_bits, uint64_t k, uint64_t ld_k) {
    if (score < STORM_HIP_SIM_JACCARD || score > STORM_HIP_TOPK_COUNT) {
        set_error("%s: unknown score %d (0 Jaccard, 1 cosine, 2 LD D, 3 LD r^2, 4 the AND count)", who, score);
        return STORM_HIP_EINVAL;
    }
    if (n_bits == 0 || n_bits > (1ull << 32)) {
        set_error("%s: n_bits %llu is not in [1, 2^32]", who, (unsigned long long)n_bits);
        return STORM_HIP_EINVAL;
    }
    return check_topk_k(who, k, ld_k);
}

// topk_rows_kernel over a complete count panel in device memory, asynchronous (the checks of storm_hip_topk_rows_device)
static int launch_topk_rows(storm_hip_ctx_t* ctx, const uint32_t* d_counts_matrix, uint64_t ld, uint64_t n_rows, uint64_t n_cols,
                            const uint32_t* d_counts_rows, const uint32_t* d_counts_cols, uint64_t skip0, int score,
                            uint64_t n_bits, uint64_t k, uint32_t* d_idx, uint32_t* d_val, uint64_t ld_k) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    if (!d_counts_matrix || !d_counts_rows || !d_counts_cols || !d_idx || !d_val) {
        set_error("topk_rows: NULL argument");
        return STORM_HIP_EINVAL;
    }
    if (int rc = check_topk("topk_rows", score, n_bits, k, ld_k)) return rc;
    if (ld < n_cols) {
        set_error("topk_rows: leading dimension %llu < %llu columns", (unsigned long long)ld, (unsigned long long)n_cols);
        return STORM_HIP_EINVAL;
    }
    if (n_rows > 0x7fffffffull || n_cols > 0xffffffffull) {
        set_error("topk_rows: %llu x %llu entries exceed the launch grid or the 32-bit column index",
                  (unsigned long long)n_rows, (unsigned long long)n_cols);
        return STORM_HIP_EINVAL;
    }
    if (n_rows == 0) return STORM_HIP_OK;
    STORM_HIP_TRY(hipSetDevice(ctx->device));
    const int vec = reinterpret_cast<uintptr_t>(d_counts_matrix) % 16 == 0 && ld % 4 == 0;
    const TopkBitScorer::Args args = {d_counts_matrix, d_counts_rows, d_counts_cols, ld, n_bits, score, vec};
    hipLaunchKernelGGL(topk_rows_kernel<TopkBitScorer>, dim3((uint32_t)n_rows), dim3(kTopkThreads), 0, ctx->stream, args, n_cols, skip0,
                       (uint32_t)k, d_idx, d_val, ld_k);
    STORM_HIP_TRY(hipGetLastError());
    ctx->pass_report[0] |= STORM_HIP_RAN_TOPK;
    return STORM_HIP_OK;
}

// rows of a panel: `panel_rows` as given (a multiple of 256), or for 0 the largest multiple of 256 whose panel of `ld`
// uint32 per row is at most 256 MiB, at least 256; never more than the rows there are, rounded up to 256
static int panel_rows_of(const char* who, uint64_t panel_rows, uint64_t n_rows, uint64_t ld, uint64_t* out) {
    if (panel_rows % 256u != 0) {
        set_error("%s: panel_rows %llu is not a multiple of 256 (0: chosen by the library)", who, (unsigned long long)panel_rows);
        return STORM_HIP_EINVAL;
    }
    if (panel_rows == 0) panel_rows = std::max<uint64_t>(256u, ((256ull << 20) / (std::max<uint64_t>(ld, 1u) * sizeof(uint32_t))) / 256u * 256u);
    *out = std::min<uint64_t>(panel_rows, (n_rows + 255u) / 256u * 256u);
    return STORM_HIP_OK;
}

// Rows of `a` against all rows of `b` (self: a == b, and row i never lists itself), panel by panel, queued on the
// context's stream and not waited for. d_idx / d_val == nullptr: both arrays packed (pitch k) behind the panel in the
// context's band buffer, at *d_idx_out / *d_val_out.
static int topk_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, bool self, int score,
                       uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* d_idx, uint32_t* d_val, uint64_t ld_k,
                       uint32_t** d_idx_out, uint32_t** d_val_out) {
    const uint64_t na = a->n_rows, nb = b->n_rows;
    const uint64_t ld = (nb + 3u) / 4u * 4u;   // whole 128-bit vectors per panel row
    const size_t panel_words = (size_t)panel_rows * ld, out_words = d_idx ? 0 : (size_t)na * k;
    if (int rc = ctx->d_band.ensure((panel_words + 2 * out_words + 4) * sizeof(uint32_t), "topk: the count panel")) return rc;
    if (!d_idx) {
        d_idx = ctx->d_band.d + panel_words;
        d_val = d_idx + out_words;
        ld_k = k;
    }
    if (int rc = ctx->d_counts.ensure((na + (self ? 0 : nb) + 1) * sizeof(uint32_t), "topk: the row-count scratch")) return rc;
    uint32_t* const d_rows = ctx->d_counts.d;
    uint32_t* const d_cols = self ? d_rows : d_rows + na;
    if (int rc = launch_row_counts(ctx, a, d_rows)) return rc;
    if (!self)
        if (int rc = launch_row_counts(ctx, b, d_cols)) return rc;
    for (uint64_t p0 = 0; p0 < na; p0 += panel_rows) {
        // the panel's A operand: a view of `a`, no rows copied. p0 is a multiple of 256, as n_rows_pad is, so the view's
        // whole 256-row tiles end inside the parent's allocation and its last tile's rows beyond n_rows are the parent's
        // zero rows. launch_square_matrix keys no cache by the operand (it builds a forced FP4 shadow fresh every call).
        storm_hip_matrix_s view = *a;
        view.d = a->d + p0 * a->stride_words;
        view.n_rows = std::min(panel_rows, na - p0);
        view.n_rows_pad = a->n_rows_pad - p0;
        if (int rc = launch_square_matrix(ctx, &view, b, STORM_HIP_OP_AND, ctx->d_band.d, ld)) return rc;
        if (int rc = launch_topk_rows(ctx, ctx->d_band.d, ld, view.n_rows, nb, d_rows + p0, d_cols, self ? p0 : ~0ull, score, n_bits,
                                      k, d_idx + p0 * ld_k, d_val + p0 * ld_k, ld_k))
            return rc;
    }
    ctx->pass_report[0] = STORM_HIP_RAN_TILES_OUT | STORM_HIP_RAN_TOPK;
    ctx->pass_report[1] = na * nb * a->n_words;
    ctx->pass_report[2] = ctx->pass_report[3] = 0;
    if (d_idx_out) *d_idx_out = d_idx;
    if (d_val_out) *d_val_out = d_val;
    return STORM_HIP_OK;
}

// the checks of the pairw (b == nullptr) and cross forms, then the panels; host != 0: idx / val are host arrays
static int topk_call(const char* who, storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, bool self,
                     int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* idx, void* val, uint64_t ld_k,
                     bool host) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    if (!a || !b || !idx || !val) {
        set_error("%s: NULL argument", who);
        return STORM_HIP_EINVAL;
    }
    if (int rc = check_topk(who, score, n_bits, k, ld_k)) return rc;
    if (a->n_words != b->n_words) {
        set_error("%s: row widths differ", who);
        return STORM_HIP_EINVAL;
    }
    uint64_t rows_per_panel = 0;
    if (int rc = panel_rows_of(who, panel_rows, a->n_rows, (b->n_rows + 3u) / 4u * 4u, &rows_per_panel)) return rc;
    if (a->n_rows == 0) return STORM_HIP_OK;
    STORM_HIP_TRY(hipSetDevice(ctx->device));
    uint32_t *d_idx = nullptr, *d_val = nullptr;
    if (int rc = topk_queued(ctx, a, b, self, score, n_bits, k, rows_per_panel, host ? nullptr : idx,
                             host ? nullptr : static_cast<uint32_t*>(val), ld_k, &d_idx, &d_val))
        return rc;
    if (host) {
        const size_t row_bytes = k * sizeof(uint32_t);
        STORM_HIP_TRY(hipMemcpy2DAsync(idx, ld_k * sizeof(uint32_t), d_idx, row_bytes, row_bytes, a->n_rows, hipMemcpyDeviceToHost,
                                       ctx->stream));
        STORM_HIP_TRY(hipMemcpy2DAsync(val, ld_k * sizeof(uint32_t), d_val, row_bytes, row_bytes, a->n_rows, hipMemcpyDeviceToHost,
                                       ctx->stream));
    }
    STORM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return STORM_HIP_OK;
}

// ---- rows of 2-bit values (dosages): the best r^2 / r / dot-product neighbours ("Top-k rows, dosage form") ----
// the score of a dosage top-k call: r^2, r, or — plain forms only — the dot product
static int check_dosage_topk_score(const char* who, int score, bool complete) {
    if (score != STORM_HIP_DOSAGE_R2 && score != STORM_HIP_DOSAGE_R && (complete || score != STORM_HIP_DOSAGE_TOPK_DOT)) {
        set_error("%s: unknown score %d (0 r^2, 1 r%s)", who, score,
                  complete ? "; the dot product has no pairwise-complete form" : ", 2 the dot product");
        return STORM_HIP_EINVAL;
    }
    return STORM_HIP_OK;
}

// topk_rows_kernel over a complete panel of dot products in device memory, asynchronous (the checks of
// storm_hip_dosage_topk_rows_device)
static int launch_dosage_topk_rows(storm_hip_ctx_t* ctx, const uint32_t* d_dots, uint64_t ld, uint64_t n_rows, uint64_t n_cols,
                                   const uint32_t* d_sum_rows, const uint32_t* d_sq_rows, const uint32_t* d_sum_cols,
                                   const uint32_t* d_sq_cols, uint64_t n_samples, uint64_t skip0, int score, uint64_t k,
                                   uint32_t* d_idx, uint32_t* d_val, uint64_t ld_k) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    if (!d_dots || !d_sum_rows || !d_sq_rows || !d_sum_cols || !d_sq_cols || !d_idx || !d_val) {
        set_error("dosage_topk_rows: NULL argument");
        return STORM_HIP_EINVAL;
    }
    if (int rc = check_dosage_topk_score("dosage_topk_rows", score, false)) return rc;
    if (n_samples == 0 || n_samples > (1ull << 24)) {
        set_error("dosage_topk_rows: n_samples %llu is not in [1, 2^24]", (unsigned long long)n_samples);
        return STORM_HIP_EINVAL;
    }
    if (int rc = check_topk_k("dosage_topk_rows", k, ld_k)) return rc;
    if (ld < n_cols) {
        set_error("dosage_topk_rows: leading dimension %llu < %llu columns", (unsigned long long)ld, (unsigned long long)n_cols);
        return STORM_HIP_EINVAL;
    }
    if (n_rows > 0x7fffffffull || n_cols > 0xffffffffull) {
        set_error("dosage_topk_rows: %llu x %llu entries exceed the launch grid or the 32-bit column index",
                  (unsigned long long)n_rows, (unsigned long long)n_cols);
        return STORM_HIP_EINVAL;
    }
    if (n_rows == 0) return STORM_HIP_OK;
    STORM_HIP_TRY(hipSetDevice(ctx->device));
    const int vec = reinterpret_cast<uintptr_t>(d_dots) % 16 == 0 && ld % 4 == 0;
    const TopkDosageScorer::Args args = {d_dots, d_sum_rows, d_sq_rows, d_sum_cols, d_sq_cols, ld, n_samples, score, vec};
    hipLaunchKernelGGL(topk_rows_kernel<TopkDosageScorer>, dim3((uint32_t)n_rows), dim3(kTopkThreads), 0, ctx->stream, args, n_cols,
                       skip0, (uint32_t)k, d_idx, d_val, ld_k);
    STORM_HIP_TRY(hipGetLastError());
    ctx->pass_report[0] |= STORM_HIP_RAN_TOPK;
    return STORM_HIP_OK;
}

// rows [p0, p0 + rows) of a matrix whose allocation holds rows_alloc rows from x->d, as an operand of its own: no rows copied
static storm_hip_matrix_s rows_view(const storm_hip_matrix_s* x, uint64_t* d, uint64_t rows_alloc, uint64_t p0, uint64_t rows) {
    storm_hip_matrix_s v = *x;
    v.d = d + p0 * x->stride_words;
    v.n_rows = rows;
    v.n_rows_pad = rows_alloc - p0;
    return v;
}

// Rows of `a` against all rows of `b` (self: a == b and row i never lists itself), panel by panel, queued on the context's
// stream and not waited for. Per call: both matrices' row sums (dosage_row_sums_kernel), or with `complete` both splits
// (one when b is a). Per panel of rows_per_panel rows of `a` the planes of integer sums against ALL of b, then the selection,
// which forms every entry's value itself — no float matrix and no finish pass:
//   plain    : P = view(a) x b                                                        (1 launch of K2h, n_a n_b products)
//   complete : P = G_p x G_b; G_p x M_b and H_p x M_b, panel_rows rows apart; M_p x [G_b ; H_b ; M_b]
//              ([G ; H] of the split is rows128 rows apart, so a panel of it is not one matrix: 4 launches, still 6 n_a n_b)
// all in the context's band buffer, with both output arrays packed (pitch k) behind them when d_idx / d_val == nullptr
// (then at *d_idx_out / *d_val_out). The scratch is rows_per_panel x about n_b (complete: 6 n_b) words, not n_a x n_b.
//
// The views: p0 is a multiple of 256. A mirror's allocation is n_rows_pad rows, a multiple of 256 with zero rows behind
// n_rows; each matrix of a split is rows128 rows, a multiple of 128 with zero rows behind n_rows, and p0 < n_rows <= both.
// K2h reads an A operand in 128-row tiles up to the view's n_rows rounded up to 256, and no row at or beyond its
// n_rows_pad (TileOperands::tile_rows: the tile's buffer range ends there, reads beyond return zero). With n_rows_pad =
// the allocation's rows - p0 every whole tile therefore ends inside the allocation the view points into — never in the
// next matrix of the split — and what a last, short panel reads behind its rows are that allocation's zero rows. A panel
// that is not the last has n_rows = rows_per_panel, a multiple of 256: it reads its own rows alone. launch_tile128 keys its
// cached list by the tiles' geometry, not by the operand: panels of equal height share one list.
static int dosage_topk_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, bool self,
                              bool complete, int score, uint64_t n_samples, uint64_t k, uint64_t rows_per_panel, uint32_t* d_idx,
                              uint32_t* d_val, uint64_t ld_k, uint32_t** d_idx_out, uint32_t** d_val_out) {
    const uint64_t na = a->n_rows, nb = b->n_rows;
    if (nb == 0) complete = false;   // (no column: k paddings per row either way, and nothing to split)
    const uint64_t ld = (nb + 3u) / 4u * 4u;   // whole 128-bit vectors per panel row, in every plane
    DosageSplit sa, sb;
    if (complete)
        if (int rc = dosage_split_pair_queued(ctx, a, b, n_samples, &sa, &sb)) return rc;
    const uint64_t ld_mghm = complete ? 2 * sb.rows128 + ld : 0;
    const size_t p_words = (size_t)rows_per_panel * ld, ghm_words = complete ? 2 * p_words : 0;
    const size_t plane_words = p_words + ghm_words + (size_t)rows_per_panel * ld_mghm;
    const size_t out_words = d_idx ? 0 : (size_t)na * k;
    if (int rc = ctx->d_band.ensure((plane_words + 2 * out_words + 4) * sizeof(uint32_t), "dosage_topk: the panel of sums")) return rc;
    uint32_t* const d_p = ctx->d_band.d;
    uint32_t* const d_ghm = d_p + p_words;
    uint32_t* const d_mghm = d_ghm + ghm_words;
    if (!d_idx) {
        d_idx = d_p + plane_words;
        d_val = d_idx + out_words;
        ld_k = k;
    }
    SquareSums sums = {};
    if (!complete && nb != 0) {
        if (int rc = dosage_square_sums_queued(ctx, a, b, &sums)) return rc;
    } else if (!complete) {   // no column reads b's sums; the rows' own are read and never used
        if (int rc = ctx->d_counts.ensure(2 * na * sizeof(uint32_t), "dosage_topk: the row-sum scratch")) return rc;
        STORM_HIP_TRY(hipMemsetAsync(ctx->d_counts.d, 0, 2 * na * sizeof(uint32_t), ctx->stream));
        sums = SquareSums{ctx->d_counts.d, ctx->d_counts.d + na, ctx->d_counts.d, ctx->d_counts.d};
    }
    for (uint64_t p0 = 0; p0 < na; p0 += rows_per_panel) {
        const uint64_t rows = std::min(rows_per_panel, na - p0);
        uint32_t* const idx_p = d_idx + p0 * ld_k;
        uint32_t* const val_p = d_val + p0 * ld_k;
        if (!complete) {
            const storm_hip_matrix_s view = rows_view(a, a->d, a->n_rows_pad, p0, rows);
            if (int rc = launch_square_dosage_matrix(ctx, &view, b, d_p, ld)) return rc;
            if (int rc = launch_dosage_topk_rows(ctx, d_p, ld, rows, nb, sums.a_sum + p0, sums.a_sq + p0, sums.b_sum, sums.b_sq,
                                                 n_samples, self ? p0 : ~0ull, score, k, idx_p, val_p, ld_k))
                return rc;
            continue;
        }
        uint64_t* const G = sa.g.d;   // H and M follow, rows128 rows each (dosage_split_at)
        const uint64_t words = sa.rows128 * a->stride_words;
        const storm_hip_matrix_s g_p = rows_view(&sa.g, G, sa.rows128, p0, rows);
        const storm_hip_matrix_s h_p = rows_view(&sa.g, G + words, sa.rows128, p0, rows);
        const storm_hip_matrix_s m_p = rows_view(&sa.g, G + 2 * words, sa.rows128, p0, rows);
        if (int rc = launch_square_dosage_matrix(ctx, &g_p, &sb.g, d_p, ld)) return rc;
        if (int rc = launch_square_dosage_matrix(ctx, &g_p, &sb.m, d_ghm, ld)) return rc;
        if (int rc = launch_square_dosage_matrix(ctx, &h_p, &sb.m, d_ghm + p_words, ld)) return rc;
        if (int rc = launch_square_dosage_matrix(ctx, &m_p, &sb.ghm, d_mghm, ld_mghm)) return rc;
        // (every plane's base is a multiple of 4 words from the buffer's, every pitch and column offset a multiple of 4)
        const int vec = reinterpret_cast<uintptr_t>(d_p) % 16 == 0;
        const TopkDosageCompleteScorer::Args args = {d_p, d_ghm, d_mghm, ld, ld, rows_per_panel, ld_mghm, sb.rows128, 2 * sb.rows128,
                                                     score, vec};
        hipLaunchKernelGGL(topk_rows_kernel<TopkDosageCompleteScorer>, dim3((uint32_t)rows), dim3(kTopkThreads), 0, ctx->stream, args,
                           nb, self ? p0 : ~0ull, (uint32_t)k, idx_p, val_p, ld_k);
        STORM_HIP_TRY(hipGetLastError());
    }
    ctx->pass_report[0] = STORM_HIP_RAN_TILES_OUT | STORM_HIP_RAN_TOPK;
    ctx->pass_report[1] = (complete ? 6u : 1u) * na * nb * a->n_words;
    ctx->pass_report[2] = ctx->pass_report[3] = 0;
    if (d_idx_out) *d_idx_out = d_idx;
    if (d_val_out) *d_val_out = d_val;
    return STORM_HIP_OK;
}

// the checks of the pairw (b == a, self) and square forms, then the panels; host: idx / val are host arrays
static int dosage_topk_call(const char* who, storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, bool self,
                            bool complete, int score, uint64_t n_samples, uint64_t k, uint64_t panel_rows, uint32_t* idx, void* val,
                            uint64_t ld_k, bool host) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    if (!val) idx = nullptr;   // (check_square names the NULL argument)
    if (int rc = check_square(who, a, b, idx, b ? b->n_rows : 0)) return rc;
    if (int rc = check_dosage_topk_score(who, score, complete)) return rc;
    if (int rc = check_samples(who, a, n_samples)) return rc;
    if (int rc = check_topk_k(who, k, ld_k)) return rc;
    if (panel_rows % 256u != 0) {
        set_error("%s: panel_rows %llu is not a multiple of 256 (0: chosen by the library)", who, (unsigned long long)panel_rows);
        return STORM_HIP_EINVAL;
    }
    if (a->n_rows == 0) return STORM_HIP_OK;
    if (a->n_rows > 0x7fffffffull || b->n_rows >= 0xffffffffull) {
        set_error("%s: %llu x %llu entries exceed the launch grid or the 32-bit row index", who, (unsigned long long)a->n_rows,
                  (unsigned long long)b->n_rows);
        return STORM_HIP_EINVAL;
    }
    const uint64_t rows_per_panel = dosage_topk_panel_rows(panel_rows, a->n_rows, dosage_topk_plane_words(b->n_rows, complete));
    STORM_HIP_TRY(hipSetDevice(ctx->device));
    uint32_t *d_idx = nullptr, *d_val = nullptr;
    if (int rc = dosage_topk_queued(ctx, a, b, self, complete, score, n_samples, k, rows_per_panel, host ? nullptr : idx,
                                    host ? nullptr : static_cast<uint32_t*>(val), ld_k, &d_idx, &d_val))
        return rc;
    if (host) {
        const size_t row_bytes = k * sizeof(uint32_t);
        STORM_HIP_TRY(hipMemcpy2DAsync(idx, ld_k * sizeof(uint32_t), d_idx, row_bytes, row_bytes, a->n_rows, hipMemcpyDeviceToHost,
                                       ctx->stream));
        STORM_HIP_TRY(hipMemcpy2DAsync(val, ld_k * sizeof(uint32_t), d_val, row_bytes, row_bytes, a->n_rows, hipMemcpyDeviceToHost,
                                       ctx->stream));
    }
    if (wait_stream(ctx) != hipSuccess) {
        ctx->tickets_dirty = true;   // (a K2h launch that died may have left tickets behind: pair_matrix_out)
        set_error("%s: HIP failure", who);
        return STORM_HIP_EHIP;
    }
    return STORM_HIP_OK;
}

}  // namespace storm

using namespace storm;

extern "C" {

int storm_hip_topk_rows_device(storm_hip_ctx_t* ctx, const uint32_t* d_counts_matrix, uint64_t ld, uint64_t n_rows, uint64_t n_cols,
                               const uint32_t* d_counts_rows, const uint32_t* d_counts_cols, uint64_t skip0, int score,
                               uint64_t n_bits, uint64_t k, uint32_t* d_idx, void* d_val, uint64_t ld_k) {
    return guarded("storm_hip_topk_rows_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        if (int rc = launch_topk_rows(ctx, d_counts_matrix, ld, n_rows, n_cols, d_counts_rows, d_counts_cols, skip0, score, n_bits,
                                      k, d_idx, static_cast<uint32_t*>(d_val), ld_k))
            return rc;
        // alone on a caller's matrix the pass is the whole call: a report of its own (no rows: nothing launched, as it was)
        if (n_rows) {
            memset(ctx->pass_report, 0, sizeof(ctx->pass_report));
            ctx->pass_report[0] = STORM_HIP_RAN_TOPK;
        }
        return STORM_HIP_OK;
    });
}

int storm_hip_pairw_topk_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int score, uint64_t n_bits, uint64_t k,
                                uint64_t panel_rows, uint32_t* d_idx, void* d_val, uint64_t ld_k) {
    return guarded("storm_hip_pairw_topk_device", [&]() -> int {
        return topk_call("pairw_topk", ctx, m, m, true, score, n_bits, k, panel_rows, d_idx, d_val, ld_k, false);
    });
}

int storm_hip_pairw_topk(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int score, uint64_t n_bits, uint64_t k,
                         uint64_t panel_rows, uint32_t* h_idx, void* h_val, uint64_t ld_k) {
    return guarded("storm_hip_pairw_topk", [&]() -> int {
        return topk_call("pairw_topk", ctx, m, m, true, score, n_bits, k, panel_rows, h_idx, h_val, ld_k, true);
    });
}

int storm_hip_cross_dense_topk_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int score,
                                      uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* d_idx, void* d_val,
                                      uint64_t ld_k) {
    return guarded("storm_hip_cross_dense_topk_device", [&]() -> int {
        return topk_call("cross_dense_topk", ctx, a, b, false, score, n_bits, k, panel_rows, d_idx, d_val, ld_k, false);
    });
}

int storm_hip_cross_dense_topk(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int score,
                               uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* h_idx, void* h_val, uint64_t ld_k) {
    return guarded("storm_hip_cross_dense_topk", [&]() -> int {
        return topk_call("cross_dense_topk", ctx, a, b, false, score, n_bits, k, panel_rows, h_idx, h_val, ld_k, true);
    });
}

int storm_hip_dosage_topk_rows_device(storm_hip_ctx_t* ctx, const uint32_t* d_dots, uint64_t ld, uint64_t n_rows, uint64_t n_cols,
                                      const uint32_t* d_sum_rows, const uint32_t* d_sq_rows, const uint32_t* d_sum_cols,
                                      const uint32_t* d_sq_cols, uint64_t n_samples, uint64_t skip0, int score, uint64_t k,
                                      uint32_t* d_idx, void* d_val, uint64_t ld_k) {
    return guarded("storm_hip_dosage_topk_rows_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        if (int rc = launch_dosage_topk_rows(ctx, d_dots, ld, n_rows, n_cols, d_sum_rows, d_sq_rows, d_sum_cols, d_sq_cols, n_samples,
                                             skip0, score, k, d_idx, static_cast<uint32_t*>(d_val), ld_k))
            return rc;
        if (n_rows) {   // alone on a caller's panel the pass is the whole call (storm_hip_topk_rows_device)
            memset(ctx->pass_report, 0, sizeof(ctx->pass_report));
            ctx->pass_report[0] = STORM_HIP_RAN_TOPK;
        }
        return STORM_HIP_OK;
    });
}

#define STORM_DOSAGE_TOPK_FORMS(name, who, complete)                                                                                  \
    int storm_hip_pairw_##name##_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int score, uint64_t n_samples, uint64_t k,  \
                                        uint64_t panel_rows, uint32_t* d_idx, void* d_val, uint64_t ld_k) {                            \
        return guarded("storm_hip_pairw_" #name "_device", [&]() -> int {                                                              \
            return dosage_topk_call("pairw_" who, ctx, m, m, true, complete, score, n_samples, k, panel_rows, d_idx, d_val, ld_k,      \
                                    false);                                                                                            \
        });                                                                                                                            \
    }                                                                                                                                  \
    int storm_hip_pairw_##name(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int score, uint64_t n_samples, uint64_t k,           \
                               uint64_t panel_rows, uint32_t* h_idx, void* h_val, uint64_t ld_k) {                                     \
        return guarded("storm_hip_pairw_" #name, [&]() -> int {                                                                        \
            return dosage_topk_call("pairw_" who, ctx, m, m, true, complete, score, n_samples, k, panel_rows, h_idx, h_val, ld_k,      \
                                    true);                                                                                             \
        });                                                                                                                            \
    }                                                                                                                                  \
    int storm_hip_square_##name##_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int score,    \
                                         uint64_t n_samples, uint64_t k, uint64_t panel_rows, uint32_t* d_idx, void* d_val,            \
                                         uint64_t ld_k) {                                                                              \
        return guarded("storm_hip_square_" #name "_device", [&]() -> int {                                                             \
            return dosage_topk_call("square_" who, ctx, a, b, false, complete, score, n_samples, k, panel_rows, d_idx, d_val, ld_k,    \
                                    false);                                                                                            \
        });                                                                                                                            \
    }                                                                                                                                  \
    int storm_hip_square_##name(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int score,             \
                                uint64_t n_samples, uint64_t k, uint64_t panel_rows, uint32_t* h_idx, void* h_val, uint64_t ld_k) {    \
        return guarded("storm_hip_square_" #name, [&]() -> int {                                                                       \
            return dosage_topk_call("square_" who, ctx, a, b, false, complete, score, n_samples, k, panel_rows, h_idx, h_val, ld_k,    \
                                    true);                                                                                             \
        });                                                                                                                            \
    }
STORM_DOSAGE_TOPK_FORMS(dosage_topk, "dosage_topk", false)
STORM_DOSAGE_TOPK_FORMS(dosage_topk_complete, "dosage_topk_complete", true)
#undef STORM_DOSAGE_TOPK_FORMS

}  // extern "C"
