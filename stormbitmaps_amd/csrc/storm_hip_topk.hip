// storm_hip_topk.hip — for each row its k best columns, selected where the counts lie: topk_rows_kernel reads a complete
// panel of intersection counts (uint32, what the matrix-output paths write), forms every entry's score (the AND count
// itself, or the similarity measure of storm_similarity_math.h: bit-identical to the similarity calls) and keeps the k
// largest keys of storm_topk_math.h per row: value descending, then column ascending. n x k entries leave the device
// instead of n x n. The count panel is read once, 4 bytes per entry, and never written.
//
// The forms above the primitive run in row panels: the AND-count rectangle (panel rows x all columns) into the context's
// band buffer through launch_square_matrix with the kernel choice as it is, then the selection over that panel.
#include "storm_hip_internal.h"
#include "storm_similarity_math.h"
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

// Grid: one workgroup per row of the panel. The lanes sweep the row kTopkStep entries at a time (the next step's load
// leaves before this step's arithmetic); a lane appends a key to the staging area only when it beats the threshold, the
// k-th best key of the last sort (0 before the first). Slots come from an LDS counter per step — three of them in
// rotation, so that the step's total is read behind ONE barrier while the lanes ahead already count the next step in
// another word — and the workgroup sorts best U staging whenever the next step could overflow the staging area. Keys
// are unique within a row, so what is kept does not depend on the order the lanes arrive in. No global atomics.
__global__ __launch_bounds__(kTopkThreads) void topk_rows_kernel(const uint32_t* __restrict__ counts, uint64_t ld, uint64_t n_cols,
                                                                 const uint32_t* __restrict__ counts_rows,
                                                                 const uint32_t* __restrict__ counts_cols, uint64_t skip0, int score,
                                                                 uint64_t n_bits, uint32_t k, uint32_t* __restrict__ idx,
                                                                 uint32_t* __restrict__ val, uint64_t ld_k, int vec) {
    __shared__ uint64_t s_keys[kTopkKeys];
    __shared__ uint32_t s_step[3];
    const uint64_t r = blockIdx.x;
    const bool is_count = score == STORM_HIP_TOPK_COUNT;
    const uint32_t* const row = counts + r * ld;
    const uint32_t a = counts_rows[r];
    const uint64_t skip = (skip0 == ~0ull || skip0 > ~0ull - r) ? ~0ull : skip0 + r;   // (no column is ~0: n_cols < 2^32)
    if (threadIdx.x < kTopkBest) s_keys[threadIdx.x] = 0ull;
    if (threadIdx.x < 3) s_step[threadIdx.x] = 0u;
    __syncthreads();
    uint64_t threshold = 0ull;
    uint32_t staged = 0u, step = 0u;   // uniform
    uint4 cur = topk_load4(row, (uint64_t)threadIdx.x * 4u, n_cols, vec);
    for (uint64_t base = 0; base < n_cols; base += kTopkStep) {
        const uint64_t c0 = base + (uint64_t)threadIdx.x * 4u;
        uint4 nxt = make_uint4(0u, 0u, 0u, 0u);
        if (base + kTopkStep < n_cols) nxt = topk_load4(row, c0 + kTopkStep, n_cols, vec);
        uint32_t* const counter = &s_step[step % 3u];
        if (threadIdx.x == 0) s_step[(step + 1u) % 3u] = 0u;   // the next step's: last read two barriers ago
        const uint32_t c[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint64_t j = c0 + e;
            if (j >= n_cols || j == skip) continue;
            const uint32_t bits = is_count ? c[e] : similarity_bits(c[e], a, counts_cols[j], score, n_bits);
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

// what every top-k call refuses alike, before anything is launched
static int check_topk(const char* who, int score, uint64_t n_bits, uint64_t k, uint64_t ld_k) {
    if (score < STORM_HIP_SIM_JACCARD || score > STORM_HIP_TOPK_COUNT) {
        set_error("%s: unknown score %d (0 Jaccard, 1 cosine, 2 LD D, 3 LD r^2, 4 the AND count)", who, score);
        return STORM_HIP_EINVAL;
    }
    if (n_bits == 0 || n_bits > (1ull << 32)) {
        set_error("%s: n_bits %llu is not in [1, 2^32]", who, (unsigned long long)n_bits);
        return STORM_HIP_EINVAL;
    }
    if (k == 0 || k > STORM_HIP_TOPK_MAX || ld_k < k) {
        set_error("%s: k %llu is not in [1, %d], or ld_k %llu < k", who, (unsigned long long)k, STORM_HIP_TOPK_MAX,
                  (unsigned long long)ld_k);
        return STORM_HIP_EINVAL;
    }
    return STORM_HIP_OK;
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
    hipLaunchKernelGGL(topk_rows_kernel, dim3((uint32_t)n_rows), dim3(kTopkThreads), 0, ctx->stream, d_counts_matrix, ld, n_cols,
                       d_counts_rows, d_counts_cols, skip0, score, n_bits, (uint32_t)k, d_idx, d_val, ld_k, vec);
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

}  // extern "C"
