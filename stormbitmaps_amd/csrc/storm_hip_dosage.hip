// storm_hip_dosage.hip — rows of 2-bit VALUES (genotype dosages 0 / 1 / 2; 3 is an ordinary value) instead of bits: value s
// of a row in bits 2 (s % 32), 2 (s % 32) + 1 of word s / 32 of an ordinary storm_hip_matrix_t. The dot products of all row
// pairs come from K2h in its dosage form (tile128_kernel<false, 2>, storm_hip_mfma.hip: launch_pairw_dosage_matrix); this
// file holds the two small kernels around it — the rows' sums and sums of squares, and the in-place uint32 -> float pass
// that turns a dot product into PLINK's --r / --r2, the (squared) Pearson correlation of two dosage vectors — and the
// C-ABI of the form. Plain vector code; the formula is storm_dosage_math.h. Missing genotypes are out of scope.
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

constexpr int kDosTileRows = 64;    // a wave walks every 4th row of the tile ...
constexpr int kDosTileCols = 256;   // ... one 128-bit vector (4 entries) per lane
constexpr int kDosUnroll = 4;       // rows a wave has in flight

// The finishing pass over the upper triangle of an n x n matrix of dot products, in place (similarity_finish_kernel's
// shape: grid (column tiles, row tiles), a tile at or below the diagonal exits at once; entries i >= j and the pitch columns
// [n, ld) are neither read nor written; vec: 16-byte aligned base and ld a multiple of 4).
__global__ __launch_bounds__(256) void dosage_finish_kernel(uint32_t* __restrict__ io, uint64_t ld, uint64_t n,
                                                            const uint32_t* __restrict__ sum, const uint32_t* __restrict__ sum_sq,
                                                            int measure, uint64_t n_samples, int vec) {
    const uint64_t row0 = (uint64_t)blockIdx.y * kDosTileRows, col0 = (uint64_t)blockIdx.x * kDosTileCols;
    if (col0 + kDosTileCols <= row0 + 1) return;   // the tile's last column is not beyond its first row
    __shared__ uint32_t s_sum[kDosTileRows], s_sq[kDosTileRows];
    if (threadIdx.x < kDosTileRows) {
        const bool in = row0 + threadIdx.x < n;
        s_sum[threadIdx.x] = in ? sum[row0 + threadIdx.x] : 0u;
        s_sq[threadIdx.x] = in ? sum_sq[row0 + threadIdx.x] : 0u;
    }
    const uint64_t c0 = col0 + (threadIdx.x & 63u) * 4u;
    uint32_t bs[4], bq[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        bs[k] = c0 + k < n ? sum[c0 + k] : 0u;
        bq[k] = c0 + k < n ? sum_sq[c0 + k] : 0u;
    }
    __syncthreads();
    const uint32_t wave = threadIdx.x >> 6;
    for (uint32_t r = wave; r < kDosTileRows; r += 4 * kDosUnroll) {
        uint4 v[kDosUnroll];
        bool whole[kDosUnroll];
#pragma unroll
        for (int u = 0; u < kDosUnroll; ++u) {   // the loads of kDosUnroll rows leave before the first divide
            const uint64_t i = row0 + r + 4u * u;
            whole[u] = vec && i < n && c0 + 4 <= n && c0 > i;
            if (whole[u]) v[u] = *reinterpret_cast<const uint4*>(io + i * ld + c0);
        }
#pragma unroll
        for (int u = 0; u < kDosUnroll; ++u) {
            const uint64_t i = row0 + r + 4u * u;
            if (i >= n) continue;
            const uint32_t as = s_sum[r + 4u * u], aq = s_sq[r + 4u * u];
            uint32_t* const p = io + i * ld + c0;
            if (whole[u]) {
                uint4 w;
                w.x = dosage_corr_bits(v[u].x, as, aq, bs[0], bq[0], measure, n_samples);
                w.y = dosage_corr_bits(v[u].y, as, aq, bs[1], bq[1], measure, n_samples);
                w.z = dosage_corr_bits(v[u].z, as, aq, bs[2], bq[2], measure, n_samples);
                w.w = dosage_corr_bits(v[u].w, as, aq, bs[3], bq[3], measure, n_samples);
                *reinterpret_cast<uint4*>(p) = w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c0 + k < n && c0 + k > i) p[k] = dosage_corr_bits(p[k], as, aq, bs[k], bq[k], measure, n_samples);
            }
        }
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
    if (int rc = launch_pairw_dosage_matrix(ctx, m, d_io, ld, false)) return rc;
    if (int rc = dosage_sums_queued(ctx, m)) return rc;
    const uint64_t tiles_x = (n + kDosTileCols - 1) / kDosTileCols, tiles_y = (n + kDosTileRows - 1) / kDosTileRows;
    if (tiles_y > 65535u) {
        set_error("pairw_dosage_corr: %llu rows exceed the finishing pass's launch grid", (unsigned long long)n);
        return STORM_HIP_EINVAL;
    }
    const int vec = reinterpret_cast<uintptr_t>(d_io) % 16 == 0 && ld % 4 == 0;
    hipLaunchKernelGGL(dosage_finish_kernel, dim3((uint32_t)tiles_x, (uint32_t)tiles_y), dim3(256), 0, ctx->stream, d_io, ld, n,
                       ctx->d_counts.d, ctx->d_counts.d + n, measure, n_samples, vec);
    STORM_HIP_TRY(hipGetLastError());
    ctx->pass_report[0] |= STORM_HIP_RAN_SIMILARITY;
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
static int check_corr(const char* who, const storm_hip_matrix_s* m, int measure, uint64_t n_samples) {
    if (measure != STORM_HIP_DOSAGE_R2 && measure != STORM_HIP_DOSAGE_R) {
        set_error("%s: unknown measure %d (0 r^2, 1 r)", who, measure);
        return STORM_HIP_EINVAL;
    }
    if (n_samples == 0 || (n_samples + 31u) / 32u != m->n_words) {
        set_error("%s: %llu samples do not fill rows of %u words (32 values per word)", who, (unsigned long long)n_samples,
                  m->n_words);
        return STORM_HIP_EINVAL;
    }
    return STORM_HIP_OK;
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
    return guarded("storm_hip_pairw_dosage_matrix_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        if (int rc = check_dosage("pairw_dosage_matrix", m, d_out, ld)) return rc;
        if (m->n_rows < 2) return STORM_HIP_OK;
        STORM_HIP_TRY(hipSetDevice(ctx->device));
        return launch_pairw_dosage_matrix(ctx, m, d_out, ld, true);
    });
}

int storm_hip_pairw_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint32_t* h_out, uint64_t ld) {
    return guarded("storm_hip_pairw_dosage_matrix", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        if (int rc = check_dosage("pairw_dosage_matrix", m, h_out, ld)) return rc;
        const uint64_t n = m->n_rows;
        if (n == 0) return STORM_HIP_OK;
        STORM_HIP_TRY(hipSetDevice(ctx->device));
        const size_t need = (size_t)n * n * sizeof(uint32_t);
        if (int rc = ctx->d_band.ensure(need, "pairw_dosage_matrix: the output")) return rc;
        STORM_HIP_TRY(hipMemsetAsync(ctx->d_band, 0, need, ctx->stream));   // (entries i >= j)
        if (int rc = launch_pairw_dosage_matrix(ctx, m, ctx->d_band, n, false)) return rc;
        STORM_HIP_TRY(hipMemcpy2DAsync(h_out, ld * sizeof(uint32_t), ctx->d_band, n * sizeof(uint32_t), n * sizeof(uint32_t), n,
                                       hipMemcpyDeviceToHost, ctx->stream));
        STORM_HIP_TRY(hipStreamSynchronize(ctx->stream));
        return STORM_HIP_OK;
    });
}

int storm_hip_pairw_dosage_corr_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                       float* d_out, uint64_t ld) {
    return guarded("storm_hip_pairw_dosage_corr_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        if (int rc = check_dosage("pairw_dosage_corr", m, d_out, ld)) return rc;
        if (int rc = check_corr("pairw_dosage_corr", m, measure, n_samples)) return rc;
        if (m->n_rows < 2) return STORM_HIP_OK;
        STORM_HIP_TRY(hipSetDevice(ctx->device));
        if (int rc = dosage_corr_queued(ctx, m, measure, n_samples, reinterpret_cast<uint32_t*>(d_out), ld)) return rc;
        STORM_HIP_TRY(hipStreamSynchronize(ctx->stream));
        return STORM_HIP_OK;
    });
}

int storm_hip_pairw_dosage_corr(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples, float* h_out,
                                uint64_t ld) {
    return guarded("storm_hip_pairw_dosage_corr", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        if (int rc = check_dosage("pairw_dosage_corr", m, h_out, ld)) return rc;
        if (int rc = check_corr("pairw_dosage_corr", m, measure, n_samples)) return rc;
        const uint64_t n = m->n_rows;
        if (n == 0) return STORM_HIP_OK;
        STORM_HIP_TRY(hipSetDevice(ctx->device));
        const size_t need = (size_t)n * n * sizeof(uint32_t);
        if (int rc = ctx->d_band.ensure(need, "pairw_dosage_corr: the output")) return rc;
        STORM_HIP_TRY(hipMemsetAsync(ctx->d_band, 0, need, ctx->stream));   // (entries i >= j: +0.0f is the same zero bits)
        if (n >= 2)
            if (int rc = dosage_corr_queued(ctx, m, measure, n_samples, ctx->d_band, n)) return rc;
        STORM_HIP_TRY(hipMemcpy2DAsync(h_out, ld * sizeof(float), ctx->d_band, n * sizeof(uint32_t), n * sizeof(uint32_t), n,
                                       hipMemcpyDeviceToHost, ctx->stream));
        STORM_HIP_TRY(hipStreamSynchronize(ctx->stream));
        return STORM_HIP_OK;
    });
}

}  // extern "C"
