// storm_hip_lag_sparse.hip — the pairs of a float matrix in the lag layout whose entry exceeds a threshold, as a CSR list
// compacted where the matrix lies (storm.h: STORM_dosage_lag_corr_sparse): the edge set pruning walks (storm_prune_math.h:
// prune_edge; the pairs within the lag and within the rows' windows), forward pairs only, in (i, j) order. Count, scan, fill:
//   lag_band_sparse_count_kernel   band + windows -> one forward bit mask and one count per row; the band is read once
//   lag_sparse_block_sums_kernel   the counts of every 1024 rows -> one sum
//   lag_sparse_scan_sums_kernel    ONE workgroup: the exclusive scan of the sums, and the total into row_start[n]
//   lag_sparse_offsets_kernel      every block scans its own 1024 counts again behind its sum -> row_start[0 .. n)
//   lag_band_sparse_fill_kernel    masks + row_start -> col, val; only listed entries of the band are read a second time
// Plain launches on the context's stream, no atomics, nothing that waits for another workgroup: every output is a pure
// function of the band, the windows and the threshold, so two calls return the same bytes.
#include "storm_hip_internal.h"
#include "storm_lag_sparse_math.h"

namespace storm {

constexpr uint32_t kSpWaves = 4;                       // count and fill: one wave per row, four rows per workgroup
constexpr uint32_t kSpThreads = kSpWaves * kLanes;     // 256
constexpr uint32_t kSpChunks = 4;                      // count: 64-lag chunks (256 B loads) a lane has in flight

// masks[i * pitch + c], bit b: the pair (i, j = i + 1 + d), d = 64 c + b, is listed: d < min(L, n - 1 - i), j <= hi[i] and
// i >= lo[j] (WIN) and prune_edge(vals[i * ld + d], min_r2). counts[i] = the row's set bits. Lanes take the consecutive lags
// of one chunk: a coalesced 256 B load, one __ballot per chunk is one word of the mask; kSpChunks loads are issued before
// the first is used. A masked lane loads entry (0, 0) — the pair (0, 1), which exists — and drops it: no load waits for a
// predicate, and the corner and the pitch columns of vals are never read.
template <bool WIN>
__global__ __launch_bounds__(kSpThreads) void lag_band_sparse_count_kernel(const float* __restrict__ vals, uint64_t ld, uint64_t n,
                                                                           uint64_t lag, float min_r2,
                                                                           const uint32_t* __restrict__ lo,
                                                                           const uint32_t* __restrict__ hi,
                                                                           uint64_t* __restrict__ masks, uint32_t pitch,
                                                                           uint32_t* __restrict__ counts) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kSpWaves + wave;
    if (i >= n) return;   // (the whole wave)
    const uint64_t live = lag < n - 1u - i ? lag : n - 1u - i;   // the row's lags that are pairs
    const uint64_t hi_i = WIN ? (uint64_t)hi[i] : 0u;
    const uint64_t row = i * ld;
    uint32_t count = 0;
    for (uint32_t c0 = 0; c0 < pitch; c0 += kSpChunks) {
        float v[kSpChunks];
        bool ok[kSpChunks];
#pragma unroll
        for (uint32_t u = 0; u < kSpChunks; ++u) {
            const uint64_t d = 64ull * (c0 + u) + lane, j = i + 1u + d;
            ok[u] = d < live;
            if (WIN) ok[u] = ok[u] && j <= hi_i && i >= (uint64_t)lo[ok[u] ? j : 0u];
            v[u] = vals[ok[u] ? row + d : 0u];
        }
#pragma unroll
        for (uint32_t u = 0; u < kSpChunks; ++u) {
            const uint64_t bits = __ballot(ok[u] && prune_edge(v[u], min_r2));
            if (c0 + u < pitch) {   // (uniform)
                if (lane == 0) masks[i * pitch + c0 + u] = bits;
                count += (uint32_t)__popcll(bits);
            }
        }
    }
    if (lane == 0) counts[i] = count;
}

// the inclusive scan of one value per thread over a workgroup of kSparseScanThreads; *total = the workgroup's sum
__device__ __forceinline__ uint64_t sparse_block_scan(uint64_t x, uint64_t* s_wave, uint64_t* total) {
    constexpr uint32_t kW = kSparseScanThreads / kLanes;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
    for (int m = 1; m < kLanes; m <<= 1) {
        const uint64_t other = __shfl_up((unsigned long long)x, m);
        if ((int)lane >= m) x += other;
    }
    if (lane == (uint32_t)kLanes - 1u) s_wave[wave] = x;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kW; ++w) {
        const uint64_t s = s_wave[w];
        before += w < wave ? s : 0u;
        all += s;
    }
    __syncthreads();   // (s_wave may be written again)
    *total = all;
    return x + before;
}

__global__ __launch_bounds__(kSparseScanThreads) void lag_sparse_block_sums_kernel(const uint32_t* __restrict__ counts, uint64_t n,
                                                                                  uint64_t* __restrict__ sums) {
    __shared__ uint64_t s_wave[kSparseScanThreads / kLanes];
    const uint64_t r0 = (uint64_t)blockIdx.x * kSparseScanRows + (uint64_t)threadIdx.x * kSparseScanPerThread;
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSparseScanPerThread; ++k) mine += r0 + k < n ? counts[r0 + k] : 0u;
    uint64_t total;
    (void)sparse_block_scan(mine, s_wave, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[b] = the sum of the blocks before b, in place; row_start[n] = the sum of all. One workgroup walks the sums in
// pieces of its own size and carries the running total from piece to piece.
__global__ __launch_bounds__(kSparseScanThreads) void lag_sparse_scan_sums_kernel(uint64_t* __restrict__ sums, uint64_t n_blocks,
                                                                                 uint64_t* __restrict__ row_start, uint64_t n) {
    __shared__ uint64_t s_wave[kSparseScanThreads / kLanes];
    uint64_t carry = 0;
    for (uint64_t b0 = 0; b0 < n_blocks; b0 += kSparseScanThreads) {
        const uint64_t b = b0 + threadIdx.x;
        const uint64_t x = b < n_blocks ? sums[b] : 0u;
        uint64_t total;
        const uint64_t incl = sparse_block_scan(x, s_wave, &total);
        if (b < n_blocks) sums[b] = carry + incl - x;
        carry += total;
    }
    if (threadIdx.x == 0) row_start[n] = carry;
}

__global__ __launch_bounds__(kSparseScanThreads) void lag_sparse_offsets_kernel(const uint32_t* __restrict__ counts, uint64_t n,
                                                                               const uint64_t* __restrict__ sums,
                                                                               uint64_t* __restrict__ row_start) {
    __shared__ uint64_t s_wave[kSparseScanThreads / kLanes];
    const uint64_t r0 = (uint64_t)blockIdx.x * kSparseScanRows + (uint64_t)threadIdx.x * kSparseScanPerThread;
    uint32_t c[kSparseScanPerThread];
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t k = 0; k < kSparseScanPerThread; ++k) {
        c[k] = r0 + k < n ? counts[r0 + k] : 0u;
        mine += c[k];
    }
    uint64_t total;
    uint64_t at = sums[blockIdx.x] + sparse_block_scan(mine, s_wave, &total) - mine;
#pragma unroll
    for (uint32_t k = 0; k < kSparseScanPerThread; ++k) {
        if (r0 + k < n) row_start[r0 + k] = at;
        at += c[k];
    }
}

// col[s] = j and val[s] = vals[i * ld + j - i - 1] for the set bits of row i's mask, s = sparse_slot(..) < capacity: one wave
// per row, the mask word of a chunk is one address for the whole wave. Nothing is written at or behind `capacity`.
__global__ __launch_bounds__(kSpThreads) void lag_band_sparse_fill_kernel(const float* __restrict__ vals, uint64_t ld, uint64_t n,
                                                                          const uint64_t* __restrict__ masks, uint32_t pitch,
                                                                          const uint64_t* __restrict__ row_start,
                                                                          uint32_t* __restrict__ col, float* __restrict__ val,
                                                                          uint64_t capacity) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t i = (uint64_t)blockIdx.x * kSpWaves + wave;
    if (i >= n) return;   // (the whole wave)
    const uint64_t first = row_start[i], end = row_start[i + 1u];
    if (first == end || first >= capacity) return;   // (uniform)
    const uint64_t row = i * ld;
    uint64_t before = 0;
    for (uint32_t c = 0; c < pitch && first + before < capacity; ++c) {
        const uint64_t word = masks[i * pitch + c];
        if (word == 0) continue;   // (uniform)
        const uint64_t slot = sparse_slot(first, before, word, lane);
        if (((word >> lane) & 1ull) && slot < capacity) {
            const uint64_t d = 64ull * c + lane;
            col[slot] = (uint32_t)(i + 1u + d);
            val[slot] = vals[row + d];
        }
        before += (uint64_t)__popcll(word);
    }
}

// what the sparse calls refuse alike, behind their own NULL / max_lag / ld checks
int check_lag_band_sparse(const char* who, uint64_t n_rows, const uint32_t* h_lo, const uint32_t* h_hi, float min_r2,
                          const void* col, const void* val, uint64_t capacity) {
    if (!h_lo != !h_hi) {
        set_error("%s: the window bounds lo and hi come together or not at all", who);
        return STORM_HIP_EINVAL;
    }
    if (!col != !val || (!col && capacity != 0)) {
        set_error("%s: col and val come together; without them (the count-only call) capacity is 0", who);
        return STORM_HIP_EINVAL;
    }
    if (n_rows >= (1ull << 32)) {
        set_error("%s: %llu rows: a column index is 32 bits", who, (unsigned long long)n_rows);
        return STORM_HIP_EINVAL;
    }
    if (min_r2 != min_r2) {
        set_error("%s: min_r2 is NaN", who);
        return STORM_HIP_EINVAL;
    }
    return STORM_HIP_OK;
}

size_t lag_band_sparse_scratch_words(uint64_t n_rows, uint64_t lag, bool windows) {
    return (size_t)sparse_scratch_words(n_rows, lag, windows);
}

// the kernels over a band in device memory with their scratch at d_scratch (8-byte aligned), queued on the context's stream
// (n_rows >= 2, lag = min(max_lag, n_rows - 1) >= 1, check_lag_band_sparse passed; d_col NULL: the offsets alone)
int launch_lag_band_sparse(storm_hip_ctx_t* ctx, const float* d_vals, uint64_t ld, uint64_t n_rows, uint64_t lag, float min_r2,
                           const uint32_t* h_lo, const uint32_t* h_hi, uint64_t* d_row_start, uint32_t* d_col, float* d_val,
                           uint64_t capacity, uint32_t* d_scratch) {
    const uint64_t n = n_rows, n_blocks = sparse_scan_blocks(n);
    const uint32_t pitch = (uint32_t)sparse_mask_pitch(lag);
    uint64_t* const d_masks = reinterpret_cast<uint64_t*>(d_scratch);
    uint64_t* const d_sums = d_masks + (size_t)n * pitch;
    uint32_t* const d_counts = reinterpret_cast<uint32_t*>(d_sums + n_blocks);
    uint32_t* const d_lo = h_lo ? d_counts + n : nullptr;
    uint32_t* const d_hi = h_lo ? d_lo + n : nullptr;
    STORM_HIP_TRY(hipSetDevice(ctx->device));
    if (h_lo) {
        STORM_HIP_TRY(hipMemcpyAsync(d_lo, h_lo, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        STORM_HIP_TRY(hipMemcpyAsync(d_hi, h_hi, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    const uint32_t row_groups = (uint32_t)((n + kSpWaves - 1) / kSpWaves);
    hipLaunchKernelGGL(h_lo ? lag_band_sparse_count_kernel<true> : lag_band_sparse_count_kernel<false>, dim3(row_groups),
                       dim3(kSpThreads), 0, ctx->stream, d_vals, ld, n, lag, min_r2, d_lo, d_hi, d_masks, pitch, d_counts);
    STORM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lag_sparse_block_sums_kernel, dim3((uint32_t)n_blocks), dim3(kSparseScanThreads), 0, ctx->stream, d_counts, n,
                       d_sums);
    STORM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lag_sparse_scan_sums_kernel, dim3(1), dim3(kSparseScanThreads), 0, ctx->stream, d_sums, n_blocks, d_row_start, n);
    STORM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(lag_sparse_offsets_kernel, dim3((uint32_t)n_blocks), dim3(kSparseScanThreads), 0, ctx->stream, d_counts, n,
                       d_sums, d_row_start);
    STORM_HIP_TRY(hipGetLastError());
    if (d_col && capacity) {
        hipLaunchKernelGGL(lag_band_sparse_fill_kernel, dim3(row_groups), dim3(kSpThreads), 0, ctx->stream, d_vals, ld, n, d_masks,
                           pitch, d_row_start, d_col, d_val, capacity);
        STORM_HIP_TRY(hipGetLastError());
    }
    return STORM_HIP_OK;
}

}  // namespace storm

using namespace storm;

extern "C" int storm_hip_lag_band_sparse_device(storm_hip_ctx_t* ctx, const float* d_vals, uint64_t ld, uint64_t n_rows,
                                                uint64_t max_lag, float min_r2, const uint32_t* h_lo, const uint32_t* h_hi,
                                                uint64_t* d_row_start, uint32_t* d_col, float* d_val, uint64_t capacity) {
    return guarded("storm_hip_lag_band_sparse_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        if (!d_vals || !d_row_start || max_lag == 0) {
            set_error("lag_band_sparse: NULL argument or max_lag 0");
            return STORM_HIP_EINVAL;
        }
        const uint64_t lag = n_rows ? std::min(max_lag, n_rows - 1) : 0;
        if (ld < lag) {
            set_error("lag_band_sparse: leading dimension %llu < min(max_lag, rows - 1) = %llu", (unsigned long long)ld,
                      (unsigned long long)lag);
            return STORM_HIP_EINVAL;
        }
        if (int rc = check_lag_band_sparse("lag_band_sparse", n_rows, h_lo, h_hi, min_r2, d_col, d_val, capacity)) return rc;
        STORM_HIP_TRY(hipSetDevice(ctx->device));
        if (n_rows < 2) {   // no pair: the offsets alone, n_rows + 1 zeros
            STORM_HIP_TRY(hipMemsetAsync(d_row_start, 0, (n_rows + 1) * sizeof(uint64_t), ctx->stream));
            return STORM_HIP_OK;
        }
        const size_t words = lag_band_sparse_scratch_words(n_rows, lag, h_lo != nullptr);
        if (int rc = ctx->d_band.ensure(words * sizeof(uint32_t), "lag_band_sparse: the forward masks, counts and windows")) return rc;
        return launch_lag_band_sparse(ctx, d_vals, ld, n_rows, lag, min_r2, h_lo, h_hi, d_row_start, d_col, d_val, capacity,
                                      ctx->d_band.d);
    });
}
