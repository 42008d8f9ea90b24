// storm_hip_prune.hip — greedy LD pruning and clumping from a float matrix in the lag layout, resolved where the matrix
// lies (storm.h: STORM_dosage_lag_prune): the lexicographically first maximal independent set of the graph whose edges are
// the pairs within the lag, within the rows' windows, whose entry exceeds a threshold (storm_prune_math.h: prune_edge), walked
// in a given order. n bytes of keep flags (and n owners) leave the device instead of the n x L band.
//   lag_band_threshold_kernel  band + windows -> one adjacency bit mask per row, both sides, aligned to absolute row numbers
//   band_mis_resolve_kernel    ONE workgroup walks the order in batches of 64 with the removed bits of all rows in the LDS
//   band_mis_rank_kernel       rank[order[k]] = k, and
//   band_mis_owner_kernel      for a removed row the kept neighbour of best rank: only when owners are asked for
// No atomics on floats, nothing that waits for another workgroup: every output is a pure function of the band, the
// windows and the order, so two calls return the same bytes, and keep is the same whether owners are asked for or not.
#include "storm_hip_internal.h"
#include "storm_prune_math.h"

#include <vector>

namespace storm {

constexpr uint32_t kPrRows = 64;                          // threshold: a workgroup owns 64 consecutive rows (i0 a multiple of 64)
constexpr uint32_t kPrWaves = 8;
constexpr uint32_t kPrThreads = kPrWaves * kLanes;        // 512: two waves per SIMD, no register pressure from the bound
constexpr uint32_t kPrRowsPerWave = kPrRows / kPrWaves;   // forward sweep: 8 whole rows per wave
constexpr uint32_t kPrChunks = 1;                         // ... one chunk of 64 rows at a time: 8 loads in flight per lane
constexpr uint32_t kPrBack = 16;                          // backward sweep: loads a lane has in flight before it uses the first
static_assert(kPrRows == (uint32_t)kLanes && 32u % kPrBack == 0, "one lane per row in the backward sweep, whole words");
static_assert(kPrChunks == 1, "the forward loop tests its bound per chunk");

// masks[v * pitch + k], bit b: row j = base(v) + 32 k + b is adjacent to row v (storm_prune_math.h: prune_mask_base /
// _pitch). For i < j the pair is adjacent when j - i <= lag, j <= hi[i] and i >= lo[j] (WIN; symmetric by construction,
// whatever the bounds hold) and prune_edge(vals[i * ld + j - i - 1], min_r2). All `pitch` words of every row are written.
//   backward sweep — the words of row i = i0 + lane that lie wholly behind the block (rows j < i0): as lag_band_sums_kernel's
//     backward sweep, for a source row j the 64 lanes read the 64 CONSECUTIVE lags i0 - j - 1 + lane of row j; a lane ORs
//     the bit of j into a register and stores one word per 32 source rows (32 x less data than it read). Wave w takes the
//     groups of 32 source rows w, w + 8, ..
//   forward sweep — wave w runs along rows i0 + 8 w .. + 7, its lanes over the ABSOLUTE rows j = i0 + 64 c + lane of chunk
//     c: consecutive lanes read consecutive lags, one __ballot per 64 entries is two words of the mask (the chunks are
//     aligned to 64, the bases to 32: no shift). The loop runs to the last word of the pitch: what lies past the lag is 0.
//   the block's own 64 x 64 tile — chunk 0 of the forward sweep gives row i the bits j > i; the bits j < i of row i are the
//     bits i of the rows j before it (the same pairs): wave 0 transposes the 64 ballots through the LDS.
// The band is read once. A masked lane loads entry (0, 0) — the pair (0, 1), which exists — and drops it: no load waits
// for a predicate, and the corner and the pitch columns of vals are never read.
template <bool WIN>
__global__ __launch_bounds__(kPrThreads) void lag_band_threshold_kernel(const float* __restrict__ vals, uint64_t ld, uint64_t n,
                                                                        uint64_t lag, float min_r2,
                                                                        const uint32_t* __restrict__ lo,
                                                                        const uint32_t* __restrict__ hi,
                                                                        uint32_t* __restrict__ masks, uint32_t pitch) {
    __shared__ uint64_t s_fwd[kPrRows];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t i0 = (uint64_t)blockIdx.x * kPrRows;

    // ---- backward: row i = i0 + lane gathers the rows before the block
    {
        const uint64_t i = i0 + lane, base_i = prune_mask_base(i, lag);
        const uint64_t lo_i = (WIN && i < n) ? (uint64_t)lo[i] : 0u;
        for (uint64_t g = prune_mask_base(i0, lag) + 32u * wave; g < i0; g += 32u * kPrWaves) {
            uint32_t word = 0;
#pragma unroll
            for (uint32_t u0 = 0; u0 < 32u; u0 += kPrBack) {
                float v[kPrBack];
                bool ok[kPrBack];
#pragma unroll
                for (uint32_t u = 0; u < kPrBack; ++u) {
                    const uint64_t j = g + u0 + u;   // (j < i0 <= n - 1: the pair (j, j + 1) exists)
                    ok[u] = i < n && i - j - 1u < lag && j >= lo_i && (!WIN || i <= (uint64_t)hi[j]);
                    v[u] = vals[j * ld + (ok[u] ? i - j - 1u : 0u)];
                }
#pragma unroll
                for (uint32_t u = 0; u < kPrBack; ++u) word |= (ok[u] && prune_edge(v[u], min_r2) ? 1u : 0u) << (u0 + u);
            }
            // (g < base_i: every row of the group is more than lag behind row i, the word is 0 and has no place)
            if (i < n && g >= base_i) masks[i * pitch + (g - base_i) / 32u] = word;
        }
    }

    // ---- forward: a whole wave along each of its eight rows, chunks of 64 absolute rows from the block's own
    {
        const uint64_t i_last = i0 + wave * kPrRowsPerWave + (kPrRowsPerWave - 1u);   // the largest base of the wave's rows
        // (a base is at most i0 + 32 — the row's window begins in the block's second half — so from chunk 1 on no difference
        // below is negative; chunk 0, the block's own tile, always runs)
        for (uint64_t c0 = 0; c0 == 0 || (i0 + 64u * c0 - prune_mask_base(i_last, lag)) / 32u < pitch; c0 += kPrChunks) {
            float v[kPrChunks][kPrRowsPerWave];
            bool ok[kPrChunks][kPrRowsPerWave];
#pragma unroll
            for (uint32_t u = 0; u < kPrChunks; ++u) {
                const uint64_t j = i0 + 64u * (c0 + u) + lane;
                const uint64_t lo_j = (WIN && j < n) ? (uint64_t)lo[j] : 0u;
#pragma unroll
                for (uint32_t k = 0; k < kPrRowsPerWave; ++k) {
                    const uint64_t i = i0 + wave * kPrRowsPerWave + k;
                    ok[u][k] = j < n && j > i && j - i - 1u < lag && (!WIN || (j <= (uint64_t)hi[i] && i >= lo_j));
                    v[u][k] = vals[ok[u][k] ? i * ld + (j - i - 1u) : 0u];
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < kPrChunks; ++u) {
#pragma unroll
                for (uint32_t k = 0; k < kPrRowsPerWave; ++k) {
                    const uint64_t i = i0 + wave * kPrRowsPerWave + k;
                    const uint64_t bits = __ballot(ok[u][k] && prune_edge(v[u][k], min_r2));
                    if (c0 + u == 0) {   // the block's own tile: wave 0 adds the bits behind the row below
                        if (lane == 0) s_fwd[wave * kPrRowsPerWave + k] = bits;
                        continue;
                    }
                    const uint64_t w = (i0 + 64u * (c0 + u) - prune_mask_base(i, lag)) / 32u + (lane & 1u);
                    if (lane < 2 && i < n && w < pitch) masks[i * pitch + w] = (uint32_t)(bits >> (32u * lane));
                }
            }
        }
    }
    __syncthreads();

    // ---- the block's own tile: the bits behind row i are the bits i of the rows before it
    if (wave == 0) {
        const uint64_t i = i0 + lane;
        uint64_t bits = s_fwd[lane];
        for (uint32_t j = 0; j < kPrRows; ++j) {
            const uint64_t f = s_fwd[j];   // (one address for the whole wave)
            bits |= j < lane ? ((f >> lane) & 1ull) << j : 0ull;
        }
        if (i < n) {
            const uint64_t base_i = prune_mask_base(i, lag);
            if (base_i <= i0) {
                const uint64_t w = (i0 - base_i) / 32u;   // (w + 1 <= ceil(lag / 32) + 1 < pitch)
                masks[i * pitch + w] = (uint32_t)bits;
                masks[i * pitch + w + 1u] = (uint32_t)(bits >> 32);
            } else {   // base_i = i0 + 32: the mask begins with the tile's second half (the first is more than lag behind: 0)
                masks[i * pitch] = (uint32_t)(bits >> 32);
            }
        }
    }
}

constexpr uint32_t kMisMaxRows = 1u << 20;               // the removed bits of all rows in the LDS: 128 KiB of the CU's 160
constexpr uint32_t kMisWaves = 16;
constexpr uint32_t kMisThreads = kMisWaves * kLanes;     // 1024
constexpr uint32_t kMisGather = 32;                      // adjacency words a lane has in flight before it uses the first

// keep[r] = 1 when row r is in the lexicographically first maximal independent set under `order` (NULL: row order), else 0.
// ONE workgroup; s_removed holds a bit per row: "a kept row is adjacent to it". Per batch of 64 rows of the order:
//   wave 0 — lane t takes r = order[b + t] and its removed bit; the ballot gives the candidates. Lane t then reads, from
//     its own row's mask, the bit of every other candidate of the batch (32 loads in flight): adj, the 64 x 64 adjacency of
//     the batch, a 64-bit register per lane. The greedy over the batch runs on registers alone: the first candidate is kept,
//     its adj (v_readlane_b32) strikes its neighbours from the candidates, and so on — no memory round trip per kept row.
//     keep is stored for all 64 rows, the kept rows go to s_rows.
//   all waves — wave w ORs the masks of the kept rows w, w + 16, .. into s_removed (ds_or_b32, a word per lane; the masks
//     are aligned to absolute rows: word k of row r is word base(r) / 32 + k of the state).
// Two barriers per batch; the kernel waits for no other workgroup. A removed row costs its share of one batch, a kept row
// pitch / 64 loads of one wave more.
__global__ __launch_bounds__(kMisThreads) void band_mis_resolve_kernel(const uint32_t* __restrict__ masks, uint32_t pitch, uint64_t n,
                                                                       uint64_t lag, const uint32_t* __restrict__ order,
                                                                       uint8_t* __restrict__ keep) {
    __shared__ uint32_t s_removed[kMisMaxRows / 32u];
    __shared__ uint32_t s_rows[kLanes];
    __shared__ uint32_t s_n;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t n_words = (uint32_t)((n + 31u) / 32u);   // (n <= kMisMaxRows: the launcher refuses more)
    for (uint32_t w = threadIdx.x; w < n_words; w += kMisThreads) s_removed[w] = 0u;
    __syncthreads();

    for (uint64_t b = 0; b < n; b += kLanes) {
        if (wave == 0) {
            const bool valid = b + lane < n;
            const uint32_t r = valid ? (order ? order[b + lane] : (uint32_t)(b + lane)) : 0u;
            const bool free_row = valid && ((s_removed[r >> 5] >> (r & 31u)) & 1u) == 0u;
            const uint64_t cand = __ballot(free_row);
            const uint64_t base_r = prune_mask_base(r, lag);
            uint64_t adj = 0;
            for (uint32_t u0 = 0; u0 < (uint32_t)kLanes; u0 += kMisGather) {
                if (((cand >> u0) & ((1ull << kMisGather) - 1ull)) == 0ull) continue;   // (uniform)
                uint32_t word[kMisGather];
#pragma unroll
                for (uint32_t q = 0; q < kMisGather; ++q) {
                    const uint32_t ru = (uint32_t)__shfl((int)r, (int)(u0 + q));
                    const bool in = free_row && ((cand >> (u0 + q)) & 1ull) && ru >= base_r && (ru - base_r) / 32u < pitch;
                    word[q] = in ? masks[(uint64_t)r * pitch + (ru - base_r) / 32u] : 0u;
                }
#pragma unroll
                for (uint32_t q = 0; q < kMisGather; ++q) {
                    const uint32_t ru = (uint32_t)__shfl((int)r, (int)(u0 + q));
                    adj |= (uint64_t)((word[q] >> (ru & 31u)) & 1u) << (u0 + q);
                }
            }
            uint64_t kept = 0;
            for (uint64_t c = cand; c;) {   // (scalar: c comes from a ballot and from v_readlane of one lane's registers)
                const int k = __builtin_amdgcn_readfirstlane(__builtin_ctzll(c));
                kept |= 1ull << k;
                const uint32_t a_lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)adj, k);
                const uint32_t a_hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(adj >> 32), k);
                c &= ~(((uint64_t)a_hi << 32) | a_lo | (1ull << k));
            }
            const bool mine = (kept >> lane) & 1ull;
            if (valid) keep[r] = mine ? 1 : 0;
            if (mine) s_rows[__popcll(kept & ((1ull << lane) - 1ull))] = r;
            if (lane == 0) s_n = (uint32_t)__popcll(kept);
        }
        __syncthreads();
        const uint32_t n_kept = s_n;
        for (uint32_t k = wave; k < n_kept; k += kMisWaves) {
            const uint32_t r = s_rows[k];
            const uint32_t w0 = (uint32_t)(prune_mask_base(r, lag) / 32u);
            for (uint32_t w = lane; w < pitch; w += kLanes) {
                if (w0 + w >= n_words) break;   // (words past the last row: 0, and no place in the state)
                const uint32_t x = masks[(uint64_t)r * pitch + w];
                if (x) atomicOr(&s_removed[w0 + w], x);
            }
        }
        __syncthreads();
    }
}

__global__ void band_mis_rank_kernel(const uint32_t* __restrict__ order, uint64_t n, uint32_t* __restrict__ rank) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) rank[order[k]] = (uint32_t)k;   // (order is a permutation: the launcher checked it)
}

// owner[v] = v for a kept row, else the kept neighbour that comes first in the order. One wave per row: a lane takes the
// words lane, lane + 64, .. of the row's mask, looks up the keep flag and the rank of every set bit, and the wave takes the
// smallest rank. A pure function of keep, the masks and the order. order / rank NULL: row order.
constexpr uint32_t kOwnWaves = 4;
__global__ __launch_bounds__(kOwnWaves* kLanes) void band_mis_owner_kernel(const uint32_t* __restrict__ masks, uint32_t pitch,
                                                                          uint64_t n, uint64_t lag,
                                                                          const uint8_t* __restrict__ keep,
                                                                          const uint32_t* __restrict__ order,
                                                                          const uint32_t* __restrict__ rank,
                                                                          uint32_t* __restrict__ owner) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t v = (uint64_t)blockIdx.x * kOwnWaves + wave;
    if (v >= n) return;   // (the whole wave)
    if (keep[v]) {
        if (lane == 0) owner[v] = (uint32_t)v;
        return;
    }
    const uint64_t base = prune_mask_base(v, lag);
    uint32_t best = 0xFFFFFFFFu;
    for (uint32_t w = lane; w < pitch; w += kLanes) {
        uint32_t x = masks[v * pitch + w];
        while (x) {
            const uint64_t j = base + 32u * w + (uint32_t)__builtin_ctz(x);
            x &= x - 1u;
            if (j < n && keep[j]) {
                const uint32_t rk = rank ? rank[j] : (uint32_t)j;
                best = rk < best ? rk : best;
            }
        }
    }
#pragma unroll
    for (int m = kLanes / 2; m >= 1; m >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)best, m);
        best = other < best ? other : best;
    }
    // (a removed row has a kept neighbour; were the masks not the resolver's, the row would own itself)
    if (lane == 0) owner[v] = best == 0xFFFFFFFFu ? (uint32_t)v : (order ? order[best] : best);
}

// what the prune calls refuse alike, behind their own NULL / max_lag / ld checks
int check_lag_band_prune(const char* who, uint64_t n_rows, const uint32_t* h_lo, const uint32_t* h_hi, float min_r2) {
    if (!h_lo != !h_hi) {
        set_error("%s: the window bounds lo and hi come together or not at all", who);
        return STORM_HIP_EINVAL;
    }
    if (n_rows > kMisMaxRows) {
        set_error("%s: %llu rows: the resolver keeps a bit per row in the LDS, at most %u rows", who, (unsigned long long)n_rows,
                  kMisMaxRows);
        return STORM_HIP_EINVAL;
    }
    if (min_r2 != min_r2) {
        set_error("%s: min_r2 is NaN", who);
        return STORM_HIP_EINVAL;
    }
    return STORM_HIP_OK;
}

// words of device scratch behind which nothing is touched: the masks, lo and hi, order and rank
size_t lag_band_prune_scratch_words(uint64_t n_rows, uint64_t lag, bool windows, bool order) {
    return (size_t)n_rows * prune_mask_pitch(lag) + (windows ? 2 * n_rows : 0) + (order ? 2 * n_rows : 0);
}

// the kernels over a band in device memory with their scratch at d_scratch, queued on the context's stream (n_rows >= 2,
// lag = min(max_lag, n_rows - 1) >= 1, check_lag_band_prune passed)
int launch_lag_band_prune(storm_hip_ctx_t* ctx, const char* who, const float* d_vals, uint64_t ld, uint64_t n_rows, uint64_t lag,
                          float min_r2, const uint32_t* h_lo, const uint32_t* h_hi, const uint32_t* h_order, uint8_t* d_keep,
                          uint32_t* d_owner, uint32_t* d_scratch) {
    const uint64_t n = n_rows;
    if (h_order) {   // a value out of range or twice would send the kernels out of their arrays
        std::vector<bool> seen(n, false);
        for (uint64_t k = 0; k < n; ++k) {
            if (h_order[k] >= n || seen[h_order[k]]) {
                set_error("%s: order[%llu] = %u: the order is not a permutation of the %llu rows", who, (unsigned long long)k,
                          h_order[k], (unsigned long long)n);
                return STORM_HIP_EINVAL;
            }
            seen[h_order[k]] = true;
        }
    }
    const uint32_t pitch = (uint32_t)prune_mask_pitch(lag);
    uint32_t* const d_masks = d_scratch;
    uint32_t* const d_lo = h_lo ? d_masks + (size_t)n * pitch : nullptr;
    uint32_t* const d_hi = h_lo ? d_lo + n : nullptr;
    uint32_t* const d_order = h_order ? d_masks + (size_t)n * pitch + (h_lo ? 2 * n : 0) : nullptr;
    uint32_t* const d_rank = h_order ? d_order + n : nullptr;
    STORM_HIP_TRY(hipSetDevice(ctx->device));
    if (h_lo) {
        STORM_HIP_TRY(hipMemcpyAsync(d_lo, h_lo, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
        STORM_HIP_TRY(hipMemcpyAsync(d_hi, h_hi, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    }
    if (h_order) STORM_HIP_TRY(hipMemcpyAsync(d_order, h_order, n * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    const uint32_t blocks = (uint32_t)((n + kPrRows - 1) / kPrRows);
    hipLaunchKernelGGL(h_lo ? lag_band_threshold_kernel<true> : lag_band_threshold_kernel<false>, dim3(blocks), dim3(kPrThreads), 0,
                       ctx->stream, d_vals, ld, n, lag, min_r2, d_lo, d_hi, d_masks, pitch);
    STORM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(band_mis_resolve_kernel, dim3(1), dim3(kMisThreads), 0, ctx->stream, d_masks, pitch, n, lag, d_order, d_keep);
    STORM_HIP_TRY(hipGetLastError());
    if (d_owner) {
        if (h_order) {
            hipLaunchKernelGGL(band_mis_rank_kernel, dim3((uint32_t)((n + 255u) / 256u)), dim3(256), 0, ctx->stream, d_order, n, d_rank);
            STORM_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(band_mis_owner_kernel, dim3((uint32_t)((n + kOwnWaves - 1) / kOwnWaves)), dim3(kOwnWaves * kLanes), 0,
                           ctx->stream, d_masks, pitch, n, lag, d_keep, d_order, d_rank, d_owner);
        STORM_HIP_TRY(hipGetLastError());
    }
    return STORM_HIP_OK;
}

}  // namespace storm

using namespace storm;

extern "C" int storm_hip_lag_band_prune_device(storm_hip_ctx_t* ctx, const float* d_vals, uint64_t ld, uint64_t n_rows,
                                               uint64_t max_lag, float min_r2, const uint32_t* h_lo, const uint32_t* h_hi,
                                               const uint32_t* h_order, uint8_t* d_keep, uint32_t* d_owner) {
    return guarded("storm_hip_lag_band_prune_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        if (!d_vals || !d_keep || max_lag == 0) {
            set_error("lag_band_prune: NULL argument or max_lag 0");
            return STORM_HIP_EINVAL;
        }
        const uint64_t lag = n_rows ? std::min(max_lag, n_rows - 1) : 0;
        if (ld < lag) {
            set_error("lag_band_prune: leading dimension %llu < min(max_lag, rows - 1) = %llu", (unsigned long long)ld,
                      (unsigned long long)lag);
            return STORM_HIP_EINVAL;
        }
        if (int rc = check_lag_band_prune("lag_band_prune", n_rows, h_lo, h_hi, min_r2)) return rc;
        if (n_rows < 2) return STORM_HIP_OK;
        STORM_HIP_TRY(hipSetDevice(ctx->device));
        const size_t words = lag_band_prune_scratch_words(n_rows, lag, h_lo != nullptr, h_order != nullptr);
        if (int rc = ctx->d_band.ensure(words * sizeof(uint32_t), "lag_band_prune: the adjacency masks, windows and order")) return rc;
        return launch_lag_band_prune(ctx, "lag_band_prune", d_vals, ld, n_rows, lag, min_r2, h_lo, h_hi, h_order, d_keep, d_owner,
                                     ctx->d_band.d);
    });
}
