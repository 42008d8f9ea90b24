// storm_hip_ldscore.hip — per-row sums over a float matrix in the lag layout, reduced where the matrix lies: the LD score
// of a variant is the sum of r^2 over the rows within max_lag on BOTH sides of it (storm.h: STORM_dosage_lag_ldscore), and
// lag_band_sums_kernel forms it for every row from the n x L band the lag calls write: n floats and n counts leave the
// device instead of n x L. The band is read twice, 4 bytes per entry each time, and never written; a
// pair's term is storm_ldscore_math.h's line. No atomics and no clearing launch: every row's sum is put together in one
// fixed order, so two calls on the same band return the same bits.
#include "storm_hip_internal.h"
#include "storm_ldscore_math.h"

namespace storm {

constexpr uint32_t kLdRows = 64;                          // a workgroup owns 64 consecutive rows: lane t of every wave, row i0 + t
constexpr uint32_t kLdWaves = 16;                         // ... and 16 waves share the two sweeps over what those rows read
constexpr uint32_t kLdThreads = kLdWaves * kLanes;        // 1024
constexpr uint32_t kLdRowsPerWave = kLdRows / kLdWaves;   // forward sweep: 4 whole rows per wave
constexpr uint32_t kLdBatch = 8;                          // loads a lane has in flight before it uses the first
static_assert(kLdRows == (uint32_t)kLanes && kLdRows % kLdWaves == 0, "one lane per row in the backward sweep");
static_assert(kLdBatch % kLdRowsPerWave == 0, "a forward step is whole rows");

// score[i] = the sum of the terms of the pairs (i, j), 1 <= |i - j| <= lag, n_pairs[i] = how many were summed (a pair whose
// entry is NaN, or that has no N - 2 under the adjusted statistic, is not: ldscore_term). vals: n rows of pitch ld, the
// pair (i, i + 1 + d) at vals[i * ld + d].
//   backward sweep — the pairs (j, i), j < i: for a source row j the 64 rows of the workgroup read the 64 CONSECUTIVE lags
//     d = i0 - j - 1 + t of row j: lane t owns row i0 + t, consecutive lanes read consecutive words, nothing is transposed.
//     Wave w takes the rows j = j_lo + w, j_lo + w + 16, ... of [max(i0 - lag, 0), min(i0 + 63, n - 1)); a lane is masked
//     where d < 0, d >= lag or its row is behind n. Each lane keeps its row's partial sum as a double in a register.
//   forward sweep — the pairs (i, j), j > i: wave w takes rows i0 + 4 w .. i0 + 4 w + 3, side by side, its lanes run
//     across d < min(lag, n - 1 - i), and the 64 partial sums meet in a butterfly (xor 32, 16, .. 1: every lane holds the same
//     sum in the same order of additions). Either sweep loads 8 entries per lane before it uses the first.
//   Then the LDS: wave w leaves its backward partials at s_sum[w][t] — 64 consecutive doubles, ds_write_b64 / ds_read_b64
//     take a half-wave per cycle over all 64 banks: no conflict — and the forward sums at s_fwd[row]; lane t of wave 0 adds
//     forward, then waves 0 .. 15 in that order, rounds once to float and stores the float and the count.
// Nothing of vals is read where d >= lag or i + 1 + d >= n (the pitch columns and the lower-right corner hold whatever
// the buffer held), and nothing of nobs where vals is not: a masked lane reads the entry of a pair that exists.
// STAT and NOBS (N from the view, not the constant) are template arguments: no branch on them between the loads.
template <int STAT, bool NOBS>
__global__ __launch_bounds__(kLdThreads) void lag_band_sums_kernel(const float* __restrict__ vals, uint64_t ld, uint64_t n,
                                                                   uint64_t lag, uint64_t n_const,
                                                                   const uint32_t* __restrict__ nobs, uint64_t nobs_row_pitch,
                                                                   uint64_t nobs_col_stride, float* __restrict__ score,
                                                                   uint32_t* __restrict__ n_pairs) {
    __shared__ double s_sum[kLdWaves][kLdRows];
    __shared__ uint32_t s_cnt[kLdWaves][kLdRows];
    __shared__ double s_fwd[kLdRows];
    __shared__ uint32_t s_fwd_cnt[kLdRows];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint64_t i0 = (uint64_t)blockIdx.x * kLdRows;
    // A step loads kLdBatch entries per lane, all of them before the first is used. A masked lane loads entry (row, 0) of
    // a row the step does visit — the pair (row, row + 1), which exists — and gets NaN for it: no load waits for a
    // predicate, and the corner and the pitch columns are never read.
    const float kNaN = __builtin_nanf("");
    auto add = [](float v, uint64_t N, double& sum, uint32_t& cnt) {
        double t = 0.0;
        const bool summed = ldscore_term(v, STAT, N, &t);
        sum += summed ? t : 0.0;   // (+0.0 leaves the sum's bits as they are)
        cnt += summed ? 1u : 0u;
    };

    // ---- backward: row i = i0 + lane gathers column i of the rows before it
    {
        const uint64_t i = i0 + lane;
        const uint64_t j_lo = i0 > lag ? i0 - lag : 0, j_hi = i0 + kLdRows - 1u < n - 1u ? i0 + kLdRows - 1u : n - 1u;
        double sum = 0.0;
        uint32_t cnt = 0;
        for (uint64_t j0 = j_lo + wave; j0 < j_hi; j0 += kLdBatch * kLdWaves) {
            float v[kLdBatch];
            uint32_t N[kLdBatch];
#pragma unroll
            for (uint32_t u = 0; u < kLdBatch; ++u) {
                const uint64_t j = j0 + u * kLdWaves;
                const bool ok = j < j_hi && i < n && j < i && i - j - 1u < lag;
                const uint64_t row = j < j_hi ? j : j0, d = ok ? i - j - 1u : 0u;
                const float x = vals[row * ld + d];
                if (NOBS) N[u] = (uint32_t)ldscore_nobs_at(nobs, nobs_row_pitch, nobs_col_stride, row, d);
                v[u] = ok ? x : kNaN;
            }
#pragma unroll
            for (uint32_t u = 0; u < kLdBatch; ++u) add(v[u], NOBS ? (uint64_t)N[u] : n_const, sum, cnt);
        }
        s_sum[wave][lane] = sum;
        s_cnt[wave][lane] = cnt;
    }

    // ---- forward: a whole wave along each of its rows, the four rows side by side, two steps of 64 lags at a time
    {
        double sum[kLdRowsPerWave];
        uint32_t cnt[kLdRowsPerWave];
        uint64_t d_end[kLdRowsPerWave], d_max = 0;
#pragma unroll
        for (uint32_t k = 0; k < kLdRowsPerWave; ++k) {
            const uint64_t i = i0 + wave * kLdRowsPerWave + k;
            sum[k] = 0.0;
            cnt[k] = 0;
            d_end[k] = i + 1u < n ? (lag < n - 1u - i ? lag : n - 1u - i) : 0u;   // 0: the last row, or one behind it
            d_max = d_end[k] > d_max ? d_end[k] : d_max;
        }
        // (d_max > 0 only if the wave's first row has a pair ahead: d_end falls with k, so row 0 is the one to fall back on)
        constexpr uint32_t kSteps = kLdBatch / kLdRowsPerWave;
        for (uint64_t d0 = 0; d0 < d_max; d0 += kSteps * kLanes) {
            float v[kSteps][kLdRowsPerWave];
            uint32_t N[kSteps][kLdRowsPerWave];
#pragma unroll
            for (uint32_t u = 0; u < kSteps; ++u) {
#pragma unroll
                for (uint32_t k = 0; k < kLdRowsPerWave; ++k) {
                    const uint64_t d1 = d0 + u * kLanes + lane;
                    const bool ok = d1 < d_end[k];
                    const uint64_t row = i0 + wave * kLdRowsPerWave + (d_end[k] ? k : 0u), d = ok ? d1 : 0u;
                    const float x = vals[row * ld + d];
                    if (NOBS) N[u][k] = (uint32_t)ldscore_nobs_at(nobs, nobs_row_pitch, nobs_col_stride, row, d);
                    v[u][k] = ok ? x : kNaN;
                }
            }
#pragma unroll
            for (uint32_t u = 0; u < kSteps; ++u) {
#pragma unroll
                for (uint32_t k = 0; k < kLdRowsPerWave; ++k) add(v[u][k], NOBS ? (uint64_t)N[u][k] : n_const, sum[k], cnt[k]);
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kLdRowsPerWave; ++k) {
#pragma unroll
            for (int m = kLanes / 2; m >= 1; m >>= 1) {
                sum[k] += __shfl_xor(sum[k], m);
                cnt[k] += __shfl_xor(cnt[k], m);
            }
            if (lane == 0) {
                s_fwd[wave * kLdRowsPerWave + k] = sum[k];
                s_fwd_cnt[wave * kLdRowsPerWave + k] = cnt[k];
            }
        }
    }
    __syncthreads();

    // ---- one lane per row: forward, then the waves' backward partials in their order
    if (wave == 0 && i0 + lane < n) {
        double sum = s_fwd[lane];
        uint32_t cnt = s_fwd_cnt[lane];
#pragma unroll
        for (uint32_t w = 0; w < kLdWaves; ++w) {
            sum += s_sum[w][lane];
            cnt += s_cnt[w][lane];
        }
        score[i0 + lane] = (float)sum;
        if (n_pairs) n_pairs[i0 + lane] = cnt;
    }
}

// the kernel over a band in device memory, queued on the context's stream (the checks of storm_hip_lag_band_sums_device)
int launch_lag_band_sums(storm_hip_ctx_t* ctx, const float* d_vals, uint64_t ld, uint64_t n_rows, uint64_t max_lag, int stat,
                         uint64_t n_const, const uint32_t* d_nobs, uint64_t nobs_row_pitch, uint64_t nobs_col_stride,
                         float* d_score, uint32_t* d_n_pairs) {
    if (!d_vals || !d_score || max_lag == 0) {
        set_error("lag_band_sums: NULL argument or max_lag 0");
        return STORM_HIP_EINVAL;
    }
    if (stat != STORM_HIP_LDSCORE_R2 && stat != STORM_HIP_LDSCORE_R2_ADJ) {
        set_error("lag_band_sums: unknown stat %d (0 r^2, 1 r^2 adjusted)", stat);
        return STORM_HIP_EINVAL;
    }
    const uint64_t lag = n_rows ? std::min(max_lag, n_rows - 1) : 0;
    if (ld < lag) {
        set_error("lag_band_sums: leading dimension %llu < min(max_lag, rows - 1) = %llu", (unsigned long long)ld,
                  (unsigned long long)lag);
        return STORM_HIP_EINVAL;
    }
    if (n_rows < 2) return STORM_HIP_OK;
    const uint64_t blocks = (n_rows + kLdRows - 1) / kLdRows;
    if (blocks > 0x7fffffffu) {
        set_error("lag_band_sums: %llu rows exceed the launch grid", (unsigned long long)n_rows);
        return STORM_HIP_EINVAL;
    }
    STORM_HIP_TRY(hipSetDevice(ctx->device));
    // (the unadjusted statistic does not read N: one instantiation)
    auto* const kernel = stat == STORM_HIP_LDSCORE_R2 ? lag_band_sums_kernel<kLdscoreR2, false>
                         : d_nobs                      ? lag_band_sums_kernel<kLdscoreR2Adj, true>
                                                       : lag_band_sums_kernel<kLdscoreR2Adj, false>;
    hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(kLdThreads), 0, ctx->stream, d_vals, ld, n_rows, lag, n_const, d_nobs,
                       nobs_row_pitch, nobs_col_stride, d_score, d_n_pairs);
    STORM_HIP_TRY(hipGetLastError());
    return STORM_HIP_OK;
}

}  // namespace storm

using namespace storm;

extern "C" int storm_hip_lag_band_sums_device(storm_hip_ctx_t* ctx, const float* d_vals, uint64_t ld, uint64_t n_rows,
                                              uint64_t max_lag, int stat, uint64_t n_const, const uint32_t* d_nobs,
                                              uint64_t nobs_row_pitch, uint64_t nobs_col_stride, float* d_score,
                                              uint32_t* d_n_pairs) {
    return guarded("storm_hip_lag_band_sums_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return launch_lag_band_sums(ctx, d_vals, ld, n_rows, max_lag, stat, n_const, d_nobs, nobs_row_pitch, nobs_col_stride, d_score,
                                    d_n_pairs);
    });
}
