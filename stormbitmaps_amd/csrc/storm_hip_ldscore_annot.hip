// storm_hip_ldscore_annot.hip — stratified LD scores: the band of a float matrix in the lag layout times an annotation
// matrix, with a window per row (storm.h: STORM_dosage_lag_ldscore_annot). score[i, c] = the sum over the rows j of row i's
// window of t(i, j) a[j, c]: a band matrix times an n x C matrix, formed where the band lies — n x C floats and n counts
// leave the device instead of n x L. lag_band_sums_kernel (storm_hip_ldscore.hip) stays what the plain calls run; a pair's
// term and the line that adds it are storm_ldscore_math.h's. No atomics and no clearing launch: every (row, column) is put
// together in one fixed order that does not depend on the other columns of the call.
#include "storm_hip_internal.h"
#include "storm_ldscore_math.h"

#include <cstdlib>
#include <cstring>

namespace storm {

constexpr uint32_t kLaTile = 64;                          // a workgroup owns 64 consecutive rows x 64 annotation columns
constexpr uint32_t kLaWaves = 4;
constexpr uint32_t kLaThreads = kLaWaves * kLanes;        // 256: a thread holds 4 rows x 4 columns of the product
constexpr uint32_t kLaPer = kLaTile / kLaWaves;           // 16 entries a lane loads per tile and side, all before the first use
constexpr uint32_t kLaPitch = kLaTile + 2;                // doubles per source row of the term tile (below)
static_assert(kLaTile == (uint32_t)kLanes, "one lane per row (behind) or per source row (ahead)");

// score[i * score_ld + c] = (float) sum over j in [lo[i], hi[i]], j != i, |i - j| <= lag, pair summed, of t(i, j) a[j * annot_ld + c];
// n_pairs[i] = how many pairs were summed (ldscore_term: not a NaN entry, not N < 3 under the adjusted statistic). vals: n
// rows of pitch ld, the pair (i, i + 1 + d) at vals[i * ld + d]. lo / hi NULL: the whole lag. The windows are symmetric
// (j in W(i) <=> i in W(j): storm_ldscore_window.h), so "j in W(i)" is lo[i] <= j behind the row and j <= hi[i] ahead of it.
//   Workgroup (x, y): rows [64 x, 64 x + 64), columns [64 y, 64 y + 64). It sweeps the source rows j in tiles of 64 aligned to
//   multiples of 64, from max(i0 - lag, 0) to min(i0 + 63 + lag, n - 1): every tile lies wholly behind the row block, on it,
//   or wholly ahead of it. Per tile:
//   terms  — the 64 x 64 terms go to the LDS once, as doubles, s_t[j][i] with +0.0 where the pair is not summed (statistic,
//     NaN rule, lag and window applied here). A tile behind the block is loaded as lag_band_sums_kernel's backward sweep
//     loads: lane t owns row i0 + t and reads the 64 consecutive lags d = i - j - 1 of ONE source row j (wave w: rows w,
//     w + 4, ..); it writes 64 consecutive doubles. A tile ahead is loaded as the forward sweep loads: the wave runs along
//     row i (wave w: rows 16 w .. 16 w + 15), lane t reads d = jt + t - i - 1; it writes a column of s_t, pitch 66 doubles
//     = 132 banks' words: lane t starts at bank 4 t mod 64, two lanes of a half-wave per bank pair (a pitch of 65 would be
//     conflict-free but breaks the 16-byte alignment of the product's reads). The tile on the block does both: behind
//     writes j < i, ahead j >= i (the diagonal: +0.0). A lane loads its 16 entries (and their N) before it uses the first.
//     A masked lane reads entry (0, 0) — the pair (0, 1), which exists — and gets NaN for it: no load waits for a
//     predicate; nothing of the lower-right corner or the pitch columns of vals is read, and nothing of nobs where vals is
//     not.
//   annotations — a[jt .. jt + 63][c0 .. c0 + 63] to the LDS as floats, lanes along the columns; 0 for rows behind n and
//     columns behind n_annot, which are never loaded.
//   product — thread (ty, tx) = (tid / 16, tid % 16) holds rows 4 ty .. + 3 x columns 4 tx .. + 3 as 16 doubles in registers
//     across the whole sweep; for j = 0 .. 63 in that order: 4 terms (one 32-byte LDS read, 4 addresses per wave), 4
//     annotations (one 16-byte read, 16 consecutive addresses) and 16 v_fma_f64 (ldscore_annot_add).
//   product, matrix core (MFMA = true) — wave w holds rows 16 w .. 16 w + 15 x all 64 columns as four 16 x 16 outputs of
//     v_mfma_f64_16x16x4_f64 (C/D: column lane & 15, row (lane >> 4) + 4 reg); per 4 source rows one A operand (a double per
//     lane: 16 consecutive doubles of 4 rows of s_t) and four B operands (a float per lane, widened exactly). The same sums
//     with the 4 source rows of a step added inside the instruction; which of the two ships: kLaShipsMfma below.
//   The order of additions of (i, c) is the tile sequence of i's block and j ascending within a tile: it does not depend on
//   c, the chunk, C or annot_ld, so a column gets the same bits whatever other columns are passed with it.
// Counts: behind, a lane counts its row's summed pairs; ahead, the wave's ballot counts row i's. Workgroups of y = 0
// store them. Rows at or behind n and columns at or behind n_annot are never stored; pitch elements of score are not touched.
typedef double LaAcc4 __attribute__((ext_vector_type(4)));   // the C/D operand of v_mfma_f64_16x16x4_f64

template <int STAT, bool NOBS, bool MFMA>
__global__ __launch_bounds__(kLaThreads) void lag_band_annot_sums_kernel(
    const float* __restrict__ vals, uint64_t ld, uint64_t n, uint64_t lag, uint64_t n_const, const uint32_t* __restrict__ nobs,
    uint64_t nobs_row_pitch, uint64_t nobs_col_stride, const uint32_t* __restrict__ lo, const uint32_t* __restrict__ hi,
    const float* __restrict__ annot, uint64_t annot_ld, uint64_t n_annot, float* __restrict__ score, uint64_t score_ld,
    uint32_t* __restrict__ n_pairs) {
    __shared__ __attribute__((aligned(16))) double s_t[kLaTile * kLaPitch];
    __shared__ __attribute__((aligned(16))) float s_a[kLaTile * kLaTile];
    __shared__ uint32_t s_hi[kLaTile];
    __shared__ uint32_t s_cnt[kLaWaves + 1][kLaTile];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint64_t i0 = (uint64_t)blockIdx.x * kLaTile, c0 = (uint64_t)blockIdx.y * kLaTile;
    const float kNaN = __builtin_nanf("");

    // the window of the lane's own row (behind) and of every row of the block (ahead: the wave reads its row's from the LDS)
    const uint64_t i_own = i0 + lane;
    const uint64_t lo_own = (lo && i_own < n) ? (uint64_t)lo[i_own] : 0u;
    if (wave == 0) s_hi[lane] = (hi && i_own < n) ? hi[i_own] : 0xFFFFFFFFu;

    auto term_of = [](float v, uint64_t N, bool* summed) {
        double t = 0.0;
        *summed = ldscore_term(v, STAT, N, &t);
        return *summed ? t : 0.0;
    };

    double acc[4][4];   // v_fma_f64: rows 4 ty + r x columns 4 tx + k
    LaAcc4 acc4[4];     // matrix core: column block cb, rows 16 wave + (lane >> 4) + 4 reg x column 16 cb + (lane & 15)
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
        acc4[r] = LaAcc4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) acc[r][k] = 0.0;
    }
    uint32_t cnt_behind = 0, cnt_ahead = 0;   // of row i0 + lane; of row i0 + 16 wave + lane (lanes 0 .. 15)
    const uint32_t ty = tid >> 4, tx = tid & 15u;

    const uint64_t j_first = (i0 > lag ? i0 - lag : 0u) / kLaTile * kLaTile;
    const uint64_t j_last = i0 + kLaTile - 1u + lag < n - 1u ? i0 + kLaTile - 1u + lag : n - 1u;
    for (uint64_t jt = j_first; jt <= j_last; jt += kLaTile) {
        __syncthreads();   // the product of the tile before has read s_t and s_a (first pass: s_hi is written)
        const bool diag = jt == i0;
        if (jt <= i0) {   // ---- behind (and the lower triangle of the tile on the block): lanes along the lags of one source row
            float v[kLaPer];
            uint32_t N[kLaPer];
#pragma unroll
            for (uint32_t u = 0; u < kLaPer; ++u) {
                const uint64_t j = jt + wave + u * kLaWaves;
                const bool ok = i_own < n && j < i_own && i_own - j - 1u < lag && j >= lo_own;
                const uint64_t row = ok ? j : 0u, d = ok ? i_own - j - 1u : 0u;
                const float x = vals[row * ld + d];
                if (NOBS) N[u] = (uint32_t)ldscore_nobs_at(nobs, nobs_row_pitch, nobs_col_stride, row, d);
                v[u] = ok ? x : kNaN;
            }
#pragma unroll
            for (uint32_t u = 0; u < kLaPer; ++u) {
                const uint32_t jl = wave + u * kLaWaves;
                bool summed;
                const double t = term_of(v[u], NOBS ? (uint64_t)N[u] : n_const, &summed);
                cnt_behind += summed ? 1u : 0u;
                if (!diag || jl < lane) s_t[jl * kLaPitch + lane] = t;
            }
        }
        if (jt >= i0) {   // ---- ahead (and the diagonal and upper triangle of the tile on the block): the wave along a row
            float v[kLaPer];
            uint32_t N[kLaPer];
            const uint64_t j = jt + lane;
#pragma unroll
            for (uint32_t u = 0; u < kLaPer; ++u) {
                const uint32_t il = wave * kLaPer + u;
                const uint64_t i = i0 + il;
                const bool ok = j < n && i < j && j - i - 1u < lag && j <= (uint64_t)s_hi[il];
                const uint64_t row = ok ? i : 0u, d = ok ? j - i - 1u : 0u;
                const float x = vals[row * ld + d];
                if (NOBS) N[u] = (uint32_t)ldscore_nobs_at(nobs, nobs_row_pitch, nobs_col_stride, row, d);
                v[u] = ok ? x : kNaN;
            }
#pragma unroll
            for (uint32_t u = 0; u < kLaPer; ++u) {
                const uint32_t il = wave * kLaPer + u;
                bool summed;
                const double t = term_of(v[u], NOBS ? (uint64_t)N[u] : n_const, &summed);
                const uint32_t row_cnt = (uint32_t)__popcll(__ballot(summed));
                cnt_ahead += lane == u ? row_cnt : 0u;
                if (!diag || lane >= il) s_t[lane * kLaPitch + il] = t;
            }
        }
        {   // ---- the annotations of the tile's source rows: lanes along the columns
            const uint64_t c = c0 + lane;
            float a[kLaPer];
#pragma unroll
            for (uint32_t u = 0; u < kLaPer; ++u) {
                const uint64_t j = jt + wave + u * kLaWaves;
                const bool ok = j < n && c < n_annot;
                const float x = annot[ok ? j * annot_ld + c : 0u];   // (entry (0, 0) exists: n >= 2, n_annot >= 1)
                a[u] = ok ? x : 0.0f;
            }
#pragma unroll
            for (uint32_t u = 0; u < kLaPer; ++u) s_a[(wave + u * kLaWaves) * kLaTile + lane] = a[u];
        }
        __syncthreads();
        // ---- 64 x 64 x 64: j ascending
        if constexpr (MFMA) {
            // wave w: rows 16 w .. 16 w + 15 x all 64 columns as four 16 x 16 outputs; per step of 4 source rows one A operand
            // (A[m = lane & 15][k = lane >> 4]: 16 consecutive doubles of each of 4 rows of s_t) and four B operands
            // (B[k = lane >> 4][n = lane & 15]: 16 consecutive floats, widened exactly)
            const uint32_t mn = lane & 15u, kq = lane >> 4;
#pragma unroll 4
            for (uint32_t k0 = 0; k0 < kLaTile; k0 += 4u) {
                const double a = s_t[(k0 + kq) * kLaPitch + 16u * wave + mn];
#pragma unroll
                for (uint32_t cb = 0; cb < 4; ++cb) {
                    const double b = (double)s_a[(k0 + kq) * kLaTile + 16u * cb + mn];
                    acc4[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc4[cb], 0, 0, 0);
                }
            }
        } else
#pragma unroll 4
        for (uint32_t jl = 0; jl < kLaTile; ++jl) {   // one fused multiply-add per (row, column, j)
            const double2 t01 = *reinterpret_cast<const double2*>(&s_t[jl * kLaPitch + 4u * ty]);
            const double2 t23 = *reinterpret_cast<const double2*>(&s_t[jl * kLaPitch + 4u * ty + 2u]);
            const float4 a4 = *reinterpret_cast<const float4*>(&s_a[jl * kLaTile + 4u * tx]);
            const double t[4] = {t01.x, t01.y, t23.x, t23.y};
            const float a[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
            for (uint32_t r = 0; r < 4; ++r)
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) acc[r][k] = ldscore_annot_add(acc[r][k], t[r], a[k]);
        }
    }

    // ---- one rounding to float; the counts once per row
#pragma unroll
    for (uint32_t r = 0; r < 4; ++r) {
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            // (matrix core: r is the column block, k the register of the C/D layout)
            const uint64_t i = MFMA ? i0 + 16u * wave + (lane >> 4) + 4u * k : i0 + 4u * ty + r;
            const uint64_t c = MFMA ? c0 + 16u * r + (lane & 15u) : c0 + 4u * tx + k;
            const double sum = MFMA ? acc4[r][k] : acc[r][k];
            if (i < n && c < n_annot) score[i * score_ld + c] = (float)sum;
        }
    }
    if (n_pairs && blockIdx.y == 0) {   // (uniform over the workgroup)
        s_cnt[wave][lane] = cnt_behind;
        if (lane < kLaPer) s_cnt[kLaWaves][wave * kLaPer + lane] = cnt_ahead;
        __syncthreads();
        if (wave == 0 && i_own < n) {
            uint32_t cnt = s_cnt[kLaWaves][lane];
#pragma unroll
            for (uint32_t w = 0; w < kLaWaves; ++w) cnt += s_cnt[w][lane];
            n_pairs[i_own] = cnt;
        }
    }
}

// The inner product: STORM_HIP_LDSCORE_ANNOT_INNER = fma | mfma, read at every launch (tools/bench_ldscore_annot.py times
// both in one process); anything else, or nothing: what ships (kLaShipsMfma, DESIGN.md §4 "Stratified LD scores").
constexpr bool kLaShipsMfma = true;    // 1.2 to 1.3 x the v_fma_f64 form at every bench shape (profiles/ldscore_annot.jsonl)
static bool annot_inner_is_mfma() {
    const char* const e = getenv("STORM_HIP_LDSCORE_ANNOT_INNER");
    if (e && !strcmp(e, "mfma")) return true;
    if (e && !strcmp(e, "fma")) return false;
    return kLaShipsMfma;
}

// the kernel over a band in device memory, queued on the context's stream (the checks of storm_hip_lag_band_annot_sums_device)
int launch_lag_band_annot_sums(storm_hip_ctx_t* ctx, const float* d_vals, uint64_t ld, uint64_t n_rows, uint64_t max_lag, int stat,
                               uint64_t n_const, const uint32_t* d_nobs, uint64_t nobs_row_pitch, uint64_t nobs_col_stride,
                               const uint32_t* d_lo, const uint32_t* d_hi, const float* d_annot, uint64_t annot_ld,
                               uint64_t n_annot, float* d_score, uint64_t score_ld, uint32_t* d_n_pairs) {
    if (!d_vals || !d_score || max_lag == 0) {
        set_error("lag_band_annot_sums: NULL argument or max_lag 0");
        return STORM_HIP_EINVAL;
    }
    if (stat != STORM_HIP_LDSCORE_R2 && stat != STORM_HIP_LDSCORE_R2_ADJ) {
        set_error("lag_band_annot_sums: unknown stat %d (0 r^2, 1 r^2 adjusted)", stat);
        return STORM_HIP_EINVAL;
    }
    const uint64_t lag = n_rows ? std::min(max_lag, n_rows - 1) : 0;
    if (ld < lag) {
        set_error("lag_band_annot_sums: leading dimension %llu < min(max_lag, rows - 1) = %llu", (unsigned long long)ld,
                  (unsigned long long)lag);
        return STORM_HIP_EINVAL;
    }
    if (!d_annot) {
        set_error("lag_band_annot_sums: NULL annotations");
        return STORM_HIP_EINVAL;
    }
    if (n_annot < 1 || n_annot > kLdscoreMaxAnnot) {
        set_error("lag_band_annot_sums: %llu annotation columns (1 .. %u)", (unsigned long long)n_annot, kLdscoreMaxAnnot);
        return STORM_HIP_EINVAL;
    }
    if (annot_ld < n_annot || score_ld < n_annot) {
        set_error("lag_band_annot_sums: annot_ld %llu or score_ld %llu < %llu annotation columns", (unsigned long long)annot_ld,
                  (unsigned long long)score_ld, (unsigned long long)n_annot);
        return STORM_HIP_EINVAL;
    }
    if (!d_lo != !d_hi) {
        set_error("lag_band_annot_sums: the window bounds lo and hi come together or not at all");
        return STORM_HIP_EINVAL;
    }
    if (n_rows < 2) return STORM_HIP_OK;
    const uint64_t blocks = (n_rows + kLaTile - 1) / kLaTile;
    if (blocks > 0x7fffffffu) {
        set_error("lag_band_annot_sums: %llu rows exceed the launch grid", (unsigned long long)n_rows);
        return STORM_HIP_EINVAL;
    }
    STORM_HIP_TRY(hipSetDevice(ctx->device));
    // (the unadjusted statistic does not read N: one instantiation per inner product)
    const bool mfma = annot_inner_is_mfma();
    auto* const kernel =
        stat == STORM_HIP_LDSCORE_R2 ? (mfma ? lag_band_annot_sums_kernel<kLdscoreR2, false, true> : lag_band_annot_sums_kernel<kLdscoreR2, false, false>)
        : d_nobs                     ? (mfma ? lag_band_annot_sums_kernel<kLdscoreR2Adj, true, true> : lag_band_annot_sums_kernel<kLdscoreR2Adj, true, false>)
                                     : (mfma ? lag_band_annot_sums_kernel<kLdscoreR2Adj, false, true> : lag_band_annot_sums_kernel<kLdscoreR2Adj, false, false>);
    const uint32_t chunks = (uint32_t)((n_annot + kLaTile - 1) / kLaTile);
    hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks, chunks), dim3(kLaThreads), 0, ctx->stream, d_vals, ld, n_rows, lag, n_const,
                       d_nobs, nobs_row_pitch, nobs_col_stride, d_lo, d_hi, d_annot, annot_ld, n_annot, d_score, score_ld,
                       d_n_pairs);
    STORM_HIP_TRY(hipGetLastError());
    return STORM_HIP_OK;
}

}  // namespace storm

using namespace storm;

extern "C" int storm_hip_lag_band_annot_sums_device(storm_hip_ctx_t* ctx, const float* d_vals, uint64_t ld, uint64_t n_rows,
                                                    uint64_t max_lag, int stat, uint64_t n_const, const uint32_t* d_nobs,
                                                    uint64_t nobs_row_pitch, uint64_t nobs_col_stride, const uint32_t* d_lo,
                                                    const uint32_t* d_hi, const float* d_annot, uint64_t annot_ld,
                                                    uint64_t n_annot, float* d_score, uint64_t score_ld, uint32_t* d_n_pairs) {
    return guarded("storm_hip_lag_band_annot_sums_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        return launch_lag_band_annot_sums(ctx, d_vals, ld, n_rows, max_lag, stat, n_const, d_nobs, nobs_row_pitch, nobs_col_stride,
                                          d_lo, d_hi, d_annot, annot_ld, n_annot, d_score, score_ld, d_n_pairs);
    });
}
