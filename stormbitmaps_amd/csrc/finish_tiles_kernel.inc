// finish_tiles_kernel.inc — the finishing pass of the per-pair statistics: a matrix of uint32 counts or dot products is
// overwritten in place with a float statistic of each entry and of its row's and its column's own sums (the same 4 bytes
// per entry; bound by HBM bandwidth, DESIGN.md §4 "Similarity finish"). Two kernels, one per layout, and one launcher for
// each; included by storm_hip_similarity.hip and storm_hip_dosage.hip, which bring the statistic as a policy
//
//   struct Stat {
//       static constexpr int W;                         // words of statistic per row, kept PLANAR: one array per word
//       static uint32_t bits(v, a[W], b[W], measure, scale);   // one entry: v with its row's words a and its column's b
//       static int check(who, measure, scale);          // what the launchers refuse of measure and scale
//   };
//
// (SimilarityStat: the row's count, similarity_bits; DosageStat: the row's sum and sum of squares, dosage_corr_bits).
//
// Both kernels: a workgroup of 4 waves takes kFinishTileRows x kFinishTileCols entries, a wave every 4th row, a lane 4
// adjacent entries. The loads of kFinishUnroll rows stand before the first divide (the rectangle's leave together; gfx950's
// compiler makes the triangle's and the lag layout's wait for one another). The rows' words go through the LDS, staged
// once per workgroup. vec: the base is 16-byte aligned and ld a multiple of 4, so a lane's 4 entries are one
// 128-bit access wherever all 4 are converted; the others (the diagonal's vector, the last columns, the edge of the lag
// layout's corner, everything of a misaligned matrix) go entry by entry. What is not converted is neither read nor written.

constexpr int kFinishTileRows = 64;    // a wave walks every 4th row of the tile ...
constexpr int kFinishTileCols = 256;   // ... one 128-bit vector (4 entries) per lane
constexpr int kFinishUnroll = 4;       // rows a wave has in flight

template <int W>
struct StatRow {   // the words of one row or column
    uint32_t w[W];
};

// A lane's 4 entries of one row at p: in one piece from v where `whole`, else those that keep(k) names; col(k): the words of
// entry k's column.
template <typename Stat, typename Col, typename Keep>
__device__ __forceinline__ void finish_entries(uint32_t* p, bool whole, const uint4& v, const uint32_t (&a)[Stat::W], Col col, Keep keep,
                                               int measure, uint64_t scale) {
    if (whole) {
        uint4 w;
        w.x = Stat::bits(v.x, a, col(0).w, measure, scale);
        w.y = Stat::bits(v.y, a, col(1).w, measure, scale);
        w.z = Stat::bits(v.z, a, col(2).w, measure, scale);
        w.w = Stat::bits(v.w, a, col(3).w, measure, scale);
        *reinterpret_cast<uint4*>(p) = w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (keep(k)) p[k] = Stat::bits(p[k], a, col(k).w, measure, scale);
    }
}

// The rectangle n_rows x n_cols, or (Triangle) its entries i < j alone: a tile at or below the diagonal exits at once, and
// entries i >= j are not touched; nor are the pitch columns [n_cols, ld). Grid (column tiles, row tiles). The words of a
// lane's 4 columns stay in registers.
template <typename Stat, bool Triangle>
__global__ __launch_bounds__(kThreads) void finish_tiles_kernel(uint32_t* __restrict__ io, uint64_t ld, uint64_t n_rows, uint64_t n_cols,
                                                                StatWords<Stat::W> rows, StatWords<Stat::W> cols, int measure,
                                                                uint64_t scale, int vec) {
    constexpr int W = Stat::W;
    const uint64_t row0 = (uint64_t)blockIdx.y * kFinishTileRows, col0 = (uint64_t)blockIdx.x * kFinishTileCols;
    if (Triangle && col0 + kFinishTileCols <= row0 + 1) return;   // the tile's last column is not beyond its first row
    __shared__ uint32_t s_rows[W][kFinishTileRows];
    if (threadIdx.x < kFinishTileRows) {
        const bool in = row0 + threadIdx.x < n_rows;
#pragma unroll
        for (int w = 0; w < W; ++w) s_rows[w][threadIdx.x] = in ? rows.w[w][row0 + threadIdx.x] : 0u;
    }
    const uint64_t c0 = col0 + (threadIdx.x & 63u) * 4u;
    uint32_t b[W][4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int w = 0; w < W; ++w) b[w][k] = c0 + k < n_cols ? cols.w[w][c0 + k] : 0u;
    __syncthreads();
    // The rectangle's `whole` is the same for every row and stays free of the row test: with the test folded in, as the
    // triangle has it, the compiler puts s_waitcnt vmcnt(0) in front of each row's load (the parent's triangle and lag
    // kernels carry those waits too), and the rectangle of 256 x 8192 dosage rows took 2.6 % longer
    // (profiles/finish_tiles_ab.txt). Without the test in the triangle's form its loads leave together as well, at 6 more
    // VGPRs and, for DosageStat, one wave per SIMD fewer than the kernel it replaces: not taken.
    const bool whole_cols = vec && c0 + 4 <= n_cols;
    const uint32_t wave = threadIdx.x >> 6;
    for (uint32_t r = wave; r < kFinishTileRows; r += 4 * kFinishUnroll) {
        uint4 v[kFinishUnroll];
        bool whole[kFinishUnroll];
#pragma unroll
        for (int u = 0; u < kFinishUnroll; ++u) {   // the loads of kFinishUnroll rows before the first divide
            const uint64_t i = row0 + r + 4u * u;
            whole[u] = Triangle ? whole_cols && i < n_rows && c0 > i : whole_cols;
            if (whole[u] && i < n_rows) v[u] = *reinterpret_cast<const uint4*>(io + i * ld + c0);
        }
#pragma unroll
        for (int u = 0; u < kFinishUnroll; ++u) {
            const uint64_t i = row0 + r + 4u * u;
            if (i >= n_rows) continue;
            uint32_t a[W];
#pragma unroll
            for (int w = 0; w < W; ++w) a[w] = s_rows[w][r + 4u * u];
            finish_entries<Stat>(
                io + i * ld + c0, whole[u], v[u], a,
                [&](int k) {
                    StatRow<W> c;
#pragma unroll
                    for (int w = 0; w < W; ++w) c.w[w] = b[w][k];
                    return c;
                },
                [&](int k) { return c0 + k < n_cols && (!Triangle || c0 + k > i); }, measure, scale);
        }
    }
}

// The LAG layout (storm_hip_pairw_lag_matrix_device): entry (r, d) of the band is the pair (i, i + 1 + d), i = row0 + r, for
// the rows [row0, band_end), so a tile reads the words of its 64 rows and of the 64 + 256 - 1 rows i0 + 1 + col0 .. behind
// them: both staged once per workgroup. Only entries with d < lag and i + 1 + d < n_rows are touched — not the lower-right
// corner, not the pitch columns.
template <typename Stat>
__global__ __launch_bounds__(kThreads) void finish_lag_tiles_kernel(uint32_t* __restrict__ io, uint64_t ld, uint64_t n_rows, uint64_t row0,
                                                                    uint64_t band_end, uint64_t lag, StatWords<Stat::W> stats,
                                                                    int measure, uint64_t scale, int vec) {
    constexpr int W = Stat::W;
    const uint64_t i0 = row0 + (uint64_t)blockIdx.y * kFinishTileRows, col0 = (uint64_t)blockIdx.x * kFinishTileCols;
    if (i0 + 1 + col0 >= n_rows) return;   // the tile's first pair is already in the corner
    __shared__ uint32_t s_rows[W][kFinishTileRows];
    __shared__ uint32_t s_cols[W][kFinishTileRows + kFinishTileCols];
    if (threadIdx.x < kFinishTileRows) {
        const bool in = i0 + threadIdx.x < band_end;
#pragma unroll
        for (int w = 0; w < W; ++w) s_rows[w][threadIdx.x] = in ? stats.w[w][i0 + threadIdx.x] : 0u;
    }
    for (uint32_t k = threadIdx.x; k < kFinishTileRows + kFinishTileCols; k += kThreads) {
        const bool in = i0 + 1 + col0 + k < n_rows;
#pragma unroll
        for (int w = 0; w < W; ++w) s_cols[w][k] = in ? stats.w[w][i0 + 1 + col0 + k] : 0u;
    }
    __syncthreads();
    const uint32_t lane4 = (threadIdx.x & 63u) * 4u;
    const uint64_t c0 = col0 + lane4;
    const uint32_t wave = threadIdx.x >> 6;
    for (uint32_t r = wave; r < kFinishTileRows; r += 4 * kFinishUnroll) {
        uint4 v[kFinishUnroll];
        bool whole[kFinishUnroll];
#pragma unroll
        for (int u = 0; u < kFinishUnroll; ++u) {   // the loads of kFinishUnroll rows leave before the first divide
            const uint64_t i = i0 + r + 4u * u;
            whole[u] = vec && i < band_end && c0 + 4 <= lag && i + 1 + c0 + 3 < n_rows;
            if (whole[u]) v[u] = *reinterpret_cast<const uint4*>(io + (i - row0) * ld + c0);
        }
#pragma unroll
        for (int u = 0; u < kFinishUnroll; ++u) {
            const uint32_t rr = r + 4u * u;
            const uint64_t i = i0 + rr;
            if (i >= band_end) continue;
            uint32_t a[W];
#pragma unroll
            for (int w = 0; w < W; ++w) a[w] = s_rows[w][rr];
            finish_entries<Stat>(
                io + (i - row0) * ld + c0, whole[u], v[u], a,
                [&](int k) {   // entry d = c0 + k: row i + 1 + c0 + k
                    StatRow<W> c;
#pragma unroll
                    for (int w = 0; w < W; ++w) c.w[w] = s_cols[w][rr + lane4 + k];
                    return c;
                },
                [&](int k) { return c0 + k < lag && i + 1 + c0 + k < n_rows; }, measure, scale);
        }
    }
}

// ---- the launchers (declared in storm_hip_internal.h): everything but Stat::check is the same for every statistic ----
// what both do once the shape is known: the grid, the vec rule, the launch on the context's stream, the report
template <typename Launch>
static int finish_tiles_queue(storm_hip_ctx_t* ctx, const char* who, void* d_io, uint64_t ld, uint64_t rows, uint64_t cols, Launch launch) {
    if (!finish_tiles_fit(rows, cols)) {
        set_error("%s: %llu x %llu entries exceed the launch grid", who, (unsigned long long)rows, (unsigned long long)cols);
        return STORM_HIP_EINVAL;
    }
    STORM_HIP_TRY(hipSetDevice(ctx->device));
    const dim3 grid((uint32_t)((cols + kFinishTileCols - 1) / kFinishTileCols), (uint32_t)((rows + kFinishTileRows - 1) / kFinishTileRows));
    launch(grid, reinterpret_cast<uintptr_t>(d_io) % 16 == 0 && ld % 4 == 0);
    STORM_HIP_TRY(hipGetLastError());
    ctx->pass_report[0] |= STORM_HIP_RAN_SIMILARITY;
    return STORM_HIP_OK;
}

template <typename Stat>
int launch_finish_tiles(storm_hip_ctx_t* ctx, const char* who, void* d_io, uint64_t ld, uint64_t n_rows, uint64_t n_cols,
                        StatWords<Stat::W> rows, StatWords<Stat::W> cols, bool triangle, int measure, uint64_t scale) {
    if (!d_io || !rows.all() || !cols.all()) {
        set_error("%s: NULL argument", who);
        return STORM_HIP_EINVAL;
    }
    if (int rc = Stat::check(who, measure, scale)) return rc;
    if (ld < n_cols || (triangle && n_rows != n_cols)) {
        set_error("%s: leading dimension < columns, or a triangle that is not square", who);
        return STORM_HIP_EINVAL;
    }
    if (n_rows == 0 || n_cols == 0) return STORM_HIP_OK;
    return finish_tiles_queue(ctx, who, d_io, ld, n_rows, n_cols, [&](dim3 grid, int vec) {
        const auto kernel = triangle ? finish_tiles_kernel<Stat, true> : finish_tiles_kernel<Stat, false>;
        hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, ctx->stream, static_cast<uint32_t*>(d_io), ld, n_rows, n_cols, rows, cols,
                           measure, scale, vec);
    });
}

template <typename Stat>
int launch_finish_lag_tiles(storm_hip_ctx_t* ctx, const char* who, void* d_io, uint64_t ld, uint64_t n_rows, uint64_t row0,
                            uint64_t n_band_rows, uint64_t max_lag, StatWords<Stat::W> stats, int measure, uint64_t scale) {
    if (!d_io || !stats.all()) {
        set_error("%s: NULL argument", who);
        return STORM_HIP_EINVAL;
    }
    if (int rc = Stat::check(who, measure, scale)) return rc;
    if (n_band_rows == ~0ull && row0 <= n_rows) n_band_rows = n_rows - row0;
    const uint64_t lag = n_rows ? std::min(max_lag, n_rows - 1) : 0;
    if (max_lag == 0 || row0 > n_rows || n_band_rows > n_rows - row0 || ld < lag) {
        set_error("%s: max_lag 0, a band outside the rows, or leading dimension < min(max_lag, rows - 1)", who);
        return STORM_HIP_EINVAL;
    }
    if (n_rows < 2 || n_band_rows == 0) return STORM_HIP_OK;
    return finish_tiles_queue(ctx, who, d_io, ld, n_band_rows, lag, [&](dim3 grid, int vec) {
        hipLaunchKernelGGL(finish_lag_tiles_kernel<Stat>, grid, dim3(kThreads), 0, ctx->stream, static_cast<uint32_t*>(d_io), ld, n_rows,
                           row0, row0 + n_band_rows, lag, stats, measure, scale, vec);
    });
}
