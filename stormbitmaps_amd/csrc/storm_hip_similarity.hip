// storm_hip_similarity.hip — the per-pair matrix finished where the counts lie: one pass that overwrites a matrix of
// intersection counts (uint32, what every matrix-output path of this library writes) with a similarity statistic
// (float, the same 4 bytes per entry): Jaccard, cosine (Ochiai), and the two linkage-disequilibrium measures D and r^2
// the reference names as the purpose of the per-pair counts (README.md:165-167).
//
// A separate launch on the context's stream, not an epilogue of the count kernels: those finish an entry in different
// places (k-parts that add into a cleared window, counts that are complete only at the end of a launch), and a
// non-linear formula is right only on complete counts. 4 bytes read and 4 written per converted entry: the pass is
// bound by HBM bandwidth. The kernels and their launchers are finish_tiles_kernel.inc, shared with the dosage
// statistics (storm_hip_dosage.hip): finish_tiles_kernel<SimilarityStat, triangle> over a rectangle or an upper triangle,
// finish_lag_tiles_kernel<SimilarityStat> over the lag layout.
#include "storm_hip_internal.h"
#include "storm_similarity_math.h"

namespace storm {

// the bit statistics as finish_tiles_kernel.inc takes them: one word per row, its count
struct SimilarityStat {
    static constexpr int W = 1;
    static __device__ __forceinline__ uint32_t bits(uint32_t c, const uint32_t (&a)[1], const uint32_t (&b)[1], int measure,
                                                    uint64_t n_bits) {
        return similarity_bits(c, a[0], b[0], measure, n_bits);
    }
    static int check(const char* who, int measure, uint64_t n_bits) {
        if (measure < STORM_HIP_SIM_JACCARD || measure > STORM_HIP_SIM_LD_R2) {
            set_error("%s: unknown measure %d (0 Jaccard, 1 cosine, 2 LD D, 3 LD r^2)", who, measure);
            return STORM_HIP_EINVAL;
        }
        if (n_bits == 0 || n_bits > (1ull << 32)) {
            set_error("%s: n_bits %llu is not in [1, 2^32]", who, (unsigned long long)n_bits);
            return STORM_HIP_EINVAL;
        }
        return STORM_HIP_OK;
    }
};

#include "finish_tiles_kernel.inc"

int launch_similarity_finish(storm_hip_ctx_t* ctx, void* d_io, uint64_t ld, uint64_t n_rows, uint64_t n_cols,
                             const uint32_t* d_counts_rows, const uint32_t* d_counts_cols, int triangle, int measure,
                             uint64_t n_bits) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    return launch_finish_tiles<SimilarityStat>(ctx, "similarity_finish", d_io, ld, n_rows, n_cols, {{d_counts_rows}}, {{d_counts_cols}},
                                               triangle != 0, measure, n_bits);
}

int launch_similarity_finish_lag(storm_hip_ctx_t* ctx, void* d_io, uint64_t ld, uint64_t n_rows, uint64_t row0,
                                 uint64_t n_band_rows, uint64_t max_lag, const uint32_t* d_counts, int measure, uint64_t n_bits) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    return launch_finish_lag_tiles<SimilarityStat>(ctx, "similarity_finish_lag", d_io, ld, n_rows, row0, n_band_rows, max_lag,
                                                   {{d_counts}}, measure, n_bits);
}

// the row counts of `m` into the context's scratch at word `at` (ensured by the caller)
static int counts_of(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, uint64_t at) {
    return launch_row_counts(ctx, m, ctx->d_counts.d + at);
}

// A's rows against B's (a == b: one matrix): the finish over counts that are already complete in stream order
static int finish_dense(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, void* d_io, uint64_t ld,
                        int triangle, int measure, uint64_t n_bits) {
    const uint64_t na = a->n_rows, nb = b->n_rows;
    if (int rc = ctx->d_counts.ensure((na + (b != a ? nb : 0)) * sizeof(uint32_t), "similarity: the row-count scratch")) return rc;
    if (int rc = counts_of(ctx, a, 0)) return rc;
    if (b != a)
        if (int rc = counts_of(ctx, b, na)) return rc;
    return launch_similarity_finish(ctx, d_io, ld, na, nb, ctx->d_counts.d, ctx->d_counts.d + (b != a ? na : 0), triangle, measure,
                                    n_bits);
}

// The AND counts of A's rows against B's, queued and not waited for, with the report storm_hip_cross_dense_matrix_device
// writes (that one waits for the stream, which the forms below do once, after the finish).
static int cross_counts(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, uint32_t* d_out,
                        uint64_t ld) {
    if (a->n_words != b->n_words) {
        set_error("cross_dense_similarity: row widths differ");
        return STORM_HIP_EINVAL;
    }
    if (int rc = launch_square_matrix(ctx, a, b, STORM_HIP_OP_AND, d_out, ld)) return rc;
    ctx->pass_report[0] = STORM_HIP_RAN_TILES_OUT;
    ctx->pass_report[1] = a->n_rows * b->n_rows * a->n_words;
    ctx->pass_report[2] = ctx->pass_report[3] = 0;
    return STORM_HIP_OK;
}

// the measure and n_bits before anything is launched (what launch_similarity_finish would refuse after the counts)
static int check_measure(int measure, uint64_t n_bits) {
    if (measure < STORM_HIP_SIM_JACCARD || measure > STORM_HIP_SIM_LD_R2 || n_bits == 0 || n_bits > (1ull << 32)) {
        set_error("similarity: unknown measure %d, or n_bits %llu is not in [1, 2^32]", measure, (unsigned long long)n_bits);
        return STORM_HIP_EINVAL;
    }
    return STORM_HIP_OK;
}

// ---- the per-pair matrix calls: one body for the device form and the host form of each (pair_matrix_out, storm_hip_internal.h) ----
// The triangle, cleared in the band buffer (entries i >= j). The device form returns below two rows without touching its
// matrix; the host form returns without rows, and for a single row writes its one zero (and the report of no pairs).
static int pairw_similarity(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, int measure, uint64_t n_bits, float* out, uint64_t ld,
                            bool host) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    if (!m || !out || ld < m->n_rows) {
        set_error("pairw_similarity: NULL argument or leading dimension < rows");
        return STORM_HIP_EINVAL;
    }
    if (int rc = check_measure(measure, n_bits)) return rc;
    const uint64_t n = m->n_rows;
    if (host ? n == 0 : n < 2) return STORM_HIP_OK;
    return pair_matrix_out(ctx, "pairw_similarity: the output", n, n, out, ld, host, true, true, [&](uint32_t* d, uint64_t d_ld) {
        if (int rc = launch_pairw_matrix(ctx, m, STORM_HIP_OP_AND, d, d_ld)) return rc;
        return n >= 2 ? finish_dense(ctx, m, m, d, d_ld, 1, measure, n_bits) : STORM_HIP_OK;
    });
}

// (a rectangle: every entry is written, nothing to clear)
static int cross_dense_similarity(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, int measure,
                                  uint64_t n_bits, float* out, uint64_t ld, bool host) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    if (!a || !b || !out || ld < b->n_rows) {
        set_error("cross_dense_similarity: NULL argument or ld < rows of B");
        return STORM_HIP_EINVAL;
    }
    if (int rc = check_measure(measure, n_bits)) return rc;
    if (a->n_rows == 0 || b->n_rows == 0) return STORM_HIP_OK;
    return pair_matrix_out(ctx, "cross_dense_similarity: the output", a->n_rows, b->n_rows, out, ld, host, false, true,
                           [&](uint32_t* d, uint64_t d_ld) {
                               if (int rc = cross_counts(ctx, a, b, d, d_ld)) return rc;
                               return finish_dense(ctx, a, b, d, d_ld, 0, measure, n_bits);
                           });
}

// ---- the lag layout (storm_hip.h): row i against the next L = min(max_lag, rows - 1) rows, an n x L matrix, cleared in the
// band buffer (the lower-right corner); both forms return below two rows ----
// what the lag calls refuse alike; *lag = L (0 for an empty matrix) (shared: storm_hip_internal.h)
int check_lag(const char* who, const storm_hip_matrix_s* m, const void* out, uint64_t max_lag, uint64_t ld, uint64_t* lag) {
    if (!m || !out || max_lag == 0) {
        set_error("%s: NULL argument or max_lag 0", who);
        return STORM_HIP_EINVAL;
    }
    *lag = m->n_rows ? std::min(max_lag, m->n_rows - 1) : 0;
    if (ld < *lag) {
        set_error("%s: leading dimension %llu < min(max_lag, rows - 1) = %llu", who, (unsigned long long)ld, (unsigned long long)*lag);
        return STORM_HIP_EINVAL;
    }
    return STORM_HIP_OK;
}

// the counts alone: the device form takes a band of rows; the host form every row, and names the op it refuses
static int pairw_lag_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, int op, uint64_t max_lag, uint64_t row0,
                            uint64_t n_band_rows, uint32_t* out, uint64_t ld, bool host) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    uint64_t lag = 0;
    if (int rc = check_lag("pairw_lag_matrix", m, out, max_lag, ld, &lag)) return rc;
    if (n_band_rows == ~0ull && row0 <= m->n_rows) n_band_rows = m->n_rows - row0;
    if (op < STORM_HIP_OP_AND || op > STORM_HIP_OP_XOR || row0 > m->n_rows || n_band_rows > m->n_rows - row0) {
        if (host) set_error("pairw_lag_matrix: unknown op %d", op);
        else set_error("pairw_lag_matrix: unknown op or a band outside the rows");
        return STORM_HIP_EINVAL;
    }
    if (m->n_rows < 2 || n_band_rows == 0) return STORM_HIP_OK;
    return pair_matrix_out(ctx, "pairw_lag_matrix: the output", n_band_rows, lag, out, ld, host, true, true,
                           [&](uint32_t* d, uint64_t d_ld) {
                               return launch_pairw_lag_matrix(ctx, m, op, max_lag, row0, n_band_rows, d, d_ld);
                           });
}

// counts in the lag layout at d_io (pitch ld), queued; then the rows' counts and the finish, queued too
static int lag_similarity_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, int measure, uint64_t n_bits, uint64_t max_lag,
                                 uint32_t* d_io, uint64_t ld) {
    const uint64_t n = m->n_rows;
    if (int rc = launch_pairw_lag_matrix(ctx, m, STORM_HIP_OP_AND, max_lag, 0, n, d_io, ld)) return rc;
    if (int rc = ctx->d_counts.ensure(n * sizeof(uint32_t), "similarity: the row-count scratch")) return rc;
    if (int rc = counts_of(ctx, m, 0)) return rc;
    return launch_similarity_finish_lag(ctx, d_io, ld, n, 0, n, max_lag, ctx->d_counts.d, measure, n_bits);
}

static int pairw_lag_similarity(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, int measure, uint64_t n_bits, uint64_t max_lag,
                                float* out, uint64_t ld, bool host) {
    if (check_ctx(ctx)) return STORM_HIP_EINVAL;
    uint64_t lag = 0;
    if (int rc = check_lag("pairw_lag_similarity", m, out, max_lag, ld, &lag)) return rc;
    if (int rc = check_measure(measure, n_bits)) return rc;
    if (m->n_rows < 2) return STORM_HIP_OK;
    return pair_matrix_out(ctx, "pairw_lag_similarity: the output", m->n_rows, lag, out, ld, host, true, true,
                           [&](uint32_t* d, uint64_t d_ld) { return lag_similarity_queued(ctx, m, measure, n_bits, max_lag, d, d_ld); });
}

}  // namespace storm

using namespace storm;

extern "C" {

int storm_hip_similarity_finish_device(storm_hip_ctx_t* ctx, void* d_io, uint64_t ld, uint64_t n_rows, uint64_t n_cols,
                                       const uint32_t* d_counts_rows, const uint32_t* d_counts_cols, int triangle, int measure,
                                       uint64_t n_bits) {
    return guarded("storm_hip_similarity_finish_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        if (int rc = launch_similarity_finish(ctx, d_io, ld, n_rows, n_cols, d_counts_rows, d_counts_cols, triangle, measure,
                                              n_bits))
            return rc;
        // alone on a caller's matrix the pass is the whole call: a report of its own, not an earlier call's kernels
        // beside it (an empty shape launched nothing and leaves the report as it was)
        if (n_rows && n_cols) {
            memset(ctx->pass_report, 0, sizeof(ctx->pass_report));
            ctx->pass_report[0] = STORM_HIP_RAN_SIMILARITY;
        }
        return STORM_HIP_OK;
    });
}

int storm_hip_pairw_similarity_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_bits,
                                      float* d_out, uint64_t ld) {
    return guarded("storm_hip_pairw_similarity_device", [&] { return pairw_similarity(ctx, m, measure, n_bits, d_out, ld, false); });
}

int storm_hip_pairw_similarity(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_bits, float* h_out,
                               uint64_t ld) {
    return guarded("storm_hip_pairw_similarity", [&] { return pairw_similarity(ctx, m, measure, n_bits, h_out, ld, true); });
}

int storm_hip_pairw_lag_matrix_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int op, uint64_t max_lag, uint64_t row0,
                                      uint64_t n_band_rows, uint32_t* d_out, uint64_t ld) {
    return guarded("storm_hip_pairw_lag_matrix_device",
                   [&] { return pairw_lag_matrix(ctx, m, op, max_lag, row0, n_band_rows, d_out, ld, false); });
}

int storm_hip_pairw_lag_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int op, uint64_t max_lag, uint32_t* h_out,
                               uint64_t ld) {
    return guarded("storm_hip_pairw_lag_matrix", [&] { return pairw_lag_matrix(ctx, m, op, max_lag, 0, ~0ull, h_out, ld, true); });
}

int storm_hip_similarity_finish_lag_device(storm_hip_ctx_t* ctx, void* d_io, uint64_t ld, uint64_t n_rows, uint64_t row0,
                                           uint64_t n_band_rows, uint64_t max_lag, const uint32_t* d_counts, int measure,
                                           uint64_t n_bits) {
    return guarded("storm_hip_similarity_finish_lag_device", [&]() -> int {
        if (check_ctx(ctx)) return STORM_HIP_EINVAL;
        if (int rc = launch_similarity_finish_lag(ctx, d_io, ld, n_rows, row0, n_band_rows, max_lag, d_counts, measure, n_bits))
            return rc;
        // (alone on a caller's matrix: a report of its own, as storm_hip_similarity_finish_device; nothing launched: as it was)
        if (n_rows >= 2 && n_band_rows != 0 && row0 < n_rows) {
            memset(ctx->pass_report, 0, sizeof(ctx->pass_report));
            ctx->pass_report[0] = STORM_HIP_RAN_SIMILARITY;
        }
        return STORM_HIP_OK;
    });
}

int storm_hip_pairw_lag_similarity_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_bits,
                                          uint64_t max_lag, float* d_out, uint64_t ld) {
    return guarded("storm_hip_pairw_lag_similarity_device",
                   [&] { return pairw_lag_similarity(ctx, m, measure, n_bits, max_lag, d_out, ld, false); });
}

int storm_hip_pairw_lag_similarity(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_bits,
                                   uint64_t max_lag, float* h_out, uint64_t ld) {
    return guarded("storm_hip_pairw_lag_similarity",
                   [&] { return pairw_lag_similarity(ctx, m, measure, n_bits, max_lag, h_out, ld, true); });
}

int storm_hip_cross_dense_similarity_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,
                                            int measure, uint64_t n_bits, float* d_out, uint64_t ld) {
    return guarded("storm_hip_cross_dense_similarity_device",
                   [&] { return cross_dense_similarity(ctx, a, b, measure, n_bits, d_out, ld, false); });
}

int storm_hip_cross_dense_similarity(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int measure,
                                     uint64_t n_bits, float* h_out, uint64_t ld) {
    return guarded("storm_hip_cross_dense_similarity",
                   [&] { return cross_dense_similarity(ctx, a, b, measure, n_bits, h_out, ld, true); });
}

}  // extern "C"
