/*
 * storm_hip.h — C-ABI of the MI355X (gfx950) device shim behind the storm.h API.
 *
 * This is the drop-in boundary for the pairwise AND+popcount hot path: plain pointers and
 * sizes, no C++ or torch types. Host code (C) calls these; they launch hand-written HIP
 * kernels (stormbitmaps_amd/csrc/storm_hip.hip). Each entry point names the reference
 * interface it replaces (file:line in mklarqvist/StormBitmaps).
 *
 * Conventions
 *   - every function returns 0 on success or a negative STORM_HIP_E* code; the message of the
 *     last failure on the calling thread is available from storm_hip_last_error().
 *   - there is NO CPU fallback: without a usable gfx950 device every compute entry point
 *     fails with STORM_HIP_ENODEV / STORM_HIP_EHIP.
 *   - `stream` arguments are hipStream_t passed as void* (NULL = the default stream).
 *   - a "dense matrix" is the device mirror of STORM_contiguous_t::data (storm.h:188-200):
 *     row-major uint64 rows, bit v of a row in word v/64 at bit v%64 (storm.c:1114). On the
 *     device the rows are padded with zeros to a multiple of 64 words and the row count to a
 *     multiple of 128 so that no kernel needs a ragged-edge path.
 */
#ifndef STORM_HIP_H_
#define STORM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: what these headers declare is its whole export list */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define STORM_HIP_OK 0
#define STORM_HIP_EINVAL (-1) /* bad argument                                  */
#define STORM_HIP_ENODEV (-2) /* no HIP device / not gfx950                    */
#define STORM_HIP_EHIP (-3)   /* a HIP runtime call failed                     */
#define STORM_HIP_ENOMEM (-4) /* host or device allocation failed              */

typedef struct storm_hip_ctx_s storm_hip_ctx_t;       /* one device + stream + workspace */
typedef struct storm_hip_matrix_s storm_hip_matrix_t; /* dense bitmap matrix in HBM      */
typedef struct storm_hip_sparse_s storm_hip_sparse_t; /* flattened STORM_t arena in HBM  */
typedef struct storm_hip_rowlists_s storm_hip_rowlists_t; /* rows of a list-only STORM_t as window-ordered positions (K5) */

/* ---- library / device ---- */
const char* storm_hip_last_error(void);
int storm_hip_device_count(void);
/* arch string of `device` ("gfx950:sramecc+:xnack-") into buf */
int storm_hip_device_arch(int device, char* buf, size_t buflen);
/* PCI address of `device` ("0000:75:00.0") into buf: which physical GPU a rank drives */
int storm_hip_device_pci_bus_id(int device, char* buf, size_t buflen);

/* ---- context: device, stream, reusable workspace ----
 * The stream contract (tests/test_gpu_streams.py; for the lag-dosage, LD-score and pruning calls tests/test_gpu_streams_ld.py):
 *   - Everything a context enqueues — kernels, zero fills, copies, the zeroing of its own workspace at creation — goes on its
 *     stream (`stream` of storm_hip_ctx_create, later storm_hip_ctx_set_stream's; NULL = the default stream). The one
 *     internal second stream (the panel copies of storm_hip_pairw_dense_upload) is ordered against it by events, both ways.
 *   - A call documented "synchronous" or "complete on return" has waited for the context's stream: its outputs, in host or
 *     in device memory, may be read by the host and by work on ANY other stream as soon as it returns.
 *   - The asynchronous calls only enqueue; a consumer enqueued on the same stream afterwards needs no host wait. They are:
 *       storm_hip_matrix_create (its zero fill), storm_hip_matrix_clear, storm_hip_matrix_fill_synthetic,
 *       storm_hip_matrix_import, storm_hip_matrix_resize when it shrinks (a growing resize waits),
 *       every `_launch` (storm_hip_pairw_dense_launch), every `_begin` (storm_hip_pairw_dense_begin, _pairw_sparse_begin,
 *       _pairw_matrix_band_begin), the primitives that say so (storm_hip_similarity_finish_device, _finish_lag_device,
 *       storm_hip_topk_rows_device, storm_hip_dosage_finish_lag_device, storm_hip_lag_band_sums_device,
 *       storm_hip_lag_band_annot_sums_device, storm_hip_lag_band_prune_device, storm_hip_lag_band_sparse_device), and the
 *       `_device` forms of the calls composed of them: storm_hip_lag_dosage_ldscore[_complete]_device,
 *       storm_hip_lag_dosage_ldscore_annot[_complete]_device, storm_hip_lag_dosage_prune[_complete]_device and
 *       storm_hip_lag_dosage_corr_sparse[_complete]_device — unlike storm_hip_pairw_lag_dosage_*_device, whose band they
 *       reduce and which are complete on return.
 *     A `_begin` is finished by its `_end` on the same context, whatever stream the context has by then.
 *   - HOST arrays handed to an asynchronous call (h_lo, h_hi, h_order of the LD-score and pruning calls, in every form) are
 *     read by copies queued on the context's stream: they must stay allocated and unchanged until that work is complete
 *     (storm_hip_ctx_synchronize, or a wait of the caller's for the stream); the outputs are final then, whatever happens to
 *     the arrays afterwards. The host forms of these calls wait themselves.
 *   - storm_hip_ctx_set_stream: work enqueued through the context after the call is ordered after ALL work enqueued through it
 *     before the call (an event recorded on the stream that is left, which the new stream waits for; if no event can be made
 *     the call waits for the old stream). The context's workspace (partial-sum slots, result word, mailbox, cached work lists)
 *     is therefore never used by two passes at once, and matrices, sparse arenas, row lists and stages made under the context
 *     stay usable. The call itself does not wait; a stream equal to the current one is a no-op. The old stream must still
 *     exist when the call is made.
 *   - The caller orders its OWN producers and consumers against the context's stream: a tensor handed to
 *     storm_hip_matrix_import or read from storm_hip_matrix_device_ptr, the word a `_launch` writes, must be produced / consumed
 *     on that stream or behind an event of the caller's.
 *   - One context is driven by one host thread at a time; two contexts on one device are independent (each has its own
 *     workspace) and may be interleaved call by call from one thread. */
int storm_hip_ctx_create(int device, void* stream, storm_hip_ctx_t** out);
int storm_hip_ctx_set_stream(storm_hip_ctx_t* ctx, void* stream);
int storm_hip_ctx_synchronize(storm_hip_ctx_t* ctx);
void storm_hip_ctx_destroy(storm_hip_ctx_t* ctx);

/* ---- dense matrix lifecycle (device mirror of STORM_contiguous_t, storm.c:1001-1147) ---- */
int storm_hip_matrix_create(storm_hip_ctx_t* ctx, uint64_t n_rows, uint32_t n_words,
                            storm_hip_matrix_t** out); /* zero-filled */
/* change the logical row count (device mirror of a container that grows row by row, storm.c:1078):
 * growing reallocates with amortised doubling and keeps the rows; new rows are zero until uploaded */
int storm_hip_matrix_resize(storm_hip_ctx_t* ctx, storm_hip_matrix_t* m, uint64_t n_rows);
/* copy n_rows host rows (row stride = src_stride_words) into rows [row0, row0+n_rows) */
int storm_hip_matrix_upload(storm_hip_ctx_t* ctx, storm_hip_matrix_t* m, uint64_t row0,
                            uint64_t n_rows, const uint64_t* host_rows,
                            uint64_t src_stride_words);
/* same from a device buffer (e.g. a torch tensor's data_ptr), device-to-device */
int storm_hip_matrix_import(storm_hip_ctx_t* ctx, storm_hip_matrix_t* m, uint64_t row0,
                            uint64_t n_rows, const void* device_rows,
                            uint64_t src_stride_words);
/* copy rows back to the host (tests) */
int storm_hip_matrix_download(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t row0,
                              uint64_t n_rows, uint64_t* host_rows, uint64_t dst_stride_words);
/* device-side construction from sorted position lists in CSR form (host pointers):
 * replaces the bit-setting loop of STORM_contig_add, storm.c:1103-1115 */
int storm_hip_matrix_set_rows_from_positions(storm_hip_ctx_t* ctx, storm_hip_matrix_t* m,
                                             uint64_t row0, uint64_t n_rows,
                                             const uint64_t* offsets, const uint32_t* positions);
/* synthetic fill on the device: identical bits to storm_synth_positions() (storm_synth.h) */
int storm_hip_matrix_fill_synthetic(storm_hip_ctx_t* ctx, storm_hip_matrix_t* m,
                                    uint64_t n_bits, uint32_t draws, uint64_t seed);
int storm_hip_matrix_clear(storm_hip_ctx_t* ctx, storm_hip_matrix_t* m);
void storm_hip_matrix_destroy(storm_hip_ctx_t* ctx, storm_hip_matrix_t* m);
uint64_t storm_hip_matrix_rows(const storm_hip_matrix_t* m);
uint32_t storm_hip_matrix_words(const storm_hip_matrix_t* m);
uint64_t storm_hip_matrix_stride_words(const storm_hip_matrix_t* m);
void* storm_hip_matrix_device_ptr(const storm_hip_matrix_t* m);

/* ---- the hot path --------------------------------------------------------------------
 * total = sum over row pairs i<j of popcount(row_i & row_j), restricted to this shard's share
 * of the pair space (shard_rank of shard_count; 0 of 1 = everything). The shards partition
 * the pairs, so the sum of the per-shard totals over all ranks is the full total.
 * Replaces: STORM_contig_pairw_intersect_cardinality[_blocked] (storm.c:1149-1241),
 *           STORM_wrapper_diag[_blocked] (storm.c:132-150, :222-279) and, through them, the
 *           libalgebra leaf STORM_compute_func (call sites storm.c:1167,1205,1217,1227,1236).
 * _launch: asynchronous on the ctx stream; d_total is a DEVICE pointer to one uint64.
 * plain   : synchronous; *h_total on the host. */
int storm_hip_pairw_dense_launch(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m,
                                 uint32_t shard_rank, uint32_t shard_count, uint64_t* d_total);
/* The same total for rows that are still in the CALLER's memory: `host_rows` (src_stride_words words per row, >= the
 * matrix's) replace all rows of `m`, travelling in panels of whole 256-row tiles on a second stream while the panel before is
 * being multiplied (the pairs whose later row lies in a panel are multiplied as soon as it has landed); *h_total on the
 * host, synchronous. What STORM_wrapper_diag[_blocked] (storm.c:132-150, :222-279) run on one device: those entry points
 * get the caller's buffer anew on every call. Matrices below 2048 rows: the copy, then the pass. */
int storm_hip_pairw_dense_upload(storm_hip_ctx_t* ctx, storm_hip_matrix_t* m, const uint64_t* host_rows,
                                 uint64_t src_stride_words, uint64_t* h_total);
int storm_hip_pairw_dense(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m,
                          uint32_t shard_rank, uint32_t shard_count, uint64_t* h_total);
/* split form, so that one host thread can keep several GPUs busy: _begin launches into the
 * ctx's own result word, _end waits for it and copies it to the host */
int storm_hip_pairw_dense_begin(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m,
                                uint32_t shard_rank, uint32_t shard_count);
int storm_hip_pairw_dense_end(storm_hip_ctx_t* ctx, uint64_t* h_total);
/* rectangle: sum over i in A, j in B of popcount(A_i & B_j) — STORM_wrapper_square,
 * storm.c:153-171 (intended semantics, storm.h:72-77) */
int storm_hip_square_dense(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a,
                           const storm_hip_matrix_t* b, uint64_t* h_total);
/* per-pair counts of one tile (tests / materialised output):
 * out[(i-i0)*(j1-j0)+(j-j0)] = popcount(row_i & row_j); out is a HOST buffer */
int storm_hip_tile_counts(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t i0,
                          uint64_t i1, uint64_t j0, uint64_t j1, uint32_t* h_out);
/* Sibling pair counts of the upstream leaf library (union / symmetric-difference cardinality,
 * reference README.md:24-26). They are not separate kernels: with the per-row
 * set-bit counts n_i,  |a|b| = n_a + n_b - |a&b|  and  |a^b| = n_a + n_b - 2|a&b|, so both ride
 * on the intersect path. */
#define STORM_HIP_OP_AND 0
#define STORM_HIP_OP_OR 1
#define STORM_HIP_OP_XOR 2
/* h_counts[i] = popcount(row_i), n_rows entries (host pointer) */
int storm_hip_row_counts(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint32_t* h_counts);
/* *h_total = sum_{i<j} popcount(row_i OP row_j) */
int storm_hip_pairw_dense_op(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int op,
                             uint64_t* h_total);

/* Materialised strict upper triangle of XX^T on the matrix cores (the product the reference
 * deliberately does not write out, README.md:41):
 *   out[i * ld + j] = popcount(row_i OP row_j) for i < j; other entries are left untouched.
 * _device: `d_out` is a DEVICE pointer to n_rows x ld uint32 (ld >= n_rows); synchronous.
 * plain  : `h_out` is a HOST n_rows x n_rows uint32 buffer; entries i >= j come back as 0.
 * Rows of 2^24 bits and more (beyond exact f32 accumulation in one go) are cut along k and the
 * parts added; the limit is 2^25 bits per row (32-bit DMA offsets of the tile kernel).
 * Empty shapes: a matrix of fewer than two rows has no pairs, a band of 0 rows and a rectangle with an empty side have no
 * entries — these calls (and the band and rectangle forms below) return STORM_HIP_OK and write nothing; the host form of a
 * one-row matrix returns its single 0. */
int storm_hip_pairw_matrix_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int op,
                                  uint32_t* d_out, uint64_t ld);
int storm_hip_pairw_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int op,
                           uint32_t* h_out);
/* A band of that triangle, for matrices whose n_rows^2 output does not fit at once: rows
 * [row0, row0 + n_band_rows) only, written from output row 0:
 *   d_out[(i - row0) * ld + j] = popcount(row_i OP row_j), row0 <= i < row0 + n_band_rows, i < j.
 * `d_out` is a DEVICE pointer to n_band_rows x ld uint32, ld >= n_rows. Bands of a few thousand
 * rows keep the matrix cores as busy as the whole triangle does. */
int storm_hip_pairw_matrix_band_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int op,
                                       uint64_t row0, uint64_t n_band_rows, uint32_t* d_out,
                                       uint64_t ld);
/* The same band into HOST memory: h_out[(i - row0) * ld + j], n_band_rows x ld uint32 with
 * ld >= n_rows; entries i >= j come back as 0. _begin only enqueues (one band per GPU can be in
 * flight from one host thread), _end waits for the context's stream. */
int storm_hip_pairw_matrix_band_begin(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int op,
                                      uint64_t row0, uint64_t n_band_rows, uint32_t* h_out,
                                      uint64_t ld);
int storm_hip_pairw_matrix_band_end(storm_hip_ctx_t* ctx);
int storm_hip_pairw_matrix_band(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int op,
                                uint64_t row0, uint64_t n_band_rows, uint32_t* h_out, uint64_t ld);
/* Materialised rectangle A x B (the two-matrix product XY^T):
 *   out[i * ld + j] = popcount(a_i OP b_j) for every row i of `a` and j of `b` (same row width).
 * _device: `d_out` is a DEVICE pointer, a->n_rows x ld uint32 with ld >= b->n_rows; synchronous.
 * plain  : `h_out` is a HOST a->n_rows x b->n_rows uint32 buffer. */
int storm_hip_square_matrix_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a,
                                   const storm_hip_matrix_t* b, int op, uint32_t* d_out, uint64_t ld);
int storm_hip_square_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a,
                            const storm_hip_matrix_t* b, int op, uint32_t* h_out);
/* The same two on the dense replicas of two STORM_t (storm.h: STORM_intersect_cardinality_square, STORM_square_matrix),
 * and a last-pass report naming the kernels that ran (the two above leave the report as it was). _matrix_device is
 * complete on return; _matrix: `h_out` is a HOST buffer, h_out[i * ld + j], ld >= b's rows. */
int storm_hip_cross_dense_total(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,
                                uint64_t* h_total);
int storm_hip_cross_dense_matrix_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,
                                        int op, uint32_t* d_out, uint64_t ld);
int storm_hip_cross_dense_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int op,
                                 uint32_t* h_out, uint64_t ld);

/* ---- per-pair similarity: the count matrix finished on the device ------------------------------------------
 * What the per-pair counts are for (reference README.md:165-167: linkage disequilibrium, "any intersect-count
 * problem"): one formula per entry over c = |A_i & B_j|, a = |A_i|, b = |B_j| and the universe size M = n_bits,
 *   STORM_HIP_SIM_JACCARD  c / (a + b - c)                         NaN when a + b - c = 0
 *   STORM_HIP_SIM_COSINE   c / sqrt(a b)   (Ochiai)                NaN when a b = 0
 *   STORM_HIP_SIM_LD_D     (M c - a b) / M^2                       always defined
 *   STORM_HIP_SIM_LD_R2    (M c - a b)^2 / (a (M - a) b (M - b))   NaN unless 0 < a < M and 0 < b < M
 * M c - a b exactly in 64-bit integers, the rest in double, rounded once to float (at most one float from the exactly
 * rounded rational); NaN is always the one quiet pattern 0x7FC00000. Jaccard and cosine do not read n_bits (it must
 * still be valid).
 * _finish_device, the primitive: `d_io` is a DEVICE matrix of n_rows x ld 32-bit words holding the counts as uint32;
 *   every converted entry is overwritten in place with its float. d_counts_rows[n_rows] / d_counts_cols[n_cols] (device)
 *   are the set-bit counts of the rows' and the columns' side. triangle != 0: only entries i < j (n_rows == n_cols);
 *   entries i >= j and the pitch columns [n_cols, ld) are neither read nor written. Asynchronous on the context's
 *   stream (finish_tiles_kernel<SimilarityStat>). STORM_HIP_EINVAL: NULL argument, unknown measure, n_bits 0 or above 2^32,
 *   ld < n_cols, a triangle that is not square. Empty shapes: STORM_HIP_OK, nothing touched. A caller with a count
 *   matrix of its own needs nothing else; the last-pass report is then STORM_HIP_RAN_SIMILARITY alone.
 * The other forms are the AND-count path of the operand kind (storm_hip_pairw_matrix_device, _cross_dense_matrix_device,
 * _rowlists_pairw_matrix_device, _rowlists_square_matrix_device: same kernels, same choice), the rows' counts, then
 * the finish; complete on return. _device: out[i * ld + j] in DEVICE memory (triangle forms: i < j, other entries as the
 * count kernel left them). Host forms: h_out[i * ld + j], whole rows, +0.0f at i >= j of a triangle. They add
 * STORM_HIP_RAN_SIMILARITY to the last-pass mask of the count kernel that ran. */
#define STORM_HIP_SIM_JACCARD 0
#define STORM_HIP_SIM_COSINE 1
#define STORM_HIP_SIM_LD_D 2
#define STORM_HIP_SIM_LD_R2 3
int storm_hip_similarity_finish_device(storm_hip_ctx_t* ctx, void* d_io, uint64_t ld, uint64_t n_rows, uint64_t n_cols,
                                       const uint32_t* d_counts_rows, const uint32_t* d_counts_cols, int triangle,
                                       int measure, uint64_t n_bits);
int storm_hip_pairw_similarity_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_bits,
                                      float* d_out, uint64_t ld);
int storm_hip_pairw_similarity(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_bits,
                               float* h_out, uint64_t ld);
int storm_hip_cross_dense_similarity_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,
                                            int measure, uint64_t n_bits, float* d_out, uint64_t ld);
int storm_hip_cross_dense_similarity(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,
                                     int measure, uint64_t n_bits, float* h_out, uint64_t ld);

/* ---- the lag layout: every row against the next max_lag rows ------------------------------------------------
 * Linkage disequilibrium (what the per-pair counts are for) is rarely wanted all-vs-all: pruning, clumping, r^2 decay and
 * banded LD matrices ask for row i against the next w rows in container order. The lag of a pair i < j is j - i; with
 * L = min(max_lag, n_rows - 1) the lag layout of an n_rows x ld matrix (ld >= L) holds the pair (i, j), 1 <= j - i <= L, at
 *   out[i * ld + (j - i - 1)]          (column d of row i is the pair (i, i + 1 + d)):
 * n x L entries instead of n x n, and only the 128 x 128 tiles within L rows of the diagonal are multiplied (always K2h,
 * tile128_kernel in its lag form, whatever k2_tile_shape says). Entries with i + 1 + d >= n_rows (the
 * lower-right corner) and the pitch columns [L, ld) are not part of the output.
 * _lag_matrix_device: counts under `op` into DEVICE memory; the row band [row0, row0 + n_band_rows) (n_band_rows = ~0: all
 *   rows from row0) is written from output row 0: d_out[(i - row0) * ld + (j - i - 1)]. Complete on return, like
 *   storm_hip_pairw_matrix_band_device. Entries outside the layout stay untouched.
 * _lag_matrix: all rows into HOST memory, h_out[i * ld + d]: columns [0, L) of every row are written, 0 in the corner;
 *   columns [L, ld) stay untouched (the n x L device matrix in between is the context's band buffer).
 * _similarity_finish_lag_device: the in-place uint32 -> float pass (see storm_hip_similarity_finish_device) over a count
 *   matrix in the lag layout: entry (i - row0, d) from d_counts[i] and d_counts[i + 1 + d] (d_counts: n_rows set-bit counts,
 *   device). Asynchronous on the context's stream (finish_lag_tiles_kernel<SimilarityStat>); alone the last-pass report is
 *   STORM_HIP_RAN_SIMILARITY.
 * _lag_similarity_device / _lag_similarity: the AND counts, the rows' counts, then that pass; complete on return; host form:
 *   +0.0f in the corner. Bit-identical to the same pairs of storm_hip_pairw_similarity.
 * STORM_HIP_EINVAL: NULL argument, unknown op or measure, bad n_bits, max_lag 0, ld < L, a band outside the rows, rows beyond
 * K2h's reach (row pitch x 128 >= 2^32 bytes, more than 65535 tiles of 128 rows). Fewer than two rows or an empty band:
 * STORM_HIP_OK, nothing written. Last-pass report: STORM_HIP_RAN_TILES_OUT (| STORM_HIP_RAN_SIMILARITY), [1] = the band's
 * pairs within the lag x n_words. */
int storm_hip_pairw_lag_matrix_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int op, uint64_t max_lag,
                                      uint64_t row0, uint64_t n_band_rows, uint32_t* d_out, uint64_t ld);
int storm_hip_pairw_lag_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int op, uint64_t max_lag, uint32_t* h_out,
                               uint64_t ld);
int storm_hip_similarity_finish_lag_device(storm_hip_ctx_t* ctx, void* d_io, uint64_t ld, uint64_t n_rows, uint64_t row0,
                                           uint64_t n_band_rows, uint64_t max_lag, const uint32_t* d_counts, int measure,
                                           uint64_t n_bits);
int storm_hip_pairw_lag_similarity_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_bits,
                                          uint64_t max_lag, float* d_out, uint64_t ld);
int storm_hip_pairw_lag_similarity(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_bits,
                                   uint64_t max_lag, float* h_out, uint64_t ld);

/* ---- per-row top-k neighbours: the selection on the device -------------------------------------------------
 * For each row its k most similar rows (k-NN graphs on Jaccard or cosine, the best LD tags of a variant, the nearest sets
 * of a query container in a reference container): n x k entries leave the device instead of n x n. `score` is one of the
 * similarity measures above (the value is bit-identical to what the similarity calls write) or STORM_HIP_TOPK_COUNT, the
 * AND count itself; that constant is valid in the top-k calls only. Order within a row: value descending, then column
 * index ascending (fully determined: no two entries of a row compare equal). An undefined entry (NaN, 0x7FC00000) is not
 * a candidate. A row with fewer than k candidates is padded: idx 0xFFFFFFFF with val NaN (0x7FC00000) for the measures,
 * idx 0xFFFFFFFF with val 0 for STORM_HIP_TOPK_COUNT. 1 <= k <= STORM_HIP_TOPK_MAX.
 * Outputs: idx is n_rows x ld_k uint32 (the column), val n_rows x ld_k 32-bit words (float, or uint32 for the count);
 *   columns [0, k) of every row are always written, columns [k, ld_k) are not touched.
 * _topk_rows_device, the primitive: `d_counts_matrix` is a COMPLETE count matrix in DEVICE memory, n_rows x ld uint32
 *   (read, never written; the pitch columns [n_cols, ld) are not read), d_counts_rows[n_rows] / d_counts_cols[n_cols] the
 *   set-bit counts of the rows' and the columns' side. Row r never takes column skip0 + r as a candidate (how a row
 *   excludes itself); skip0 = ~0: none. Asynchronous on the context's stream (topk_rows_kernel, one 128-bit load per lane
 *   where the base is 16-byte aligned and ld a multiple of 4); alone the last-pass report is STORM_HIP_RAN_TOPK.
 * _pairw_topk: row i of `m` against every other row j != i, on both sides of the diagonal. _cross_dense_topk: every row of
 *   `a` against every row of `b` (equal row widths). Both run in row panels: the AND-count rectangle of panel_rows rows
 *   against all columns into the context's band buffer (the kernels and the choice of storm_hip_cross_dense_matrix_device),
 *   then the selection over it. panel_rows = 0: the largest multiple of 256 whose panel is at most 256 MiB, at least 256;
 *   else a multiple of 256. _device: idx / val in DEVICE memory, complete on return; the others copy n x k of each back.
 *   The pairw form multiplies both sides of the diagonal: twice the work of the triangle (open).
 * STORM_HIP_EINVAL: NULL argument, unknown score, n_bits outside [1, 2^32] (read by LD D and r^2 only), k of 0 or above the
 *   maximum, ld_k < k, ld < n_cols, panel_rows not a multiple of 256, row widths that differ. No rows: STORM_HIP_OK,
 *   nothing written; pairw on one row, or cross with an empty `b`: every row is k paddings. Last-pass report:
 *   STORM_HIP_RAN_TILES_OUT | STORM_HIP_RAN_TOPK, [1] = rows x columns x n_words. */
#define STORM_HIP_TOPK_COUNT 4
#define STORM_HIP_TOPK_MAX 128
int storm_hip_topk_rows_device(storm_hip_ctx_t* ctx, const uint32_t* d_counts_matrix, uint64_t ld, uint64_t n_rows,
                               uint64_t n_cols, const uint32_t* d_counts_rows, const uint32_t* d_counts_cols, uint64_t skip0,
                               int score, uint64_t n_bits, uint64_t k, uint32_t* d_idx, void* d_val, uint64_t ld_k);
int storm_hip_pairw_topk_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int score, uint64_t n_bits, uint64_t k,
                                uint64_t panel_rows, uint32_t* d_idx, void* d_val, uint64_t ld_k);
int storm_hip_pairw_topk(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int score, uint64_t n_bits, uint64_t k,
                         uint64_t panel_rows, uint32_t* h_idx, void* h_val, uint64_t ld_k);
int storm_hip_cross_dense_topk_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,
                                      int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* d_idx,
                                      void* d_val, uint64_t ld_k);
int storm_hip_cross_dense_topk(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int score,
                               uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* h_idx, void* h_val, uint64_t ld_k);

/* ---- rows of 2-bit values: dot products and genotype correlation (PLINK --r / --r2) --------------------------
 * Unphased genotype data holds a dosage of 0, 1 or 2 per sample, and the LD asked of it is the (squared) Pearson
 * correlation of two dosage vectors. Here a "dosage matrix" is an ordinary storm_hip_matrix_t whose rows hold VALUES
 * 0 .. 3 in 2 bits each: value s of a row in bits 2 (s % 32) and 2 (s % 32) + 1 of word s / 32 (ceil(n_samples / 32)
 * words per row, tail bits zero, at most 2^24 samples). 3 is an ordinary value in the calls of this block; the block below
 * reads it as "missing".
 * With P = sum v_i v_j, s = sum v, q = sum v^2 and S = n_samples:
 *   num = S P - s_i s_j and d = S q - s^2 exactly in 64-bit integers, then in double, rounded once to float,
 *   STORM_HIP_DOSAGE_R2   num^2 / (d_i d_j)          STORM_HIP_DOSAGE_R   num / sqrt(d_i d_j)
 *   at most one float from the exactly rounded value; NaN (0x7FC00000) when d_i or d_j is 0: a constant row.
 * _dosage_row_sums: h_sum[i] = s_i, h_sum_sq[i] = q_i (host pointers, n_rows entries), computed on the device.
 * _pairw_dosage_matrix[_device]: out[i * ld + j] = P(i, j) for i < j (uint32, exact), ld >= n_rows. Always K2h in its
 *   dosage form (tile128_kernel on two classes per nibble at block scale 128: the FP4 codes 0 .. 3 are linear in the
 *   value), whatever k2_tile_shape says; read-only option "k2_tile_shape_used" then reads 7 (6: K2h on
 *   bits). _device: entries i >= j stay as they were, complete on return. Host form: whole rows, 0 at i >= j.
 * _pairw_dosage_corr[_device]: the dot products, the rows' sums, then finish_tiles_kernel<DosageStat, true> in place; n_samples must be
 *   the S the rows were packed with (ceil(S / 32) == the matrix's words). Host form: +0.0f at i >= j.
 * STORM_HIP_EINVAL: NULL argument, ld < rows, unknown measure, n_samples that does not match the row width, rows of more
 * than 2^24 values, rows beyond K2h's reach. Fewer than two rows: STORM_HIP_OK, nothing written (host forms of one row:
 * its single 0). Last-pass report: STORM_HIP_RAN_TILES_OUT (| STORM_HIP_RAN_SIMILARITY for the correlation). */
#define STORM_HIP_DOSAGE_R2 0
#define STORM_HIP_DOSAGE_R 1
int storm_hip_dosage_row_sums(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint32_t* h_sum, uint32_t* h_sum_sq);
int storm_hip_pairw_dosage_matrix_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint32_t* d_out, uint64_t ld);
int storm_hip_pairw_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint32_t* h_out, uint64_t ld);
int storm_hip_pairw_dosage_corr_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                       float* d_out, uint64_t ld);
int storm_hip_pairw_dosage_corr(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                float* h_out, uint64_t ld);

/* ---- the rectangle of two dosage matrices; rows with missing genotypes: pairwise-complete r / r^2 ----------------
 * _square_dosage_matrix[_device]: out[i * ld + j] = sum_s a_i[s] b_j[s] for EVERY row i of A and j of B (uint32, exact;
 *   3 is an ordinary value), ld >= b's rows. K2h in its dosage form over the rectangle's 128 x 128 tiles. Both matrices
 *   must have the same words per row (a mismatch: STORM_HIP_EINVAL). An empty matrix: STORM_HIP_OK, nothing written.
 *   _device: complete on return, nothing outside the n_a x n_b window is written.
 * In the three calls below — and only there — code 3 of a value means MISSING. With g = the value (0 where missing) and
 * m = 1 where a sample s < n_samples is present, per pair (i, j):
 *   N = sum m_i m_j, P = sum g_i g_j, Sx = sum g_i m_j, Sy = sum m_i g_j, Qx = sum g_i^2 m_j, Qy = sum m_i g_j^2,
 *   num = N P - Sx Sy, dx = N Qx - Sx^2, dy = N Qy - Sy^2 exactly in 64-bit integers, then in double, rounded once to float:
 *   STORM_HIP_DOSAGE_R2 num^2 / (dx dy), STORM_HIP_DOSAGE_R num / sqrt(dx dy): PLINK's r over the samples BOTH rows have.
 *   NaN (0x7FC00000) exactly when dx or dy is 0: N = 0, N = 1, or a row constant on the shared samples. On rows without a 3
 *   the floats are bit-identical to _pairw_dosage_corr's.
 * _dosage_row_missing: h_missing[i] = the samples of row i that are missing (host pointer, n_rows entries).
 * _pairw_dosage_nobs[_device]: out[i * ld + j] = N(i, j) for i < j (uint32).
 * _pairw_dosage_corr_complete[_device]: the rows are split on the device into three matrices of 2-bit rows (G: 3 -> 0;
 *   H: 1 where the value is 2, so that g^2 = g + 2 h; M: 1 where present), K2h multiplies the triangles of G and of M and
 *   the rectangle [G ; H] x M (3 n^2 row-pair products), and dosage_complete_finish_kernel finishes in place. Device
 *   scratch held by the context: about 3 n^2 uint32 of sums and three copies of the rows; an allocation that fails returns
 *   STORM_HIP_ENOMEM with the reason.
 * Output conventions, n_samples and refusals as _pairw_dosage_corr[_device]: entries i >= j stay as they were (_device) or
 * are 0 / +0.0f (host forms); fewer than two rows: STORM_HIP_OK, nothing written (host forms of one row: its single 0). */
int storm_hip_square_dosage_matrix_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,
                                          uint32_t* d_out, uint64_t ld);
int storm_hip_square_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,
                                   uint32_t* h_out, uint64_t ld);
int storm_hip_dosage_row_missing(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint32_t* h_missing);
int storm_hip_pairw_dosage_nobs_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint32_t* d_out,
                                       uint64_t ld);
int storm_hip_pairw_dosage_nobs(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint32_t* h_out,
                                uint64_t ld);
int storm_hip_pairw_dosage_corr_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure,
                                                uint64_t n_samples, float* d_out, uint64_t ld);
int storm_hip_pairw_dosage_corr_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                         float* h_out, uint64_t ld);

/* ---- r / r^2 and N of the rectangle of two dosage matrices ---------------------------------------------------------
 * The three correlation calls above for EVERY row i of A against every row j of B (a list of index variants against a
 * panel: PLINK's --r2 --ld-snp-list ... inter-chr), entry out[i * ld + j], ld >= b's rows; each row's sums are taken in
 * its own matrix. A may be B.
 * _square_dosage_corr[_device]: 3 is an ordinary value. The dot products (storm_hip_square_dosage_matrix_device), both
 *   matrices' row sums, then finish_tiles_kernel<DosageStat, false> in place: _pairw_dosage_corr's formula and bits for the pair.
 * _square_dosage_nobs[_device], _square_dosage_corr_complete[_device]: code 3 means MISSING, as in the block above. Both
 *   matrices are split into G, H and M (once when A is B); _nobs is M_a x M_b; _corr_complete is six n_a x n_b products on
 *   K2h in three launches — G_a x G_b into the output, [G_a ; H_a] x M_b and M_a x [G_b ; H_b ; M_b] into scratch — and
 *   dosage_square_complete_finish_kernel in place: _pairw_dosage_corr_complete's formula and bits for the pair, and on rows
 *   without a 3 _square_dosage_corr's. Device scratch held by the context: about 5 n_a n_b uint32 of sums and three copies
 *   of the rows of each matrix (nothing bounds it by panels of B: the caller cuts B); an allocation that fails returns
 *   STORM_HIP_ENOMEM with the buffer named.
 * n_samples, the measures and the refusals as _square_dosage_matrix and _pairw_dosage_corr: STORM_HIP_EINVAL for a NULL
 * argument, rows of different widths, ld < b's rows, an unknown measure, n_samples that does not match the row width,
 * rows of more than 2^24 values, rows beyond the reach of K2h, of the split (65408 rows) or of the finishing pass's launch
 * grid. An empty matrix: STORM_HIP_OK, nothing written. _device: complete on return, nothing outside the n_a x n_b window
 * is written; host forms write the window alone. Last-pass report: STORM_HIP_RAN_TILES_OUT (| STORM_HIP_RAN_SIMILARITY for
 * the correlations), [1] = n_a n_b n_words (_corr_complete: 6 times that). */
int storm_hip_square_dosage_corr_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int measure,
                                        uint64_t n_samples, float* d_out, uint64_t ld);
int storm_hip_square_dosage_corr(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int measure,
                                 uint64_t n_samples, float* h_out, uint64_t ld);
int storm_hip_square_dosage_nobs_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,
                                        uint64_t n_samples, uint32_t* d_out, uint64_t ld);
int storm_hip_square_dosage_nobs(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, uint64_t n_samples,
                                 uint32_t* h_out, uint64_t ld);
int storm_hip_square_dosage_corr_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,
                                                 int measure, uint64_t n_samples, float* d_out, uint64_t ld);
int storm_hip_square_dosage_corr_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int measure,
                                          uint64_t n_samples, float* h_out, uint64_t ld);

/* ---- per-row top-k neighbours of dosage rows: the best r^2 / r tags of a variant, selected on the device -----------
 * The top-k calls above for dosage matrices: for each row its k best rows by STORM_HIP_DOSAGE_R2, STORM_HIP_DOSAGE_R (the
 * SIGNED value: ranking by |r| is what STORM_HIP_DOSAGE_R2 gives) or STORM_HIP_DOSAGE_TOPK_DOT, the dot product itself
 * (val is uint32 then and a padding entry has val 0; valid in the top-k calls only, and not in the _complete forms).
 * Order, NaN entries, padding, k and the outputs idx / val (pitch ld_k) exactly as in the top-k block above. The value bits
 * are what _square_dosage_corr writes for the two rows (3 an ordinary value), in the _complete forms what
 * _square_dosage_corr_complete writes (3 = MISSING). No float matrix is formed: the selection kernel (topk_rows_kernel over
 * a dosage scorer) reads the panel of integer sums once and forms each entry's value itself.
 * _dosage_topk_rows_device, the primitive: `d_dots` is a COMPLETE panel of dot products in DEVICE memory, n_rows x ld uint32
 *   (read, never written; the pitch columns [n_cols, ld) are not read), d_sum_rows / d_sq_rows [n_rows] and d_sum_cols /
 *   d_sq_cols [n_cols] the sums s and q of the rows' and of the columns' side, n_samples in [1, 2^24]; skip0 as in
 *   _topk_rows_device. Asynchronous on the context's stream; alone the last-pass report is STORM_HIP_RAN_TOPK.
 * _pairw_dosage_topk[_complete]: row i of `m` against every other row, on both sides of the diagonal (twice the work of
 *   the triangle: DESIGN.md §8, open). _square_dosage_topk[_complete]: every row of `a` against every row of `b` (a may be
 *   b: a row lists itself then). Row panels: each matrix's row sums (plain) or split into G, H, M (complete: at most 65408
 *   rows per matrix) once per call, then per panel of panel_rows rows of `a` the sums' rectangles against all of `b` — one
 *   K2h launch, or G_p x G_b, G_p x M_b, H_p x M_b and M_p x [G_b ; H_b ; M_b] — into the context's scratch and the
 *   selection over them. panel_rows = 0: the largest multiple of 256 whose planes (1 word per entry, complete: about 6)
 *   hold at most 256 MiB, at least 256; else a multiple of 256. The scratch is O(panel_rows x n_b), not O(n_a x n_b).
 *   _device: idx / val in DEVICE memory, complete on return; the others copy n x k of each back.
 * STORM_HIP_EINVAL: NULL argument, rows of different widths, unknown score (or the dot product in a _complete form),
 *   n_samples that does not match the row width, rows of more than 2^24 values, k of 0 or above STORM_HIP_TOPK_MAX,
 *   ld_k < k, ld < n_cols, panel_rows not a multiple of 256. No rows: STORM_HIP_OK, nothing written; pairw on one row, or an
 *   empty `b`: every row is k paddings. Last-pass report: STORM_HIP_RAN_TILES_OUT | STORM_HIP_RAN_TOPK, [1] = n_a n_b
 *   n_words (_complete: 6 times that). */
#define STORM_HIP_DOSAGE_TOPK_DOT 2
int storm_hip_dosage_topk_rows_device(storm_hip_ctx_t* ctx, const uint32_t* d_dots, uint64_t ld, uint64_t n_rows, uint64_t n_cols,
                                      const uint32_t* d_sum_rows, const uint32_t* d_sq_rows, const uint32_t* d_sum_cols,
                                      const uint32_t* d_sq_cols, uint64_t n_samples, uint64_t skip0, int score, uint64_t k,
                                      uint32_t* d_idx, void* d_val, uint64_t ld_k);
int storm_hip_pairw_dosage_topk_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int score, uint64_t n_samples, uint64_t k,
                                       uint64_t panel_rows, uint32_t* d_idx, void* d_val, uint64_t ld_k);
int storm_hip_pairw_dosage_topk(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int score, uint64_t n_samples, uint64_t k,
                                uint64_t panel_rows, uint32_t* h_idx, void* h_val, uint64_t ld_k);
int storm_hip_pairw_dosage_topk_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int score, uint64_t n_samples,
                                                uint64_t k, uint64_t panel_rows, uint32_t* d_idx, void* d_val, uint64_t ld_k);
int storm_hip_pairw_dosage_topk_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int score, uint64_t n_samples, uint64_t k,
                                         uint64_t panel_rows, uint32_t* h_idx, void* h_val, uint64_t ld_k);
int storm_hip_square_dosage_topk_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int score,
                                        uint64_t n_samples, uint64_t k, uint64_t panel_rows, uint32_t* d_idx, void* d_val,
                                        uint64_t ld_k);
int storm_hip_square_dosage_topk(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int score,
                                 uint64_t n_samples, uint64_t k, uint64_t panel_rows, uint32_t* h_idx, void* h_val, uint64_t ld_k);
int storm_hip_square_dosage_topk_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,
                                                 int score, uint64_t n_samples, uint64_t k, uint64_t panel_rows, uint32_t* d_idx,
                                                 void* d_val, uint64_t ld_k);
int storm_hip_square_dosage_topk_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b, int score,
                                          uint64_t n_samples, uint64_t k, uint64_t panel_rows, uint32_t* h_idx, void* h_val,
                                          uint64_t ld_k);

/* ---- dosage matrices in the lag layout: PLINK --r / --r2 within a window (--ld-window) ---------------------------
 * The calls of the two blocks above for the pairs within max_lag rows of each other, in the lag layout of
 * storm_hip_pairw_lag_matrix_device: with L = min(max_lag, n_rows - 1), entry out[i * ld + (j - i - 1)] is the pair
 * (i, j), 1 <= j - i <= L, ld >= L: n x L entries, and memory and work are O(n L). Always K2h in its lag and dosage form
 * (tile128_kernel<true, 2>); read-only option "k2_tile_shape_used" reads 7.
 * _lag_dosage_matrix_device: P(i, j) = sum v_i v_j (uint32, exact; 3 is an ordinary value) into DEVICE memory; the row band
 *   [row0, row0 + n_band_rows) (n_band_rows = ~0: all rows from row0) is written from output row 0. Complete on return.
 *   The lower-right corner (i + 1 + d >= n_rows) and the pitch columns [L, ld) stay untouched.
 * _lag_dosage_matrix: all rows into HOST memory: columns [0, L) of every row are written, 0 in the corner; columns [L, ld)
 *   stay untouched.
 * _dosage_finish_lag_device: the in-place uint32 -> float pass alone over a matrix of dot products in the lag layout
 *   (finish_lag_tiles_kernel<DosageStat>): entry (i - row0, d) from d_sum / d_sum_sq (n_rows entries each, device) of rows i and
 *   i + 1 + d. Asynchronous on the context's stream; alone the last-pass report is STORM_HIP_RAN_SIMILARITY.
 * _lag_dosage_corr[_device]: the dot products, the rows' sums, then that pass. Bit-identical to the same pairs of
 *   storm_hip_pairw_dosage_corr. Host form: +0.0f in the corner.
 * _lag_dosage_nobs[_device], _lag_dosage_corr_complete[_device]: code 3 means MISSING, as in the block above. The rows are
 *   split on the device into ONE matrix of 3 n rows (row 3 i: G_i, 3 i + 1: H_i, 3 i + 2: M_i); _nobs is the lag form on
 *   its M rows; _corr_complete is one launch of K2h over all 3 n rows at lag 3 L + 2 — which holds every product of G, H
 *   and M of two rows within L of each other — into a scratch matrix of 3 n x (3 L + 2) uint32 and
 *   dosage_complete_finish_lag_kernel from there into the caller's matrix. Device scratch held by the context: that
 *   matrix and three copies of the rows, nothing that grows with n^2; an allocation that fails returns STORM_HIP_ENOMEM
 *   with the buffer named. Bit-identical to the same pairs of storm_hip_pairw_dosage_corr_complete; on rows without a 3,
 *   to _lag_dosage_corr's.
 * STORM_HIP_EINVAL: NULL argument, unknown measure, max_lag 0, ld < L, a band outside the rows, n_samples that does not match
 * the row width, rows of more than 2^24 values, rows beyond K2h's reach (for the two calls on missing genotypes: 3 n rows).
 * Fewer than two rows or an empty band: STORM_HIP_OK, nothing written. Last-pass report: STORM_HIP_RAN_TILES_OUT
 * (| STORM_HIP_RAN_SIMILARITY), [1] = the pairs within the lag x n_words (_corr_complete: of the 3 n rows within 3 L + 2). */
int storm_hip_pairw_lag_dosage_matrix_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t max_lag, uint64_t row0,
                                             uint64_t n_band_rows, uint32_t* d_out, uint64_t ld);
int storm_hip_pairw_lag_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t max_lag, uint32_t* h_out,
                                      uint64_t ld);
int storm_hip_dosage_finish_lag_device(storm_hip_ctx_t* ctx, void* d_io, uint64_t ld, uint64_t n_rows, uint64_t row0,
                                       uint64_t n_band_rows, uint64_t max_lag, const uint32_t* d_sum, const uint32_t* d_sum_sq,
                                       int measure, uint64_t n_samples);
int storm_hip_pairw_lag_dosage_corr_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                           uint64_t max_lag, float* d_out, uint64_t ld);
int storm_hip_pairw_lag_dosage_corr(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                    uint64_t max_lag, float* h_out, uint64_t ld);
int storm_hip_pairw_lag_dosage_nobs_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples,
                                           uint64_t max_lag, uint32_t* d_out, uint64_t ld);
int storm_hip_pairw_lag_dosage_nobs(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                    uint32_t* h_out, uint64_t ld);
int storm_hip_pairw_lag_dosage_corr_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure,
                                                    uint64_t n_samples, uint64_t max_lag, float* d_out, uint64_t ld);
int storm_hip_pairw_lag_dosage_corr_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                             uint64_t max_lag, float* h_out, uint64_t ld);

/* ---- LD scores: per-row sums over both sides of a band in the lag layout, reduced on the device --------------------
 * storm_hip_lag_band_sums_device: d_vals is any float matrix in the lag layout in DEVICE memory (n_rows rows of pitch ld,
 *   the pair (i, i + 1 + d) at d_vals[i * ld + d], L = min(max_lag, n_rows - 1), ld >= L). For every row i,
 *     d_score[i]   = the sum of the terms of the pairs (i, j), 1 <= |i - j| <= L, accumulated in double, rounded once to
 *                    float (+0.0f when no pair is summed),
 *     d_n_pairs[i] = how many pairs were summed (may be NULL),
 *   where a pair's term is its float widened to double (stat STORM_HIP_LDSCORE_R2) or rho - (1 - rho) / (N - 2) in double
 *   (STORM_HIP_LDSCORE_R2_ADJ), and a pair is NOT summed when its float is NaN or, under _ADJ, N < 3. N is n_const, or,
 *   with d_nobs not NULL, the uint32 at d_nobs[i * nobs_row_pitch + d * nobs_col_stride] of the pair's entry (i, d).
 *   Exactly elements [0, n_rows) of the outputs are written. The lower-right corner (i + 1 + d >= n_rows) and the pitch
 *   columns [L, ld) of d_vals — and the same places of d_nobs — are never read. lag_band_sums_kernel: one workgroup per
 *   64 rows, every entry read twice (once for either row of its pair), no atomics and no clearing launch: the order of the
 *   additions is fixed, two calls on the same band return the same bits. Queued on the context's stream; no host wait.
 *   The LD r^2 of storm_hip_pairw_lag_similarity_device goes through the same call with n_const = n_bits.
 * storm_hip_lag_dosage_ldscore[_device]: rows of 2-bit dosages: storm_hip_pairw_lag_dosage_corr's r^2 into the context's
 *   band buffer (n x L floats of device scratch, beside that call's own), then the reduction with n_const = n_samples.
 * storm_hip_lag_dosage_ldscore_complete[_device]: the same over storm_hip_pairw_lag_dosage_corr_complete's r^2 (value 3 =
 *   missing); under _ADJ N(i, j) is read from that call's scratch matrix of sums, where it already lies: the nobs form is
 *   not launched again.
 *   The _device forms write d_score / d_n_pairs in DEVICE memory and return with everything queued on the context's
 *   stream; the host forms copy 2 n words back and wait.
 *   NOTE: unlike storm_hip_pairw_lag_dosage_*_device above, which are complete on return, these _device forms (and
 *   storm_hip_lag_band_sums_device) do NOT wait: order later work on the context's stream, or call storm_hip_ctx_synchronize. Sums are over the neighbours only: LDSC's l_i is 1 + score[i].
 * STORM_HIP_EINVAL: NULL context, matrix, band or score, unknown stat, max_lag 0, ld < L, n_samples that does not match the
 * row width, rows of more than 2^24 values. Fewer than two rows: STORM_HIP_OK, nothing written. */
#define STORM_HIP_LDSCORE_R2 0
#define STORM_HIP_LDSCORE_R2_ADJ 1
int storm_hip_lag_band_sums_device(storm_hip_ctx_t* ctx, const float* d_vals, uint64_t ld, uint64_t n_rows, uint64_t max_lag,
                                   int stat, uint64_t n_const, const uint32_t* d_nobs, uint64_t nobs_row_pitch,
                                   uint64_t nobs_col_stride, float* d_score, uint32_t* d_n_pairs);
int storm_hip_lag_dosage_ldscore_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                        uint64_t max_lag, float* d_score, uint32_t* d_n_pairs);
int storm_hip_lag_dosage_ldscore(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples, uint64_t max_lag,
                                 float* h_score, uint32_t* h_n_pairs);
int storm_hip_lag_dosage_ldscore_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                                 uint64_t max_lag, float* d_score, uint32_t* d_n_pairs);
int storm_hip_lag_dosage_ldscore_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                          uint64_t max_lag, float* h_score, uint32_t* h_n_pairs);

/* ---- stratified LD scores: the band times an annotation matrix, with a window per row ------------------------------
 * storm_hip_lag_band_annot_sums_device: d_vals, ld, n_rows, max_lag, stat, n_const and the d_nobs view as in
 *   storm_hip_lag_band_sums_device. d_annot: n_rows x n_annot floats of pitch annot_ld, d_score: n_rows x n_annot floats
 *   of pitch score_ld, d_lo / d_hi: n_rows uint32 each or both NULL, all in DEVICE memory. For every row i and column c,
 *     d_score[i * score_ld + c] = the sum over the summed pairs (i, j), j != i, |i - j| <= L, d_lo[i] <= j <= d_hi[i], of
 *                                 term(i, j) * (double)d_annot[j * annot_ld + c], accumulated in double (the
 *                                 products are not rounded on their own), rounded once to float (+0.0f when no pair is
 *                                 summed),
 *     d_n_pairs[i]              = how many pairs were summed (one number per row; may be NULL).
 *   d_lo / d_hi NULL: the whole lag. The bounds must be symmetric — j within [d_lo[i], d_hi[i]] exactly when i is within
 *   [d_lo[j], d_hi[j]] — as storm.h's planner makes them: the kernel tests d_lo[i] behind row i and d_hi[i] ahead of it.
 *   Whatever they hold, nothing outside the band is read. The annotations must be finite (a NaN or an infinity spreads
 *   over its column's window). Columns [n_annot, annot_ld) of d_annot are never read and columns [n_annot, score_ld) of
 *   d_score never written; the corner and the pitch columns of d_vals and d_nobs are never read.
 *   lag_band_annot_sums_kernel: one workgroup per 64 rows x 64 columns, tiles of 64 source rows through the LDS, double
 *   accumulators of v_mfma_f64_16x16x4_f64 in registers (STORM_HIP_LDSCORE_ANNOT_INNER=fma in the environment runs the
 *   v_fma_f64 form instead, for comparison; read at every launch); no atomics and no clearing launch. The order of the additions of (i, c) depends on i and
 *   L alone: a column has the same bits whatever other columns are passed with it, and two calls return the same bits.
 *   Queued on the context's stream; no host wait.
 * storm_hip_lag_dosage_ldscore_annot[_complete][_device]: rows of 2-bit dosages: the band of r^2 as in
 *   storm_hip_lag_dosage_ldscore[_complete] (L = min(max_lag, n - 1)), then the kernel above. h_lo / h_hi are HOST arrays
 *   of n entries in every form (both or NULL); the windows must need no more than max_lag rows (storm.h checks). The host
 *   forms upload the annotations, download n x n_annot scores and the counts, and wait; the _device forms take d_annot,
 *   d_score and d_n_pairs in device memory and return with everything queued: h_lo / h_hi must stay unchanged until that
 *   work is complete (storm_hip_ctx_synchronize). Device scratch: n x L floats, 2 n words, and for the host forms
 *   2 n x n_annot + n words, in the context's band buffer.
 * STORM_HIP_EINVAL: what storm_hip_lag_band_sums_device / storm_hip_lag_dosage_ldscore refuse, in their order, then NULL
 * annotations, n_annot outside [1, 1024], annot_ld or score_ld < n_annot, one of lo / hi without the other. Fewer than two
 * rows: STORM_HIP_OK, nothing written. */
int storm_hip_lag_band_annot_sums_device(storm_hip_ctx_t* ctx, const float* d_vals, uint64_t ld, uint64_t n_rows, uint64_t max_lag,
                                         int stat, uint64_t n_const, const uint32_t* d_nobs, uint64_t nobs_row_pitch,
                                         uint64_t nobs_col_stride, const uint32_t* d_lo, const uint32_t* d_hi,
                                         const float* d_annot, uint64_t annot_ld, uint64_t n_annot, float* d_score,
                                         uint64_t score_ld, uint32_t* d_n_pairs);
int storm_hip_lag_dosage_ldscore_annot_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                              uint64_t max_lag, const uint32_t* h_lo, const uint32_t* h_hi, const float* d_annot,
                                              uint64_t annot_ld, uint64_t n_annot, float* d_score, uint64_t score_ld,
                                              uint32_t* d_n_pairs);
int storm_hip_lag_dosage_ldscore_annot(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                       uint64_t max_lag, const uint32_t* h_lo, const uint32_t* h_hi, const float* h_annot,
                                       uint64_t annot_ld, uint64_t n_annot, float* h_score, uint64_t score_ld, uint32_t* h_n_pairs);
int storm_hip_lag_dosage_ldscore_annot_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat,
                                                       uint64_t n_samples, uint64_t max_lag, const uint32_t* h_lo,
                                                       const uint32_t* h_hi, const float* d_annot, uint64_t annot_ld,
                                                       uint64_t n_annot, float* d_score, uint64_t score_ld, uint32_t* d_n_pairs);
int storm_hip_lag_dosage_ldscore_annot_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples,
                                                uint64_t max_lag, const uint32_t* h_lo, const uint32_t* h_hi, const float* h_annot,
                                                uint64_t annot_ld, uint64_t n_annot, float* h_score, uint64_t score_ld,
                                                uint32_t* h_n_pairs);

/* ---- greedy LD pruning and clumping from a band in the lag layout, resolved on the device ---------------------------
 * storm_hip_lag_band_prune_device: d_vals is any float matrix in the lag layout in DEVICE memory (as in
 *   storm_hip_lag_band_sums_device: the pair (i, i + 1 + d) at d_vals[i * ld + d], L = min(max_lag, n_rows - 1), ld >= L).
 *   Rows i < j are ADJACENT when j - i <= L, j <= h_hi[i] and i >= h_lo[j] (both NULL: the lag alone; storm.h's planner
 *   makes bounds for which the two tests agree), and d_vals' float of the pair > min_r2, compared as floats, strictly (a NaN
 *   float is never an edge). The rows are walked in the order h_order[0], h_order[1], .. (a permutation of the rows; NULL:
 *   row order) and a row is KEPT exactly when no row kept before it is adjacent to it — the lexicographically first
 *   maximal independent set:
 *     d_keep[i]  = 1 or 0 (uint8_t),
 *     d_owner[i] = i for a kept row, else the kept row adjacent to it that comes first in the order (may be NULL; d_keep is
 *                  the same bytes either way).
 *   Exactly elements [0, n_rows) of the outputs, in DEVICE memory, are written. h_lo, h_hi, h_order are HOST arrays of
 *   n_rows uint32 in every form; the corner and the pitch columns of d_vals are never read. Three kernels
 *   (lag_band_threshold_kernel: one adjacency bit mask per row, the band read once; band_mis_resolve_kernel: ONE workgroup,
 *   the removed bits of all rows in 128 KiB of LDS, hence n_rows <= 2^20; band_mis_owner_kernel: only with d_owner), no
 *   atomics on floats and nothing that waits for another workgroup: two calls return the same bytes. Device scratch in the
 *   context's band buffer: n x (2 ceil(L / 32) + 2) words of masks, 2 n words of bounds, 2 n words of order and rank.
 *   Queued on the context's stream; no host wait: h_lo / h_hi / h_order must stay unchanged until that work is complete
 *   (storm_hip_ctx_synchronize). The LD r^2 of storm_hip_pairw_lag_similarity_device goes through the same call.
 * storm_hip_lag_dosage_prune[_complete][_device]: rows of 2-bit dosages: the band of r^2 as in
 *   storm_hip_lag_dosage_ldscore[_complete] into the context's band buffer, then the kernels above. The host forms copy n
 *   bytes (and n words when h_owner is given) back and wait; the _device forms take d_keep / d_owner in device memory and
 *   return with everything queued: h_lo / h_hi / h_order must stay unchanged until that work is complete
 *   (storm_hip_ctx_synchronize).
 * STORM_HIP_EINVAL: NULL context, band / matrix or keep, max_lag 0, ld < L, (dosage forms: rows of more than 2^24 values,
 * n_samples that does not match the row width,) one of lo / hi without the other, more than 2^20 rows (never truncated), a
 * NaN min_r2, an order that is not a permutation. STORM_HIP_ENOMEM names the buffer. Fewer than two rows: STORM_HIP_OK,
 * nothing written — except that the dosage forms answer a matrix of exactly ONE row: keep[0] = 1, owner[0] = 0 (a row
 * without any edge is kept and owns itself), so that storm.h's _device forms have someone to write it. */
int storm_hip_lag_band_prune_device(storm_hip_ctx_t* ctx, const float* d_vals, uint64_t ld, uint64_t n_rows, uint64_t max_lag,
                                    float min_r2, const uint32_t* h_lo, const uint32_t* h_hi, const uint32_t* h_order,
                                    uint8_t* d_keep, uint32_t* d_owner);
int storm_hip_lag_dosage_prune_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                      float min_r2, const uint32_t* h_lo, const uint32_t* h_hi, const uint32_t* h_order,
                                      uint8_t* d_keep, uint32_t* d_owner);
int storm_hip_lag_dosage_prune(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag, float min_r2,
                               const uint32_t* h_lo, const uint32_t* h_hi, const uint32_t* h_order, uint8_t* h_keep,
                               uint32_t* h_owner);
int storm_hip_lag_dosage_prune_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples,
                                               uint64_t max_lag, float min_r2, const uint32_t* h_lo, const uint32_t* h_hi,
                                               const uint32_t* h_order, uint8_t* d_keep, uint32_t* d_owner);
int storm_hip_lag_dosage_prune_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                        float min_r2, const uint32_t* h_lo, const uint32_t* h_hi, const uint32_t* h_order,
                                        uint8_t* h_keep, uint32_t* h_owner);

/* ---- the sparse pair list of a band in the lag layout, compacted on the device ------------------------------------------
 * storm_hip_lag_band_sparse_device: d_vals is any float matrix in the lag layout in DEVICE memory, as in
 *   storm_hip_lag_band_prune_device, and a pair i < j is LISTED exactly when it is adjacent there: j - i <= L =
 *   min(max_lag, n_rows - 1), j <= h_hi[i] and i >= h_lo[j] (both NULL: the lag alone), and d_vals' float of the pair >
 *   min_r2, compared as floats, strictly (a NaN float is never listed; a negative min_r2 lists every pair that is a number).
 *   The output is CSR over the forward pairs, in DEVICE memory:
 *     d_row_start[0 .. n_rows]  uint64: row i's pairs are the slots [d_row_start[i], d_row_start[i + 1]); [n_rows] the total,
 *     d_col[s]                  uint32: j, ascending within a row,
 *     d_val[s]                  the very float of d_vals (the same 32 bits).
 *   d_row_start always holds the true offsets. Only the slots below `capacity` are written — the first `capacity` pairs in
 *   (i, j) order — and nothing is written at or behind d_col[capacity] / d_val[capacity]: the caller compares
 *   d_row_start[n_rows] with capacity. d_col and d_val NULL with capacity 0 is the count-only call. h_lo / h_hi are HOST
 *   arrays of n_rows uint32; the corner and the pitch columns of d_vals are never read. Five plain launches
 *   (lag_band_sparse_count_kernel: one 64-bit forward mask word per 64 lags and one count per row, the band read once;
 *   three launches of a reduce-then-scan over the counts; lag_band_sparse_fill_kernel: reads the masks and, of the band, the
 *   listed entries only), no atomics and nothing that waits for another workgroup: two calls return the same bytes. Device
 *   scratch in the context's band buffer: n x ceil(L / 64) 64-bit words of masks, a 64-bit sum per 1024 rows, n words of
 *   counts, 2 n words of bounds. Queued on the context's stream; no host wait: h_lo / h_hi must stay unchanged until that
 *   work is complete (storm_hip_ctx_synchronize). Fewer than two rows: d_row_start[0 .. n_rows] = 0. The LD r^2 of
 *   storm_hip_pairw_lag_similarity_device goes through the same call.
 * storm_hip_lag_dosage_corr_sparse[_complete][_device]: rows of 2-bit dosages: the band of r^2 as in
 *   storm_hip_lag_dosage_ldscore[_complete] into the context's band buffer, then the kernels above. The _device forms take
 *   d_row_start / d_col / d_val in device memory and return with everything queued. The host forms stage the list behind the
 *   band (min(capacity, n L) entries), copy the offsets back, wait, write the total to *h_n_pairs (may be NULL) and copy
 *   exactly that many entries of col and val; a total above capacity is STORM_HIP_EINVAL with h_row_start and *h_n_pairs
 *   valid and the message naming both numbers.
 * STORM_HIP_EINVAL: NULL context, band / matrix or row_start, max_lag 0, ld < L, (dosage forms: rows of more than 2^24 values,
 * n_samples that does not match the row width,) one of lo / hi without the other, one of col / val without the other or a
 * capacity without them, 2^32 rows or more, a NaN min_r2. STORM_HIP_ENOMEM names the buffer. */
int storm_hip_lag_band_sparse_device(storm_hip_ctx_t* ctx, const float* d_vals, uint64_t ld, uint64_t n_rows, uint64_t max_lag,
                                     float min_r2, const uint32_t* h_lo, const uint32_t* h_hi, uint64_t* d_row_start,
                                     uint32_t* d_col, float* d_val, uint64_t capacity);
int storm_hip_lag_dosage_corr_sparse_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                            float min_r2, const uint32_t* h_lo, const uint32_t* h_hi, uint64_t* d_row_start,
                                            uint32_t* d_col, float* d_val, uint64_t capacity);
int storm_hip_lag_dosage_corr_sparse(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                     float min_r2, const uint32_t* h_lo, const uint32_t* h_hi, uint64_t* h_row_start, uint32_t* h_col,
                                     float* h_val, uint64_t capacity, uint64_t* h_n_pairs);
int storm_hip_lag_dosage_corr_sparse_complete_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples,
                                                     uint64_t max_lag, float min_r2, const uint32_t* h_lo, const uint32_t* h_hi,
                                                     uint64_t* d_row_start, uint32_t* d_col, float* d_val, uint64_t capacity);
int storm_hip_lag_dosage_corr_sparse_complete(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag,
                                              float min_r2, const uint32_t* h_lo, const uint32_t* h_hi, uint64_t* h_row_start,
                                              uint32_t* h_col, float* h_val, uint64_t capacity, uint64_t* h_n_pairs);

/* sum_c C(n_c,2) on the device — verification identity only, never the product
 * path: used by tests at sizes where a CPU pairwise oracle is infeasible */
int storm_hip_column_identity(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m,
                              uint64_t* h_total);

/* kernel selection / tuning knobs (benchmarks; defaults are what ships; none changes a result)
 *   key "variant": -1 = auto (default): matrix-core strips (4) whenever 64 shadow rows fit 32-bit
 *                  DMA offsets, else the popcount kernel (2)
 *                  0/1/2 = K1 popcount kernel, B operand direct / via VGPR->LDS / via LDS-DMA
 *                  3 = K2 FP4 matrix-core tiles, 4 = K2s FP4 matrix-core strips (256-row A tiles),
 *                  5 = wide strips (512-row A tiles)
 *   key "keep_shadow": 1 = keep the FP4 shadow of a dense matrix between all-pairs calls while the
 *                  matrix is unchanged (default 0). Only valid when the matrix is modified through
 *                  this library alone (upload / import / set_rows / fill / clear), never through
 *                  storm_hip_matrix_device_ptr. storm.h handles use it.
 *   key "time_kernels": see storm_hip_kernel_time
 *   key "sparse_probe": sparse container, block columns whose blocks are all lists: -1 = auto (the
 *                  list-probe kernel K4 when the mean list has <= 1000 positions, else the dense path),
 *                  0 = never, 1 = every eligible column
 *   key "seg_rows": K1 B rows per work item (default 256)
 *   key "chunks_per_item": K1 k-chunks (64 words each) per work item, 0 = auto
 *   key "k2_stages_per_item": K2 tile kernel k-slice length in 128-bit stages (default 32)
 *   keys "k2_max_run" (128), "k2_tail_slices" (3), "k2_tail_run" (32): strip work-list shaping; once either tail key
 *        is set on a context both hold as they stand, until then the 128-rows-per-wave strips choose them for one
 *        device's whole pass; read-only "k2_max_run_used", "k2_tail_run_used", "k2_tail_slices_used": the shaping of
 *        the strip list planned last (0 before the first);
 *        "k2_persistent" (0): per-XCD work queues; "k2_ring" (4): LDS ring depth 3..5;
 *        "k2_pitch_pad" (-1 = auto): extra bytes per shadow row; "k2_lds_pad": cap workgroups per CU;
 *        "k2_matrix_split" (1): cut the last round of matrix-output tiles along k;
 *        "k2_shape" (16): MFMA form of the default strips, 16 = 16x16x128, 32 = 32x32x64;
 *        "k2_strip_operands" (0): operands of the strips: 0 / 5 = the bit matrix itself, the FP4 image of every B
 *        stage built in the LDS by the workgroup (K2b, the default); 4 = FP4 shadow (expansion pass + strips); 2 = one
 *        stage stream per workgroup on bit operands (K2q); 1 / 3: tools build only;
 *        "k2_strip_rows" (0): K2b's A rows per wave: 64 = 256-row A tiles on slices of a class pair of 512 bits
 *        (strip16_bits_kernel); 128 = 512-row A tiles on slices of 128 bits, one image store and four fragment reads per
 *        stage instead of two and eight (strip16_rows_kernel) — only where the matrix's zero rows reach the next multiple
 *        of 512, otherwise 64 runs; 0 = by measurement: 128 for one device's whole pass over 2048 rows x 65536 bits and
 *        more. Read-only "k2_strip_rows_used": what the last K2b launch ran ("k2_operands_used" is 5 for both);
 *        "k2_tile_shape" (0): materialised-output kernel: 0 = by the matrix (5 for a dense matrix, 2 for the dense
 *        replica of a sparse container); 5 = tilering_kernel: both operands as FP4 images built once per workgroup in the
 *        LDS, 16x16x128 MFMAs, SIMD partners half a stage apart ("k2_ring_sync" (0): 0 = one barrier per stage, 1 = arrival
 *        counters in the LDS); 2 / 1 = bit operands inflated to FP4 in registers, 32x32x64 MFMAs (two / one wave per SIMD);
 *        3 / 4 = B as LDS images, A in registers; 16 / 32 = the FP4-shadow kernels (1, 16: tools build only);
 *        "k2_fold_inline" (-1): the all-pairs total is folded inside the last kernel of the pass by the workgroup dispatched
 *        last (-1: for short launches, where the fold launch and its gaps are a fifth of a pass; 1: always; 0: never);
 *        "k2_tile_cost_diag" (63), "k2_tile_cost_ragged" (30): percent of a full tile's time the
 *        planner assumes for diagonal / ragged-column tiles when it cuts the last round into k-parts;
 *        "k2_shadow_budget_mb" (98304): when the FP4 shadow (4 x the bits) of a matrix would exceed
 *        this many MiB the pass runs k-chunk by k-chunk over a compact shadow of one chunk
 *        (HBM-tiled: bounded footprint for any M x N; 0 = never chunk)
 *   key "k2_debug", "k2_ring" >= 11: timing probes only (results may then be wrong), see
 *        storm_hip_mfma.hip
 *   read-only "variant_used": what the last dense launch ran; "n_cus" */
int storm_hip_ctx_set_option(storm_hip_ctx_t* ctx, const char* key, int64_t value);
/* Whether storm_hip_ctx_set_option would accept (key, value), without a context (STORM_HIP_OK, or STORM_HIP_EINVAL with
 * storm_hip_last_error() saying why): callers that remember options for contexts still to be made validate with it. */
int storm_hip_option_check(const char* key, int64_t value);
/* Allocates the context's pinned staging ring (24 MiB, what the sparse arena builder ships lists and blocks through) now
 * instead of inside the first arena build: callers that know an arena is coming (storm.h's STORM_add) call it while nobody
 * is waiting for a result (5 - 6 ms of a first all-pairs call otherwise). */
int storm_hip_ctx_reserve_staging(storm_hip_ctx_t* ctx);
int64_t storm_hip_ctx_get_option(storm_hip_ctx_t* ctx, const char* key);
/* Tuning aid: with option "k2_ring" = 18 the strip kernel records, per work item, its start and
 * end on the 100 MHz device counter, three phase marks (operands in / diagonal phase done / main
 * loop done, 16 bits each, relative to the start) and the XCC_ID register of the workgroup's first
 * wave. out[i*8 ..] = {start, end, phases, xcc_id, a_row0, diag, stages, k-slice}; results of the
 * launch are unaffected. `out` may be NULL to query the item count. */
int storm_hip_debug_strip_trace(storm_hip_ctx_t* ctx, uint64_t* out, uint64_t capacity_items,
                                uint64_t* n_items);

/* Duration of the dominant kernel alone (the popcount, tile or strip kernel — not the FP4
 * expansion or the final fold), for roofline accounting: with option "time_kernels" = 1 every
 * pairwise launch brackets that kernel with HIP events on the launch stream. This call waits for
 * the stream, returns the summed duration and the number of launches since the last call, and
 * starts a new series. "time_kernels" = 0 pauses the bracketing and keeps the series, 2 resumes it
 * (1 starts a new one): bench.py brackets every 4th step at N > 1. */
int storm_hip_kernel_time(storm_hip_ctx_t* ctx, double* sum_ms, uint64_t* launches);
/* work decomposition of the last dense launch: out[0]=work items, [1]=k-chunks per item,
 * [2]=word-pairs executed incl. zero padding (popcount kernel) / k-chunks of the pass (matrix-core
 * strips: 1 unless the shadow budget forced HBM tiling), [3]=segments (popcount kernel) / block columns
 * counted by the list-probe kernel (sparse container) */
int storm_hip_last_launch_info(storm_hip_ctx_t* ctx, uint64_t out[4]);

/* ---- multi-GPU work split of the default (matrix-core strip) path, host-only ---------------
 * The work list shard `shard_rank` of `shard_count` would multiply for an n_rows x n_words
 * matrix, as 5 uint32 per item: {a_row0, diag, j0, j1, ks} =
 *   A tile rows [a_row0, a_row0 + 256) x k-slice ks (bits [256 ks, 256 ks + 256) of every row) x
 *   (diag ? the strict upper triangle inside the A tile : nothing) + the 64-row B blocks
 *   [j0, j1) (rows [64 j0, 64 j1)), i.e. the pairs (i, j), i in the A tile, j in those blocks.
 * Ownership: whole k-slices, in units of 4 (one 128-byte line of the bit matrix), go
 * to shard (ks / 4) % shard_count; the leftover slices (fewer than 4 x shard_count) are cut along
 * the pair space, longest item first onto the least loaded shard. The lists of all shards tile (pair, k-slice) space exactly once. Touches no
 * device; `out` may be NULL to query the item count. Shards the reference loop storm.c:1199-1238. */
int storm_hip_strip_plan(uint64_t n_rows, uint32_t n_words, uint32_t shard_rank,
                         uint32_t shard_count, uint32_t* out, uint64_t capacity_items,
                         uint64_t* n_items);
/* The same with the operand form and the ownership mode spelled out (storm_hip_strip_plan = form 0, mode 0):
 *   form 0: the FP4-shadow strips: slice ks = bits [256 ks, 256 ks + 256) of every row;
 *   form 1: the strips on bit operands (K2b, the DEFAULT path): slice ks = class pair ks & 1 — the bits b of
 *           the 512-bit chunk ks / 2 (bits [512 (ks / 2), +512)) with (b % 4) / 2 == ks & 1 — 256 bit positions
 *           as well; 2 x ceil(n_words / 8) slices;
 *   form 2: K2b with 128 A rows per wave (option k2_strip_rows = 128): slice ks = bits [128 ks, 128 ks + 128) of
 *           every row, ceil(n_words / 2) slices; the A tile is 512 rows (a_row0 a multiple of 512, 8 own blocks), the
 *           ownership units are 4 slices = 64 bytes of every row;
 *   pair_space 0: whole k-slices first, leftover slices along the pair space (above);
 *   pair_space 1: EVERY slice is cut along the pair space (context option k2_shard_pairs): a shard multiplies
 *           its share of every slice's items (longest first onto the least loaded shard, the load carried
 *           from slice to slice). */
int storm_hip_strip_plan2(uint64_t n_rows, uint32_t n_words, uint32_t shard_rank, uint32_t shard_count,
                          int form, int pair_space, uint32_t* out, uint64_t capacity_items, uint64_t* n_items);
/* The same with the work-list options spelled out — the context options of the same names, and the device's
 * compute-unit count (context option "n_cus", read-only) — i.e. EXACTLY the list a context with these options
 * launches for this shard: one function derives the shaping for the device path and for this planner. max_run = 0
 * selects the run length automatically (64 / 96 / 128, whichever schedules the SLOWEST of the shard_count ranks
 * shortest: the choice never depends on shard_rank, so that all ranks cut the slices they deal among themselves at
 * the same length); *run_chosen (may be NULL) receives the run length used.
 * tail_run = 0 stands for a context on which neither k2_tail_run nor k2_tail_slices was set (tail_slices is then not
 * read): form 2 with shard_count 1 chooses run length and tail together, from a fixed set of candidates by a model of
 * what an XCD makes of its list, and orders its items by what they cost in that model; every other list
 * takes tail_run 32 and tail_slices 3. *run_chosen then receives max_run | tail_run << 16 | tail_slices << 24 as used.
 * tail_run >= 1 gives the list of a context with both options set to these values.
 * storm_hip_strip_plan2 = the defaults (max_run 0, no tail set, lpt_rounds 6, 256 compute units). */
int storm_hip_strip_plan3(uint64_t n_rows, uint32_t n_words, uint32_t shard_rank, uint32_t shard_count,
                          int form, int pair_space, int max_run, int tail_run, int tail_slices, int lpt_rounds,
                          uint32_t n_cus, uint32_t* out, uint64_t capacity_items, uint64_t* n_items,
                          int* run_chosen);

/* The item list of the materialised-output kernel for matrices of few 256 x 256 tiles (K2h, tile128_kernel; DESIGN.md
 * §4) on a device of `n_cus` compute units, as 8 uint32 per item, in launch order:
 *   {I, J, first chunk, chunks, tile, part, n_parts, narrow}
 *   = the pairs (row of the 128-row tile I, row of the 128-row tile J) over the 512-bit chunks [first, first + chunks) of
 *     every row; `tile` numbers the tiles, an item is part `part` of the `n_parts` its tile is cut into along k (their
 *     sums meet inside the launch; `narrow`: through windows of 16-bit counts).
 * n_rows_b == 0: the triangle of one matrix of n_rows_a rows (tiles I <= J), band_rows != 0: only the output rows
 * [band_row0, band_row0 + band_rows); n_rows_b != 0: the rectangle A x B (B's tiles count on behind A's rows padded to a
 * multiple of 256). slots_per_cu / min_chunks / diag_cost_pct: the context options k2_part_slots / k2_part_min_chunks /
 * k2_part_cost_diag. The items of a tile cover its chunks exactly once, the tiles every pair of the output exactly once.
 * Cuts the reference loop storm.c:1199-1238 (its per-pair results kept). Host only; `out` may be NULL to query the count. */
int storm_hip_matrix_plan(uint64_t n_rows_a, uint64_t n_rows_b, uint32_t n_words, uint64_t band_row0, uint64_t band_rows,
                          uint32_t n_cus, int slots_per_cu, int min_chunks, int diag_cost_pct, uint32_t* out,
                          uint64_t capacity_items, uint64_t* n_items);

/* The K2h list of the dosage form (storm_hip_pairw_dosage_matrix_device): arguments and records as storm_hip_matrix_plan
 * for a matrix of n_words words of 2-bit values, planned with what a chunk of such values can add to an accumulator
 * (9 x 256 instead of 512): an item covers at most 7281 chunks (chunks x 2304 <= 2^24, exact f32 accumulation), and a
 * tile's windows are narrow only while a part covers at most 28 (chunks x 2304 <= 65535). Triangle only: n_rows_b must
 * be 0. Host only; `out` may be NULL to query the count. */
int storm_hip_dosage_plan(uint64_t n_rows_a, uint64_t n_rows_b, uint32_t n_words, uint64_t band_row0, uint64_t band_rows,
                          uint32_t n_cus, int slots_per_cu, int min_chunks, int diag_cost_pct, uint32_t* out,
                          uint64_t capacity_items, uint64_t* n_items);

/* The same for the dosage form's rectangle (storm_hip_square_dosage_matrix_device): every 128 x 128 tile of
 * n_rows_a x n_rows_b, I over A's tiles and J counting on behind A's rows padded to 256 (storm_hip_matrix_plan's
 * rectangle), under the same two limits. Host only; `out` may be NULL to query the count. */
int storm_hip_dosage_square_plan(uint64_t n_rows_a, uint64_t n_rows_b, uint32_t n_words, uint32_t n_cus, int slots_per_cu,
                                 int min_chunks, int diag_cost_pct, uint32_t* out, uint64_t capacity_items, uint64_t* n_items);

/* The K2h list of the lag layout (storm_hip_pairw_lag_matrix_device): the same records for the triangle's tiles (I, J) that
 * hold a pair with j - i <= L = min(max_lag, n_rows - 1), I <= J <= (128 I + 127 + L) / 128; band_rows == 0: all rows.
 * max_lag >= n_rows - 1 lists what storm_hip_matrix_plan lists for the triangle. Host only; `out` may be NULL. */
int storm_hip_lag_plan(uint64_t n_rows, uint32_t n_words, uint64_t max_lag, uint64_t band_row0, uint64_t band_rows,
                       uint32_t n_cus, int slots_per_cu, int min_chunks, int diag_cost_pct, uint32_t* out,
                       uint64_t capacity_items, uint64_t* n_items);

/* The K2h list of the dosage form in the lag layout (storm_hip_pairw_lag_dosage_matrix_device): storm_hip_lag_plan's tiles
 * for a matrix of n_words words of 2-bit values, under storm_hip_dosage_plan's two limits (7281 chunks per item, narrow
 * windows up to 28 chunks per part). Host only; `out` may be NULL. */
int storm_hip_lag_dosage_plan(uint64_t n_rows, uint32_t n_words, uint64_t max_lag, uint64_t band_row0, uint64_t band_rows,
                              uint32_t n_cus, int slots_per_cu, int min_chunks, int diag_cost_pct, uint32_t* out,
                              uint64_t capacity_items, uint64_t* n_items);

/* The same for the one-launch stage stream on bit operands (K2q, the default for matrices of up to 8192
 * rows on one device): the segments shard `shard_rank` of `shard_count` walks on a device of
 * `n_cus` compute units, workgroup by workgroup, as 8 uint32 per segment:
 *   {workgroup, a_blk, ks, b_first, n_b, range_nb, diag, stages}
 *   = A tile = the 64-row blocks [a_blk, a_blk + 4) x k-slice ks (bits [512 ks, 512 ks + 512) of every row);
 *     diag ? the pairs inside the tile (strictly above the diagonal) : nothing; then the n_b later blocks
 *     (b_first + i) % range_nb, i < n_b, whole: the pairs (row of the tile, row of the block).
 * Tile pairs are dealt cyclically (tile I takes the (T - 1) / 2 tiles behind it, wrapping around; with an
 * even number of tiles the opposite one goes to the lower tile on even k-slices and to the upper on odd ones),
 * so the segments of all shards cover every unordered row pair x k-slice exactly once. Shards the reference
 * loop storm.c:1199-1238 into contiguous parts of the k-slice-major stage stream. Host only. */
int storm_hip_stream_plan(uint64_t n_rows, uint32_t n_words, uint32_t shard_rank, uint32_t shard_count,
                          uint32_t n_cus, uint32_t* out, uint64_t capacity_segments, uint64_t* n_segments,
                          uint32_t* n_workgroups);

/* ---- the 8-byte exchange of a multi-process run (one process per GPU), over RCCL / xGMI ----------------
 * Every rank computes its shard's partial (storm_hip_pairw_dense(..., shard_rank, shard_count), or a storm.h
 * handle after STORM_hip_set_shard) and the partials are summed: ncclAllReduce(count 1, ncclUint64, ncclSum)
 * — SURVEY §5; the reference is single-process and has no counterpart. librccl.so is loaded on first use
 * (dlopen; STORM_HIP_RCCL names another build), single-GPU users need none.
 *   rank 0: storm_hip_comm_unique_id(id); hand the 128 bytes to the other ranks (pipe, file, MPI, ...);
 *   every rank, AFTER forking / starting its own process and BEFORE the first collective:
 *     storm_hip_comm_init_rank(ctx, id, rank, world, &comm)      (collective: all ranks call it)
 *   per all-pairs call: storm_hip_comm_allreduce_u64(ctx, comm, &value)   value := sum over ranks, or
 *     storm_hip_pairw_dense_begin(...) + storm_hip_comm_allreduce_result(ctx, comm, &total): the shard's
 *     partial is reduced where the pass left it (the context's result word), one host wait for both.
 * tools/storm_benchmark.cpp --ranks N is a complete example (fork before any HIP call, id through a pipe). */
#define STORM_HIP_COMM_ID_BYTES 128
typedef struct storm_hip_comm_s storm_hip_comm_t;
/* What the last all-pairs pass of this context ran: out[0] = mask of STORM_HIP_RAN_*; out[1] = 64-bit word pairs
 * multiplied by the dense kernels (pairs x words, this shard's share); out[2] = positions streamed by the
 * list-probe kernel (= its lookups: one 2-byte LDS read + one add each); out[3] = rows of the group one lookup
 * stands for (128: a lookup is 128 of the reference's per-pair list tests, storm.c:4-73, folded into a count).
 * For a harness that prices a row against the roof of the kernel that ran (tools/storm_benchmark.cpp). */
#define STORM_HIP_RAN_POPCOUNT 1u   /* pairw_dense_kernel (VALU popcount)                 roof: VALU issue     */
#define STORM_HIP_RAN_FP4_TILES 2u  /* pairw_fp4_kernel on the FP4 shadow                 roof: FP4 matrix cores */
#define STORM_HIP_RAN_FP4_STRIPS 4u /* strip16_fp4_kernel on the FP4 shadow               roof: FP4 matrix cores */
#define STORM_HIP_RAN_BITSTREAM 8u  /* bitstream_kernel (K2q), bit operands               roof: FP4 matrix cores */
#define STORM_HIP_RAN_BIT_STRIPS 16u /* strip16_bits_kernel (K2b), bit operands (default) roof: FP4 matrix cores */
#define STORM_HIP_RAN_LIST_PROBE 32u /* probe_lists_kernel (K4), list x list blocks       roof: LDS lookups    */
#define STORM_HIP_RAN_TILES_OUT 128u  /* tilering_kernel / tilebits8_kernel: per-pair output of a dense matrix (or replica) roof: FP4 matrix cores */
#define STORM_HIP_RAN_LISTS_MATRIX 64u /* lists_matrix_kernel (K5), per-pair output from the lists: out[2] = its table lookups, out[3] = 64 */
#define STORM_HIP_RAN_LISTS_SQUARE 256u /* lists_square_kernel (K5x), the rectangle of two list-only containers: out[2] = its table lookups, out[3] = 64 */
#define STORM_HIP_RAN_SIMILARITY 512u /* the finishing pass (finish_tiles_kernel, finish_lag_tiles_kernel) behind one of the per-pair kernels above (its flag stays set), or alone (storm_hip_similarity_finish_device)  roof: HBM bandwidth */
#define STORM_HIP_RAN_TOPK 1024u /* topk_rows_kernel behind the panels' count kernel (its flag stays set), or alone (storm_hip_topk_rows_device)  roof: HBM bandwidth */
int storm_hip_last_pass_report(storm_hip_ctx_t* ctx, uint64_t out[4]);

int storm_hip_comm_unique_id(uint8_t id[STORM_HIP_COMM_ID_BYTES]);
int storm_hip_comm_init_rank(storm_hip_ctx_t* ctx, const uint8_t id[STORM_HIP_COMM_ID_BYTES], uint32_t rank,
                             uint32_t world, storm_hip_comm_t** out);
int storm_hip_comm_allreduce_u64(storm_hip_ctx_t* ctx, storm_hip_comm_t* comm, uint64_t* value);
/* up to 8 words in one collective (e.g. {partial, failure flag}: a failed rank still enters it) */
int storm_hip_comm_allreduce_u64s(storm_hip_ctx_t* ctx, storm_hip_comm_t* comm, uint64_t* values, uint32_t n);
int storm_hip_comm_allreduce_result(storm_hip_ctx_t* ctx, storm_hip_comm_t* comm, uint64_t* total);
uint32_t storm_hip_comm_rank(const storm_hip_comm_t* comm);
uint32_t storm_hip_comm_world(const storm_hip_comm_t* comm);
void storm_hip_comm_destroy(storm_hip_comm_t* comm);

/* ---- sparse (STORM_t) arena: flattened rows -> blocks (storm.h:157-178) --------------
 * Host-side flat description of all rows' 65536-bit blocks:
 *   row_block_offset[n_rows+1]   CSR over blocks
 *   block_id[n_blocks]           ascending within a row (storm.c:711-723)
 *   block_kind[n_blocks]         0 = uint16 list, 1 = 1024-word bitmap (storm.c:745-749)
 *   block_data_offset[n_blocks]  offset into list_pool (uint16 units) or bitmap_pool (words)
 *   block_n[n_blocks]            list length (kind 0)
 * Replaces STORM_pairw_intersect_cardinality[_blocked] (storm.c:877-961) and the per-pair
 * dispatch STORM_bitmap_cont_intersect_cardinality_premade / STORM_bitmap_intersect_
 * cardinality_func (storm.c:790-814, :618-656). */
int storm_hip_sparse_create(storm_hip_ctx_t* ctx, uint64_t n_rows, uint64_t n_blocks,
                            const uint64_t* row_block_offset, const uint32_t* block_id,
                            const uint8_t* block_kind, const uint64_t* block_data_offset,
                            const uint32_t* block_n, const uint16_t* list_pool,
                            uint64_t list_pool_len, const uint64_t* bitmap_pool,
                            uint64_t bitmap_pool_words, storm_hip_sparse_t** out);
/* the same arena from a serialized STORM_t (STORM_serialize, storm.h; sizes as reference
 * storm.c:372-394): the host walks the headers only, the payload bytes go up as they are and both
 * block kinds are unpacked on the device. `buf` 2-byte aligned. */
/* The same from per-block POINTERS into the caller's own containers (what storm.h's STORM_t handles use: nothing
 * is flattened on the host): block_ptr[b] = the block's sorted uint16 list (block_n[b] entries, kind 0; 2-byte
 * aligned) or its 1024 words (kind 1; any alignment). The library walks the block headers, ships the raw lists
 * and bitmaps through a pinned staging ring and lays the list elements out on the device. */
int storm_hip_sparse_create_blocks(storm_hip_ctx_t* ctx, uint64_t n_rows, uint64_t n_blocks,
                                   const uint64_t* row_block_offset, const uint32_t* block_id,
                                   const uint8_t* block_kind, const uint32_t* block_n,
                                   const void* const* block_ptr, storm_hip_sparse_t** out);
/* [r6] Block stage: the bitmap blocks of a container travel to the device while the caller is still building it
 * (storm.h's STORM_add hands every bitmap block it finishes to one), so that the first all-pairs call — the one call
 * the reference's harness times, benchmark.cpp:605-613 — does not carry them over the bus. storm_hip_stage_add copies
 * the block's 1024 words into a pinned ring (sent 4 MiB at a time into 64 MiB device chunks) and returns its token;
 * storm_hip_sparse_create_blocks_staged builds the arena of storm_hip_sparse_create_blocks with the pool rows gathered
 * from the stage when EVERY bitmap block carries a valid token (token[b] < storm_hip_stage_count), and from block_ptr
 * otherwise; list blocks: a token of storm_hip_stage_add_list or ~0 (from block_ptr). The stage may be destroyed once the arena exists.
 * A list token is the list's byte position in the stage's list space, which is cut into chunks of 64 MiB; a list never runs
 * across a chunk's end, so the bytes between a chunk's last list and its end (the gap) are never written. Both staged
 * builders refuse — STORM_HIP_EINVAL, *out NULL, storm_hip_last_error() names the stage token, nothing is sent or launched —
 * a list token (other than ~0) with block_n[b] = n that
 *   - is odd,
 *   - lies beyond the chunks the stage has written to,
 *   - lies in a gap, or
 *   - whose 2 n bytes run across its chunk's end or past the last list the chunk holds.
 * A token that points into the middle of a staged list is in bounds and is read as it lies. */
typedef struct storm_hip_stage_s storm_hip_stage_t;
int storm_hip_stage_create(storm_hip_ctx_t* ctx, storm_hip_stage_t** out);
int storm_hip_stage_add(storm_hip_ctx_t* ctx, storm_hip_stage_t* stage, const uint64_t* words, uint64_t* token);
/* The same for a LIST block (kind 0: n ascending 16-bit positions, 1 <= n <= 65536): the token is the list's place in the
 * stage and goes into token[b] of storm_hip_sparse_create_blocks_staged; a list block whose token is ~0 travels from
 * block_ptr[b] at build time, as in storm_hip_sparse_create_blocks (list and bitmap tokens are separate sequences). */
int storm_hip_stage_add_list(storm_hip_ctx_t* ctx, storm_hip_stage_t* stage, const uint16_t* list, uint32_t n, uint64_t* token);
uint64_t storm_hip_stage_count(const storm_hip_stage_t* stage);
void storm_hip_stage_destroy(storm_hip_ctx_t* ctx, storm_hip_stage_t* stage);
int storm_hip_sparse_create_blocks_staged(storm_hip_ctx_t* ctx, uint64_t n_rows, uint64_t n_blocks,
                                          const uint64_t* row_block_offset, const uint32_t* block_id,
                                          const uint8_t* block_kind, const uint32_t* block_n,
                                          const void* const* block_ptr, storm_hip_stage_t* stage, const uint64_t* token,
                                          storm_hip_sparse_t** out);
int storm_hip_sparse_create_serialized(storm_hip_ctx_t* ctx, const void* buf, uint64_t n_bytes,
                                       storm_hip_sparse_t** out);
/* The rows of such a container as a DENSE bit matrix on the device (row width = 65536 x (largest block id + 1) bits,
 * at most 2^25): what the per-pair output of a STORM_t runs on (storm.h: STORM_pairw_matrix) — a row pair of the
 * reference (block-id merge + 4-way kind dispatch, storm.c:790-814, :618-656) is popcount(row_i & row_j) over
 * exactly these bits. Same block description as storm_hip_sparse_create_blocks; blocks travel through the pinned
 * ring as they lie in the containers and are unpacked by the device. Destroy with storm_hip_matrix_destroy. */
int storm_hip_matrix_create_from_blocks(storm_hip_ctx_t* ctx, uint64_t n_rows, uint64_t n_blocks,
                                        const uint64_t* row_block_offset, const uint32_t* block_id,
                                        const uint8_t* block_kind, const uint32_t* block_n,
                                        const void* const* block_ptr, storm_hip_matrix_t** out);
/* ... with rows of at least min_blocks x 65536 bits (the common width of two containers whose rectangle is multiplied;
 * at most 512 blocks = 2^25 bits). 0: the container's own width, as above. */
int storm_hip_matrix_create_from_blocks_wide(storm_hip_ctx_t* ctx, uint64_t n_rows, uint64_t n_blocks,
                                             const uint64_t* row_block_offset, const uint32_t* block_id,
                                             const uint8_t* block_kind, const uint32_t* block_n,
                                             const void* const* block_ptr, uint32_t min_blocks, storm_hip_matrix_t** out);
void storm_hip_sparse_destroy(storm_hip_ctx_t* ctx, storm_hip_sparse_t* s);
/* [r5] K5 — the per-pair matrix of a LIST-ONLY container straight from its lists (replaces, for every pair at once,
 * STORM_bitmap_cont_intersect_cardinality, storm.c:790-814, with two list blocks meeting in
 * STORM_intersect_vector16_cardinality, storm.c:4-73). Same block description as storm_hip_sparse_create_blocks.
 * *out stays NULL (and the call returns STORM_HIP_OK) when the container is not eligible — a bitmap block, a row of
 * more than 65535 positions, more than 2^26 positions in all: the dense replica (storm_hip_matrix_create_from_blocks)
 * is the path then. _worthwhile: 1 when the lists are expected to beat the dense replica's multiply (l = NULL: 1 unless the
 * path is switched off, i.e. whether building the lists is worth a try; option
 * `matrix_lists`: -1 by density, 0 never, 1 whenever eligible; `matrix_lists_density`: the crossover in 1/10000).
 * _pairw_matrix_device: out[i * ld + j] = popcount(row_i OP row_j) for i < j, device memory, complete on return;
 * entries i >= j are not written. */
int storm_hip_rowlists_create_blocks(storm_hip_ctx_t* ctx, uint64_t n_rows, uint64_t n_blocks,
                                     const uint64_t* row_block_offset, const uint32_t* block_id,
                                     const uint8_t* block_kind, const uint32_t* block_n,
                                     const void* const* block_ptr, storm_hip_rowlists_t** out);
/* ... with the lists taken from a block stage (storm_hip_stage_add_list) when EVERY non-empty block carries a token
 * (token[b] != ~0); from block_ptr otherwise. The stage is only read. Tokens the stage cannot answer are refused as above,
 * before anything is allocated on the device. */
int storm_hip_rowlists_create_blocks_staged(storm_hip_ctx_t* ctx, uint64_t n_rows, uint64_t n_blocks,
                                            const uint64_t* row_block_offset, const uint32_t* block_id,
                                            const uint8_t* block_kind, const uint32_t* block_n,
                                            const void* const* block_ptr, storm_hip_stage_t* stage, const uint64_t* token,
                                            storm_hip_rowlists_t** out);
void storm_hip_rowlists_destroy(storm_hip_ctx_t* ctx, storm_hip_rowlists_t* l);
int storm_hip_rowlists_worthwhile(storm_hip_ctx_t* ctx, const storm_hip_rowlists_t* l);
/* the same rule from the counts alone (rows, listed positions, bits per row), BEFORE anything is built: a container the
 * rule sends to the dense replica should not pay for row lists it will not use (9 ms of a first call at 3670 positions
 * per row of BASELINE c4's shape) */
int storm_hip_rowlists_worthwhile_counts(storm_hip_ctx_t* ctx, uint64_t n_rows, uint64_t n_elems, uint64_t n_bits);
int storm_hip_rowlists_pairw_matrix_device(storm_hip_ctx_t* ctx, const storm_hip_rowlists_t* l, int op,
                                           uint32_t* d_out, uint64_t ld);
/* ... and into host memory: whole rows, zeros at i >= j (what storm_hip_pairw_matrix writes) */
int storm_hip_rowlists_pairw_matrix(storm_hip_ctx_t* ctx, const storm_hip_rowlists_t* l, int op, uint32_t* h_out,
                                    uint64_t ld);
uint64_t storm_hip_rowlists_n_elems(const storm_hip_rowlists_t* l);
/* [K5x] The rectangle of TWO list-only containers from their lists: A = la's rows, B = lb's (la == lb allowed), each built
 * by storm_hip_rowlists_create_blocks*. The window kernel's join with A's groups of 64 rows against B's chunks of 768 rows,
 * every tile (no triangle); windows beyond either container's universe are skipped. The hash join (K5h) has no cross form:
 * option matrix_lists_kernel = 2 still runs this one.
 *   _square_total          : *h_total = sum over i < n_A, j < n_B of |A_i & B_j| (integer fold on the device).
 *   _square_matrix_device  : out[i * ld + j] = popcount(A_i OP B_j) for EVERY i < n_A, j < n_B (ld >= n_B); device
 *                            memory, complete on return.
 *   _square_matrix         : the same into HOST memory, h_out[i * ld + j].
 * la's device copy caches the tile list of the last B (not its rows). */
int storm_hip_rowlists_square_total(storm_hip_ctx_t* ctx, storm_hip_rowlists_t* la, const storm_hip_rowlists_t* lb,
                                    uint64_t* h_total);
int storm_hip_rowlists_square_matrix_device(storm_hip_ctx_t* ctx, storm_hip_rowlists_t* la, const storm_hip_rowlists_t* lb,
                                            int op, uint32_t* d_out, uint64_t ld);
int storm_hip_rowlists_square_matrix(storm_hip_ctx_t* ctx, storm_hip_rowlists_t* la, const storm_hip_rowlists_t* lb, int op,
                                     uint32_t* h_out, uint64_t ld);
/* The similarity forms of the row lists (see storm_hip_similarity_finish_device): K5 / K5x with op AND, then the finish
 * with the lists' own row lengths as the counts. */
int storm_hip_rowlists_pairw_similarity_device(storm_hip_ctx_t* ctx, const storm_hip_rowlists_t* l, int measure,
                                               uint64_t n_bits, float* d_out, uint64_t ld);
int storm_hip_rowlists_pairw_similarity(storm_hip_ctx_t* ctx, const storm_hip_rowlists_t* l, int measure, uint64_t n_bits,
                                        float* h_out, uint64_t ld);
int storm_hip_rowlists_square_similarity_device(storm_hip_ctx_t* ctx, storm_hip_rowlists_t* la, const storm_hip_rowlists_t* lb,
                                                int measure, uint64_t n_bits, float* d_out, uint64_t ld);
int storm_hip_rowlists_square_similarity(storm_hip_ctx_t* ctx, storm_hip_rowlists_t* la, const storm_hip_rowlists_t* lb,
                                         int measure, uint64_t n_bits, float* h_out, uint64_t ld);

int storm_hip_pairw_sparse(storm_hip_ctx_t* ctx, const storm_hip_sparse_t* s,
                           uint32_t shard_rank, uint32_t shard_count, uint64_t* h_total);
/* split form (one host thread, one arena replica per GPU): _begin launches this shard into the
 * context's result word, _end waits for it and copies it to the host */
int storm_hip_pairw_sparse_begin(storm_hip_ctx_t* ctx, const storm_hip_sparse_t* s,
                                 uint32_t shard_rank, uint32_t shard_count);
int storm_hip_pairw_sparse_end(storm_hip_ctx_t* ctx, uint64_t* h_total);
/* work census of the last sparse call: out[0]=list×list block pairs, [1]=list×bitmap,
 * [2]=bitmap×bitmap, [3]=block columns */
int storm_hip_sparse_last_census(storm_hip_ctx_t* ctx, uint64_t out[4]);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* STORM_HIP_H_ */
