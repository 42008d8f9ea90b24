/*
 * storm.h — the StormBitmaps container API, served by the MI355X-native library
 * libstorm_hip.so (stormbitmaps_amd/). Source-compatible with the reference header
 * (mklarqvist/StormBitmaps storm.h): same type names, same public struct members in the same
 * order, same function signatures and return conventions, so a C/C++ caller of the reference
 * recompiles against this header and links -lstorm_hip instead of storm.c.
 *
 * What differs behind the API
 *   - The all-pairs entry points (STORM_contig_pairw_*, STORM_pairw_*, STORM_wrapper_*) run on
 *     the GPU: hand-written gfx950 kernels reached through the C-ABI shim in storm_hip.h.
 *     There is no CPU fallback; without a usable device they return (uint64_t)-1 and leave
 *     a message in storm_hip_last_error().
 *   - `bsize` / `block_size` arguments are accepted and ignored as tuning hints: the device
 *     tiling is chosen internally and the integer result does not depend on it.
 *   - Results follow the intended semantics (the mathematically exact count). The reference
 *     deviates from it in three sparse regimes (SURVEY.md §8 a-note, defects D1-D3).
 *   - *_free() also releases the handle itself and every device buffer.
 *   - The container structs and the block struct carry private members after the reference's public ones.
 *
 * Every declaration cites the reference lines it stands in for (storm.h / storm.c).
 */
#ifndef STORM_H_MI355X_DROPIN
#define STORM_H_MI355X_DROPIN

#include <assert.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "libalgebra/libalgebra.h" /* reference storm.h:33 */

/* reference storm.h:35-47 — kept for callers that size blocks with them */
#ifndef STORM_CACHE_BLOCK_SIZE
#define STORM_CACHE_BLOCK_SIZE 256e3
#endif
#ifndef STORM_DEFAULT_BLOCK_SIZE
#define STORM_DEFAULT_BLOCK_SIZE 65536
#endif
#ifndef STORM_DEFAULT_SCALAR_THRESHOLD
#define STORM_DEFAULT_SCALAR_THRESHOLD 4096
#endif

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: what these headers declare is its whole export list */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* ------------------------------------------------------------------ list kernels (host) --
 * Single-pair helpers on host memory (reference storm.h:56-61, storm.c:4-129). They are not
 * on the all-pairs path; they exist so that one-pair callers keep working. */
uint64_t STORM_intersect_vector16_cardinality(const uint16_t* STORM_RESTRICT v1,
                                              const uint16_t* STORM_RESTRICT v2,
                                              const uint32_t len1, const uint32_t len2);
uint64_t STORM_intersect_vector32_unsafe(const uint32_t* STORM_RESTRICT v1,
                                         const uint32_t* STORM_RESTRICT v2, const uint32_t len1,
                                         const uint32_t len2, uint32_t* STORM_RESTRICT out);
uint64_t STORM_intersect_bitmaps_scalar_list(const uint64_t* STORM_RESTRICT b1,
                                             const uint64_t* STORM_RESTRICT b2,
                                             const uint32_t* l1, const uint32_t* l2,
                                             const uint32_t n1, const uint32_t n2);

/* list-aware leaf signature (reference storm.h:66-67) */
typedef uint64_t (*STORM_compute_lfunc)(const uint64_t*, const uint64_t*, const uint32_t*,
                                        const uint32_t*, const size_t, const size_t);

/* ------------------------------------------------------ raw-buffer all-pairs (device) ----
 * sum over row pairs of popcount(row_i & row_j) for `n_vectors` rows of `n_ints` 64-bit words
 * in a caller-owned HOST buffer (reference storm.h:95-148, storm.c:132-369). The buffer is
 * copied to the device per call. `f` / `fl` must be NULL or leaves exported by this library.
 * The *_list variants return the same exact count as the plain ones (the position lists are
 * a CPU-side shortcut; the device kernel is density independent). */
uint64_t STORM_wrapper_diag(const uint32_t n_vectors, const uint64_t* vals,
                            const uint32_t n_ints, const STORM_compute_func f);
uint64_t STORM_wrapper_diag_blocked(const uint32_t n_vectors, const uint64_t* vals,
                                    const uint32_t n_ints, const STORM_compute_func f,
                                    uint32_t block_size);
/* every row of vals1 against every row of vals2 (storm.c:153-171, intent of storm.h:72-77) */
uint64_t STORM_wrapper_square(const uint32_t n_vectors1, const uint64_t* STORM_RESTRICT vals1,
                              const uint32_t n_vectors2, const uint64_t* STORM_RESTRICT vals2,
                              const uint32_t n_ints, const STORM_compute_func f);
uint64_t STORM_wrapper_diag_list(const uint32_t n_vectors, const uint64_t* STORM_RESTRICT vals,
                                 const uint32_t n_ints, const uint32_t* STORM_RESTRICT n_alts,
                                 const uint32_t* STORM_RESTRICT alt_positions,
                                 const uint32_t* STORM_RESTRICT alt_offsets,
                                 const STORM_compute_func f, const STORM_compute_lfunc fl,
                                 const uint32_t cutoff);
uint64_t STORM_wrapper_diag_list_blocked(const uint32_t n_vectors,
                                         const uint64_t* STORM_RESTRICT vals,
                                         const uint32_t n_ints,
                                         const uint32_t* STORM_RESTRICT n_alts,
                                         const uint32_t* STORM_RESTRICT alt_positions,
                                         const uint32_t* STORM_RESTRICT alt_offsets,
                                         const STORM_compute_func f,
                                         const STORM_compute_lfunc fl, const uint32_t cutoff,
                                         uint32_t block_size);

/* ------------------------------------------------------------------------ containers ---- */
typedef struct STORM_bitmap_s STORM_bitmap_t;
typedef struct STORM_bitmap_cont_s STORM_bitmap_cont_t;
typedef struct STORM_s STORM_t;
typedef struct STORM_contiguous_bitmap_s STORM_contiguous_bitmap_t;
typedef struct STORM_contiguous_s STORM_contiguous_t;

/* one 65536-bit block of one row: a sorted uint16 list OR a 1024-word bitmap
 * (reference storm.h:158-166) */
struct STORM_bitmap_s {
    STORM_ALIGN(64) uint64_t* data;
    STORM_ALIGN(64) uint16_t* scalar;
    uint32_t n_bitmap : 30, own_data : 1, own_scalar : 1;
    uint32_t n_bits_set;
    uint32_t n_scalar : 31, n_scalar_set : 1, n_missing;
    uint32_t m_scalar;
    uint32_t id;
    /* private (in the tail padding: the struct stays 128 bytes): the mutation epoch of the block's last change through
     * the public block / row functions (storm_host.c). The device copies of a STORM_t are matched to it. */
    uint64_t hip_stamp;
};

/* one row: its blocks in ascending id order (reference storm.h:168-173) */
struct STORM_bitmap_cont_s {
    STORM_bitmap_t* bitmaps;
    uint32_t* block_ids;
    uint32_t n_bitmaps, m_bitmaps;
    uint32_t prev_inserted_value;
};

/* sparse container (reference storm.h:175-178) + private device state */
struct STORM_s {
    STORM_bitmap_cont_t* conts;
    uint32_t n_conts, m_conts;
    /* private */
    void* hip_arena;        /* device replicas of the flattened arena, rebuilt when dirty */
    uint32_t hip_dirty;
    uint32_t hip_generation; /* device configuration the arena was built for */
    uint64_t hip_fingerprint; /* rows / blocks / set-bit counts the arena was built from */
    uint32_t hip_private;     /* a container the library keeps for itself (the list mirror of a
                                 STORM_contiguous_t): nobody edits its members, no fingerprint per call */
    uint64_t hip_epoch;       /* the mutation epoch (storm_host.c) the device arena was last verified at */
    void* hip_stage;          /* [r6] the bitmap blocks STORM_add has already sent to the device (storm_host.c) */
};

/* one row of the dense container (reference storm.h:181-186) */
struct STORM_contiguous_bitmap_s {
    uint64_t* data;
    uint32_t* scalar;
    uint32_t n_scalar;
};

/* dense container (reference storm.h:188-200) + private device state */
struct STORM_contiguous_s {
    uint64_t* data;
    uint32_t* scalar;
    uint32_t* n_scalar;
    STORM_contiguous_bitmap_t* bitmaps;
    uint64_t n_data, m_data;
    uint64_t tot_scalar, m_scalar;
    uint64_t vector_length;
    uint32_t n_bitmaps_vector;
    STORM_compute_func intsec_func;
    uint32_t alignment;
    uint32_t scalar_cutoff;
    /* private */
    uint64_t* scalar_offset; /* start of each row's list in `scalar` (per row)     */
    void* hip_matrix;        /* storm_hip_matrix_t*: device mirror of `data`        */
    uint64_t hip_rows_synced;
    uint64_t hip_rows_capacity;
    STORM_t* hip_lists;      /* the same rows as a STORM_t while EVERY row is below scalar_cutoff:   */
    uint32_t hip_lists_off;  /* such a container goes through the list-probe kernel (see storm_host.c) */
    void* hip_pending;       /* positions of rows not yet on the device (STORM_contig_add; storm_host.c)    */
    uint64_t hip_words_below; /* rows below this one were edited in place (STORM_contig_hip_invalidate): sent as words */
};

/* per-block API (reference storm.h:203-212, storm.c:372-380, :398-656) */
STORM_bitmap_t* STORM_bitmap_new();
void STORM_bitmap_init(STORM_bitmap_t* all);
void STORM_bitmap_free(STORM_bitmap_t* bitmap);
int STORM_bitmap_add(STORM_bitmap_t* bitmap, const uint32_t* values, const uint32_t n_values);
int STORM_bitmap_add_with_scalar(STORM_bitmap_t* bitmap, const uint32_t* values,
                                 const uint32_t n_values);
int STORM_bitmap_add_scalar_only(STORM_bitmap_t* bitmap, const uint32_t* values,
                                 const uint32_t n_values);
uint64_t STORM_bitmap_intersect_cardinality(STORM_bitmap_t* STORM_RESTRICT bitmap1,
                                            STORM_bitmap_t* STORM_RESTRICT bitmap2);
uint64_t STORM_bitmap_intersect_cardinality_func(STORM_bitmap_t* STORM_RESTRICT bitmap1,
                                                 STORM_bitmap_t* STORM_RESTRICT bitmap2,
                                                 const STORM_compute_func func);
int STORM_bitmap_clear(STORM_bitmap_t* bitmap);
uint32_t STORM_bitmap_serialized_size(STORM_bitmap_t* bitmap);

/* per-row API (reference storm.h:215-222, storm.c:383-394, :659-824) */
STORM_bitmap_cont_t* STORM_bitmap_cont_new();
void STORM_bitmap_cont_init(STORM_bitmap_cont_t* bitmap);
void STORM_bitmap_cont_free(STORM_bitmap_cont_t* bitmap);
int STORM_bitmap_cont_add(STORM_bitmap_cont_t* bitmap, const uint32_t* values,
                          const uint32_t n_values);
int STORM_bitmap_cont_clear(STORM_bitmap_cont_t* bitmap);
uint64_t STORM_bitmap_cont_intersect_cardinality(
    const STORM_bitmap_cont_t* STORM_RESTRICT bitmap1,
    const STORM_bitmap_cont_t* STORM_RESTRICT bitmap2);
uint64_t STORM_bitmap_cont_intersect_cardinality_premade(
    const STORM_bitmap_cont_t* STORM_RESTRICT bitmap1,
    const STORM_bitmap_cont_t* STORM_RESTRICT bitmap2, const STORM_compute_func func,
    uint32_t* out);
uint32_t STORM_bitmap_cont_serialized_size(STORM_bitmap_cont_t* bitmap);

/* sparse container (reference storm.h:225-232, storm.c:827-973).
 * STORM_add: values sorted ascending; returns 1 (an empty input still appends an empty row).
 * STORM_pairw_*: sum over row pairs i<j of |row_i ∩ row_j|, computed on the GPU;
 * NULL handle or device failure -> (uint64_t)-1. */
STORM_t* STORM_new();
void STORM_free(STORM_t* bitmap);
int STORM_add(STORM_t* bitmap, const uint32_t* values, const uint32_t n_values);
int STORM_clear(STORM_t* bitmap);
uint64_t STORM_pairw_intersect_cardinality(STORM_t* bitmap);
uint64_t STORM_pairw_intersect_cardinality_blocked(STORM_t* bitmap, uint32_t bsize);
uint64_t STORM_serialized_size(const STORM_t* bitmap);
/* Extension: the serialized form whose SIZE the reference defines (STORM_serialized_size,
 * storm.c:372-394, :963-973) but never writes. STORM_serialize writes exactly
 * STORM_serialized_size(h) bytes (layout: storm_host.c) and returns that count, 0 if `capacity`
 * is too small. STORM_deserialize returns NULL on a malformed stream.
 * STORM_serialized_pairw_intersect_cardinality computes the all-pairs total of a serialized
 * container without building it on the host: the bytes are uploaded as they are and unpacked into
 * the block arena by the device (`buf` 2-byte aligned; (uint64_t)-1 on failure). */
uint64_t STORM_serialize(const STORM_t* bitmap, void* buf, uint64_t capacity);
STORM_t* STORM_deserialize(const void* buf, uint64_t n_bytes);
uint64_t STORM_serialized_pairw_intersect_cardinality(const void* buf, uint64_t n_bytes);
/* Reference storm.h:231 declares this and never defines it (storm.c:975). Here: the sum over every row i of bitmap1 and
 * every row j of bitmap2 of STORM_bitmap_cont_intersect_cardinality(&bitmap1->conts[i], &bitmap2->conts[j]) — the whole
 * rectangle, both orders, no triangle — computed on the GPU. 0 when either container is empty; (uint64_t)-1 for a NULL
 * handle or a device failure (STORM_hip_error says why). bitmap1 == bitmap2 is allowed: 2 x the all-pairs total plus each
 * row's count with itself. `const` is the containers': the device copies kept behind the handles may be (re)built.
 * One device slot and one process only (STORM_hip_set_devices / _set_thread_devices with several slots, or
 * STORM_hip_set_shard with more than one shard: refused, on every rank alike). */
uint64_t STORM_intersect_cardinality_square(const STORM_t* STORM_RESTRICT bitmap1, const STORM_t* STORM_RESTRICT bitmap2);

/* dense container (reference storm.h:235-242, storm.c:1001-1346).
 * STORM_contig_add: returns n_values; 0 for an empty input (no row appended); -1 / -2 for a
 * NULL handle / NULL values.
 * STORM_contig_pairw_*: GPU; NULL handle or device failure -> (uint64_t)-1; the *_list
 * variants return (uint64_t)-2 / -3 before the first add, like the reference. */
STORM_contiguous_t* STORM_contig_new(size_t vector_length);
void STORM_contig_free(STORM_contiguous_t* bitmap);
int STORM_contig_add(STORM_contiguous_t* bitmap, const uint32_t* values,
                     const uint32_t n_values);
int STORM_contig_clear(STORM_contiguous_t* bitmap);
uint64_t STORM_contig_pairw_intersect_cardinality(STORM_contiguous_t* bitmap);
uint64_t STORM_contig_pairw_intersect_cardinality_blocked(STORM_contiguous_t* bitmap,
                                                          uint32_t bsize);
uint64_t STORM_contig_pairw_intersect_cardinality_list(STORM_contiguous_t* bitmap);
uint64_t STORM_contig_pairw_intersect_cardinality_blocked_list(STORM_contiguous_t* bitmap,
                                                               uint32_t bsize);

/* Extension: the per-pair matrix the reference only sums (README.md:41). op: 0 = intersect,
 * 1 = union, 2 = symmetric difference. `out` holds out_rows x out_ld uint32, row-major; entry
 * (i, j) = popcount(row_i OP row_j) for i < j < n_data at out[i * out_ld + j], 0 for i >= j.
 * Returns 0; -1 NULL handle, -2 NULL out, -3 device failure (see STORM_hip_error), -4 when
 * out_rows or out_ld is smaller than the number of rows the handle holds (nothing is written).
 * STORM_contig_n_rows: rows appended so far (empty inputs append none, storm.c:1034). */
uint64_t STORM_contig_n_rows(const STORM_contiguous_t* bitmap);
int STORM_contig_pairw_matrix(STORM_contiguous_t* bitmap, int op, uint32_t* out, uint64_t out_rows,
                              uint64_t out_ld);
/* The same for a STORM_t: entry (i, j), i < j, is what STORM_bitmap_cont_intersect_cardinality(&conts[i], &conts[j])
 * returns (storm.c:790-814; the LD use case of README.md:165-167 on the sparse container), or the union / symmetric
 * difference count for op 1 / 2. The device keeps the rows as a dense bit matrix for this (65536 x (largest block
 * id + 1) bits per row; rows beyond 2^25 bits are refused with -3). Same return codes; STORM_n_rows: rows added. */
uint64_t STORM_n_rows(const STORM_t* bitmap);
int STORM_pairw_matrix(STORM_t* bitmap, int op, uint32_t* out, uint64_t out_rows, uint64_t out_ld);
/* Both with the output left in DEVICE memory: `d_out` is a device pointer (hipMalloc) to out_rows x out_ld uint32 on the one
 * device slot the calling thread drives (-5 when its view spans several: STORM_hip_set_thread_devices). Entries i >= j of
 * the n x n window are written as 0 only inside the tiles the kernel touches: clear the buffer once if they matter. The
 * 4 n^2 bytes then never cross the bus (half of a STORM_pairw_matrix call at n = 10000). Same return codes otherwise. */
int STORM_pairw_matrix_device(STORM_t* bitmap, int op, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld);
/* The rectangle of two STORM_t: entry (i, j) = popcount(A_i OP B_j) for EVERY row i of `a` and j of `b` at
 * out[i * out_ld + j] (op 0 / 1 / 2 as above; STORM_bitmap_cont_intersect_cardinality(&a->conts[i], &b->conts[j]) for
 * op 0). Every entry of the N_A x N_B window is written. a == b is allowed (the full symmetric matrix, the rows' own
 * counts on the diagonal). Same return codes as STORM_pairw_matrix, with -4 when out_rows < N_A or out_ld < N_B;
 * _device: `d_out` in device memory, -5 as for STORM_pairw_matrix_device. Two list-only containers that are sparse
 * enough (option matrix_lists, as for STORM_pairw_matrix) are joined from their lists; otherwise both go to dense
 * replicas of one common width (the wider of the two: a handle may keep its widened replica; the 2^25-bit row limit
 * applies). One device slot and one process, as STORM_intersect_cardinality_square. */
int STORM_square_matrix(STORM_t* a, STORM_t* b, int op, uint32_t* out, uint64_t out_rows, uint64_t out_ld);
int STORM_square_matrix_device(STORM_t* a, STORM_t* b, int op, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld);
int STORM_contig_pairw_matrix_device(STORM_contiguous_t* bitmap, int op, uint32_t* d_out, uint64_t out_rows,
                                     uint64_t out_ld);

/* Extension: the per-pair matrices above finished into the statistic they are computed for (README.md:165-167: linkage
 * disequilibrium, "any intersect-count problem") — on the device, where the counts lie, instead of 4 n^2 bytes over the bus
 * and n^2 divisions on the host. With c = the pair's intersect count (storm.c:790-814 / :1149-1173 per pair), a and b the
 * two rows' set-bit counts and M = n_bits, the size of the universe (for LD: the number of haplotypes):
 *   STORM_SIM_JACCARD  c / (a + b - c)                         NaN when both rows are empty
 *   STORM_SIM_COSINE   c / sqrt(a b)   (Ochiai)                NaN when either row is empty
 *   STORM_SIM_LD_D     (M c - a b) / M^2                       always defined
 *   STORM_SIM_LD_R2    (M c - a b)^2 / (a (M - a) b (M - b))   NaN unless 0 < a < M and 0 < b < M
 * as float: M c - a b exactly in integers, the rest in double, rounded once (at most one float from the exactly rounded
 * value); NaN is always the bit pattern 0x7FC00000. `out` holds out_rows x out_ld float, row-major, entry (i, j) at
 * out[i * out_ld + j].
 *   STORM_contig_pairw_similarity / STORM_pairw_similarity: entries i < j < n; 0.0f for i >= j (_device: entries i >= j stay
 *     as the count kernel left them, see STORM_pairw_matrix_device). The kernels and their choice are those of
 *     STORM_contig_pairw_matrix / STORM_pairw_matrix with op 0.
 *   STORM_square_similarity: every entry of the N_A x N_B window, as STORM_square_matrix; a == b is allowed (the diagonal is
 *     a row with itself: Jaccard = cosine = 1, NaN for an empty row).
 * n_bits: not read by Jaccard and cosine. STORM_contiguous_t: 0 = the container's vector_length (storm.h:188-200). A STORM_t
 * declares no universe: the LD measures need n_bits > 0. At most 2^32.
 * Returns 0; -1 NULL handle, -2 NULL out, -4 out_rows or out_ld smaller than the rows held (nothing is written), -3 device
 * failure, unknown measure or bad n_bits (STORM_hip_error says which), -5 when the calling thread's view spans several
 * device slots — host forms too: like the rectangle, these run on one device slot and one process. Empty containers: 0,
 * nothing written. _device: `d_out` in device memory on that slot. */
#define STORM_SIM_JACCARD 0
#define STORM_SIM_COSINE 1
#define STORM_SIM_LD_D 2
#define STORM_SIM_LD_R2 3
int STORM_contig_pairw_similarity(STORM_contiguous_t* bitmap, int measure, uint64_t n_bits, float* out, uint64_t out_rows,
                                  uint64_t out_ld);
int STORM_contig_pairw_similarity_device(STORM_contiguous_t* bitmap, int measure, uint64_t n_bits, float* d_out,
                                         uint64_t out_rows, uint64_t out_ld);
int STORM_pairw_similarity(STORM_t* bitmap, int measure, uint64_t n_bits, float* out, uint64_t out_rows, uint64_t out_ld);
int STORM_pairw_similarity_device(STORM_t* bitmap, int measure, uint64_t n_bits, float* d_out, uint64_t out_rows,
                                  uint64_t out_ld);
int STORM_square_similarity(STORM_t* a, STORM_t* b, int measure, uint64_t n_bits, float* out, uint64_t out_rows,
                            uint64_t out_ld);
int STORM_square_similarity_device(STORM_t* a, STORM_t* b, int measure, uint64_t n_bits, float* d_out, uint64_t out_rows,
                                   uint64_t out_ld);

/* Extension: the per-pair matrices for the pairs within max_lag rows of each other only — what LD pruning, clumping, r^2 decay
 * and banded LD matrices ask for: row i against the next w rows in container order, not all-vs-all. With n the rows held
 * and L = min(max_lag, n - 1), `out` holds out_rows x out_ld entries (out_rows >= n, out_ld >= L) and the pair (i, j),
 * 1 <= j - i <= L, lies at out[i * out_ld + (j - i - 1)]: n x L entries instead of n x n, and only the tiles within L rows
 * of the diagonal are multiplied. Host forms write columns [0, L) of every row (0 / 0.0f where i + 1 + d >= n); _device forms
 * (`d_out` in device memory) leave everything outside the layout untouched. Counts under `op` (0 and, 1 or, 2 xor) as uint32,
 * or the measures of STORM_*_pairw_similarity as float (same n_bits rule, bit-identical to the same pairs of those calls).
 * A STORM_t always runs on its dense replica here (there is no list-join form). One device slot and one process.
 * Returns 0; -1 NULL handle, -2 NULL out, -4 out_rows < n or out_ld < L (nothing is written), -3 device failure, bad op,
 * measure or n_bits, or max_lag 0 (STORM_hip_error says which), -5 several device slots in view. Fewer than two rows: 0,
 * nothing written. */
int STORM_contig_pairw_lag_matrix(STORM_contiguous_t* bitmap, int op, uint64_t max_lag, uint32_t* out, uint64_t out_rows,
                                  uint64_t out_ld);
int STORM_contig_pairw_lag_matrix_device(STORM_contiguous_t* bitmap, int op, uint64_t max_lag, uint32_t* d_out,
                                         uint64_t out_rows, uint64_t out_ld);
int STORM_contig_pairw_lag_similarity(STORM_contiguous_t* bitmap, int measure, uint64_t n_bits, uint64_t max_lag, float* out,
                                      uint64_t out_rows, uint64_t out_ld);
int STORM_contig_pairw_lag_similarity_device(STORM_contiguous_t* bitmap, int measure, uint64_t n_bits, uint64_t max_lag,
                                             float* d_out, uint64_t out_rows, uint64_t out_ld);
int STORM_pairw_lag_matrix(STORM_t* bitmap, int op, uint64_t max_lag, uint32_t* out, uint64_t out_rows, uint64_t out_ld);
int STORM_pairw_lag_matrix_device(STORM_t* bitmap, int op, uint64_t max_lag, uint32_t* d_out, uint64_t out_rows,
                                  uint64_t out_ld);
int STORM_pairw_lag_similarity(STORM_t* bitmap, int measure, uint64_t n_bits, uint64_t max_lag, float* out, uint64_t out_rows,
                               uint64_t out_ld);
int STORM_pairw_lag_similarity_device(STORM_t* bitmap, int measure, uint64_t n_bits, uint64_t max_lag, float* d_out,
                                      uint64_t out_rows, uint64_t out_ld);

/* Extension: for each row its k most similar rows, selected on the device (k-NN graphs on Jaccard or cosine, the best LD
 * tags of a variant, the nearest sets of a query container in a reference container): n x k entries instead of n x n.
 * `score` is one of the measures of STORM_*_pairw_similarity (same n_bits rule, values bit-identical to those calls) or
 * STORM_TOPK_COUNT, the AND count itself. idx[i * out_ld + t] is the row (of `b` for STORM_square_topk) that ranks t-th for
 * row i, val[i * out_ld + t] its value (float bits, or the count as uint32): value descending, then row index ascending. A
 * row never lists itself (pairw forms), and never a row its value is undefined (NaN) against. Fewer than k candidates: the
 * rest of columns [0, k) is padding, idx 0xFFFFFFFF with val NaN (0x7FC00000), or val 0 under STORM_TOPK_COUNT. Columns
 * [k, out_ld) are not touched. 1 <= k <= STORM_TOPK_MAX; out_rows >= n and out_ld >= k. panel_rows: rows whose counts are
 * on the device at a time, 0 (chosen by the library) or a multiple of 256. _device forms: idx / val in device memory.
 * A STORM_t always runs on its dense replica here, two of them at their common width (there is no list-join form). One
 * device slot and one process. Returns 0; -1 NULL handle, -2 NULL idx or val, -4 out_rows < n or out_ld < k (nothing is
 * written), -3 device failure, bad score, n_bits, k or panel_rows (STORM_hip_error says which), -5 several device slots in
 * view. No rows: 0, nothing written. */
#define STORM_TOPK_COUNT 4
#define STORM_TOPK_MAX 128
int STORM_contig_pairw_topk(STORM_contiguous_t* bitmap, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows,
                            uint32_t* idx, void* val, uint64_t out_rows, uint64_t out_ld);
int STORM_contig_pairw_topk_device(STORM_contiguous_t* bitmap, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows,
                                   uint32_t* d_idx, void* d_val, uint64_t out_rows, uint64_t out_ld);
int STORM_pairw_topk(STORM_t* bitmap, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* idx, void* val,
                     uint64_t out_rows, uint64_t out_ld);
int STORM_pairw_topk_device(STORM_t* bitmap, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* d_idx,
                            void* d_val, uint64_t out_rows, uint64_t out_ld);
int STORM_square_topk(STORM_t* a, STORM_t* b, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows, uint32_t* idx,
                      void* val, uint64_t out_rows, uint64_t out_ld);
int STORM_square_topk_device(STORM_t* a, STORM_t* b, int score, uint64_t n_bits, uint64_t k, uint64_t panel_rows,
                             uint32_t* d_idx, void* d_val, uint64_t out_rows, uint64_t out_ld);

/* Extension: rows of 2-bit DOSAGES instead of bits — unphased genotypes, 0 / 1 / 2 copies of an allele per sample — and
 * the LD asked of them: PLINK's --r / --r2, the (squared) Pearson correlation of two dosage vectors. A row is n_samples
 * values in 0 .. 3, packed 2 bits each: sample s in bits 2 (s % 32) and 2 (s % 32) + 1 of 64-bit word s / 32, as an
 * unsigned integer; ceil(n_samples / 32) words per row, tail bits zero. 3 is an ordinary value (the arithmetic is linear
 * up to 3) in every call but the three "missing genotypes" calls below, which read it as STORM_DOSAGE_MISSING. On the device one FP4 multiply does the work (the E2M1 codes 0 .. 3 are 0, 0.5, 1, 1.5: linear
 * in the value), so a sample pair costs what a bit pair costs the other containers; every result is exact.
 *   STORM_dosage_new(n_samples)        1 <= n_samples <= 2^24, else NULL
 *   STORM_dosage_add(h, values, n)     one row, one byte per sample; n must be n_samples and every value <= 3
 *   STORM_dosage_add_packed(h, w, r)   r rows already packed, ceil(n_samples / 32) words each; tail bits must be zero
 *   STORM_dosage_row_sums              sum[i] = sum_s v, sum_sq[i] = sum_s v^2 of every row, computed on the device
 *   STORM_dosage_pairw_dot             out[i * out_ld + j] = P(i, j) = sum_s v_i[s] v_j[s] for i < j < n (uint32, exact)
 *   STORM_dosage_pairw_corr            with S = n_samples, s = sum v, q = sum v^2: num = S P - s_i s_j, d = S q - s^2, exactly in
 *                                      64-bit integers; STORM_DOSAGE_R2: num^2 / (d_i d_j), STORM_DOSAGE_R: num / sqrt(d_i d_j);
 *                                      the division in double, rounded once to float (at most one float from the exactly
 *                                      rounded value); NaN (0x7FC00000) when d_i or d_j is 0: a constant row
 * Output conventions of STORM_contig_pairw_matrix[_device] and STORM_*_similarity: out_rows >= n and out_ld >= n; host forms
 * write 0 / +0.0f at i >= j inside the n x n window; _device forms (`d_out` in device memory) leave i >= j as they were;
 * nothing outside the n x n window is touched. The host keeps the packed rows and uploads them on the first call after a
 * change (no streaming at add time). One device slot and one process.
 * Returns 0; -1 NULL handle, -2 NULL values / words / out, -4 out_rows < n or out_ld < n (nothing is written), -3 device
 * failure or a bad argument — a value above 3, n != n_samples, non-zero tail bits (nothing is appended), an unknown
 * measure — STORM_hip_error says which; -5 several device slots in view. Fewer than two rows: 0, nothing written. There
 * is no CPU fallback: without a device the compute calls return -3. */
typedef struct STORM_dosage_s STORM_dosage_t;
#define STORM_DOSAGE_R2 0
#define STORM_DOSAGE_R 1
STORM_dosage_t* STORM_dosage_new(uint64_t n_samples);
void STORM_dosage_free(STORM_dosage_t* h);
int STORM_dosage_add(STORM_dosage_t* h, const uint8_t* values, uint64_t n_values);
int STORM_dosage_add_packed(STORM_dosage_t* h, const uint64_t* words, uint64_t n_rows);
int STORM_dosage_clear(STORM_dosage_t* h);
uint64_t STORM_dosage_n_rows(const STORM_dosage_t* h);
int STORM_dosage_row_sums(STORM_dosage_t* h, uint32_t* sum, uint32_t* sum_sq);
int STORM_dosage_pairw_dot(STORM_dosage_t* h, uint32_t* out, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_pairw_dot_device(STORM_dosage_t* h, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_pairw_corr(STORM_dosage_t* h, int measure, float* out, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_pairw_corr_device(STORM_dosage_t* h, int measure, float* d_out, uint64_t out_rows, uint64_t out_ld);

/* The rectangle of two dosage containers, and rows with MISSING genotypes (PLINK's .bed spends one of its four codes on
 * them): pairwise-complete statistics, over the samples that BOTH rows of a pair have.
 *   STORM_dosage_square_dot            out[i * out_ld + j] = sum_s a_i[s] b_j[s] for EVERY row i of a and j of b (uint32,
 *                                      exact; 3 is an ordinary value); out_rows >= a's rows, out_ld >= b's rows; both
 *                                      containers must hold the same number of samples (-3 otherwise); an empty one: 0,
 *                                      nothing written
 * In the calls below, and only there, the value 3 (STORM_DOSAGE_MISSING) means "no call for this sample":
 *   STORM_dosage_row_missing           missing[i] = the samples of row i that are missing
 *   STORM_dosage_pairw_nobs            out[i * out_ld + j] = N(i, j), the samples both rows have, for i < j < n (uint32)
 *   STORM_dosage_pairw_corr_complete   with g = the value (0 where missing) and m = 1 where present: P = sum g_i g_j,
 *                                      Sx = sum g_i m_j, Sy = sum m_i g_j, Qx = sum g_i^2 m_j, Qy = sum m_i g_j^2;
 *                                      num = N P - Sx Sy, dx = N Qx - Sx^2, dy = N Qy - Sy^2 exactly in 64-bit integers;
 *                                      STORM_DOSAGE_R2: num^2 / (dx dy), STORM_DOSAGE_R: num / sqrt(dx dy), in double, rounded
 *                                      once to float; NaN (0x7FC00000) exactly when dx or dy is 0: no or one shared sample,
 *                                      or a row constant on the shared samples. On rows without a 3: the same bits as
 *                                      STORM_dosage_pairw_corr. Device scratch: about 3 n^2 uint32 and three copies of the
 *                                      rows, kept by the device context
 * Output conventions, argument checks and return codes as STORM_dosage_pairw_dot / STORM_dosage_pairw_corr above. */
#define STORM_DOSAGE_MISSING 3
int STORM_dosage_square_dot(STORM_dosage_t* a, STORM_dosage_t* b, uint32_t* out, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_square_dot_device(STORM_dosage_t* a, STORM_dosage_t* b, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_row_missing(STORM_dosage_t* h, uint32_t* missing);
int STORM_dosage_pairw_nobs(STORM_dosage_t* h, uint32_t* out, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_pairw_nobs_device(STORM_dosage_t* h, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_pairw_corr_complete(STORM_dosage_t* h, int measure, float* out, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_pairw_corr_complete_device(STORM_dosage_t* h, int measure, float* d_out, uint64_t out_rows, uint64_t out_ld);

/* r / r^2 between TWO dosage containers: every row i of a against every row j of b at out[i * out_ld + j] — a list of index
 * variants against a panel (PLINK's --r2 --ld-snp-list ... inter-chr), one chromosome against another, a new batch
 * against what is loaded — for 6 n_a n_b row-pair products where the triangle of the stacked container costs 3 (n_a + n_b)^2.
 *   STORM_dosage_square_corr            STORM_dosage_pairw_corr's formula with P = sum_s a_i[s] b_j[s] and s, q of each row
 *                                       taken in its own container (S = n_samples; 3 is an ordinary value); NaN
 *                                       (0x7FC00000) when either row is constant
 *   STORM_dosage_square_nobs            N(i, j): the samples that neither a_i nor b_j has as 3 (STORM_DOSAGE_MISSING) (uint32)
 *   STORM_dosage_square_corr_complete   STORM_dosage_pairw_corr_complete's formula over the samples both rows have; on rows
 *                                       without a 3 the same bits as STORM_dosage_square_corr. Device scratch: about
 *                                       5 n_a n_b uint32 and three copies of the rows of each container, kept by the
 *                                       device context (nothing bounds it by panels of b: cut b into several containers)
 * Each float is bit-identical to the pairw call's for the same two rows in one container. Output conventions, argument
 * checks and return codes are STORM_dosage_square_dot's: every entry (i, j), i < a's rows, j < b's rows, is written by the
 * host and the _device forms alike and nothing outside that window is touched; out_rows >= a's rows and out_ld >= b's rows
 * (-4 otherwise, nothing written); unequal sample counts or an unknown measure: -3, STORM_hip_error says which; an empty
 * container: 0, nothing written; a may be b; -1 NULL handle, -2 NULL out, -5 several device slots in view. */
int STORM_dosage_square_corr(STORM_dosage_t* a, STORM_dosage_t* b, int measure, float* out, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_square_corr_device(STORM_dosage_t* a, STORM_dosage_t* b, int measure, float* d_out, uint64_t out_rows,
                                    uint64_t out_ld);
int STORM_dosage_square_nobs(STORM_dosage_t* a, STORM_dosage_t* b, uint32_t* out, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_square_nobs_device(STORM_dosage_t* a, STORM_dosage_t* b, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_square_corr_complete(STORM_dosage_t* a, STORM_dosage_t* b, int measure, float* out, uint64_t out_rows,
                                      uint64_t out_ld);
int STORM_dosage_square_corr_complete_device(STORM_dosage_t* a, STORM_dosage_t* b, int measure, float* d_out, uint64_t out_rows,
                                             uint64_t out_ld);

/* The best LD tags of a variant for UNPHASED genotypes: for each row of a dosage container its k best rows, selected on the
 * device — n x k indices and values leave it instead of the n x n float matrix of STORM_dosage_pairw_corr /
 * _square_corr[_complete] (4 GiB at 32768 variants), and the device scratch is one row panel of integer sums: O(panel_rows x
 * n_b) words, about 6 times that in the _complete forms, never O(n_a x n_b).
 *   STORM_dosage_pairw_topk[_complete]    row i of h against every OTHER row of h (a row never lists itself)
 *   STORM_dosage_square_topk[_complete]   row i of a against every row of b (the same number of samples; a may be b, and a
 *                                         row lists itself then)
 * `score`: STORM_DOSAGE_R2, STORM_DOSAGE_R — ranked by the SIGNED value; ranking by |r| is what STORM_DOSAGE_R2 gives — or
 * STORM_DOSAGE_TOPK_DOT, the dot product P itself (val is uint32 then; valid in these calls only and in the plain forms only:
 * the _complete forms refuse it with -3). The value bits are exactly what STORM_dosage_square_corr writes for the two rows
 * (bit-identical to STORM_dosage_pairw_corr; 3 is an ordinary value), in the _complete forms exactly what
 * STORM_dosage_square_corr_complete writes (3 = STORM_DOSAGE_MISSING).
 * Order, padding and limits are STORM_pairw_topk's: idx[i * out_ld + t] is the row that ranks t-th for row i, val[i * out_ld
 * + t] its value; value descending, then row index ascending; a NaN entry (0x7FC00000: a constant row, no shared samples)
 * is never a candidate; a row with fewer than k candidates is padded with idx 0xFFFFFFFF and val NaN (val 0 under
 * STORM_DOSAGE_TOPK_DOT); columns [k, out_ld) and everything outside the n_a x k window are not touched. 1 <= k <=
 * STORM_TOPK_MAX; out_rows >= a's rows and out_ld >= k. panel_rows: rows of a whose sums are on the device at a time, 0
 * (chosen by the library: at most 256 MiB of them, at least 256 rows) or a multiple of 256. The _device forms take idx /
 * val in DEVICE memory and are complete on return. The _complete forms hold at most 65408 rows per container.
 * Returns 0; -1 NULL handle; -2 NULL idx or val; -4 out_rows or out_ld too small (nothing written); -3 a bad score, k or
 * panel_rows, unequal sample counts, or a device failure (STORM_hip_error says which); -5 several device slots in view. An
 * empty a: 0, nothing written. An empty b, or pairw on one row: every row is k paddings. */
#define STORM_DOSAGE_TOPK_DOT 2
int STORM_dosage_pairw_topk(STORM_dosage_t* h, int score, uint64_t k, uint64_t panel_rows, uint32_t* idx, void* val,
                            uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_pairw_topk_device(STORM_dosage_t* h, int score, uint64_t k, uint64_t panel_rows, uint32_t* d_idx, void* d_val,
                                   uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_pairw_topk_complete(STORM_dosage_t* h, int score, uint64_t k, uint64_t panel_rows, uint32_t* idx, void* val,
                                     uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_pairw_topk_complete_device(STORM_dosage_t* h, int score, uint64_t k, uint64_t panel_rows, uint32_t* d_idx,
                                            void* d_val, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_square_topk(STORM_dosage_t* a, STORM_dosage_t* b, int score, uint64_t k, uint64_t panel_rows, uint32_t* idx,
                             void* val, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_square_topk_device(STORM_dosage_t* a, STORM_dosage_t* b, int score, uint64_t k, uint64_t panel_rows,
                                    uint32_t* d_idx, void* d_val, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_square_topk_complete(STORM_dosage_t* a, STORM_dosage_t* b, int score, uint64_t k, uint64_t panel_rows,
                                      uint32_t* idx, void* val, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_square_topk_complete_device(STORM_dosage_t* a, STORM_dosage_t* b, int score, uint64_t k, uint64_t panel_rows,
                                             uint32_t* d_idx, void* d_val, uint64_t out_rows, uint64_t out_ld);

/* The four pairwise calls of the dosage container for the pairs within max_lag rows of each other only — PLINK's --r / --r2
 * as it is run on genotype files: within a window (--ld-window), never all-vs-all. The layout is STORM_pairw_lag_matrix's:
 * with n the rows held and L = min(max_lag, n - 1), `out` holds out_rows x out_ld entries (out_rows >= n, out_ld >= L) and
 * the pair (i, j), 1 <= j - i <= L, lies at out[i * out_ld + (j - i - 1)]. Memory and work are O(n L): only the tiles within
 * L rows of the diagonal are multiplied, and no buffer of any of the calls grows with n^2.
 *   STORM_dosage_pairw_lag_dot             P(i, j) (uint32, exact; 3 is an ordinary value)
 *   STORM_dosage_pairw_lag_corr            STORM_dosage_pairw_corr's float at the pair: the same bits
 *   STORM_dosage_pairw_lag_nobs            N(i, j), 3 = STORM_DOSAGE_MISSING
 *   STORM_dosage_pairw_lag_corr_complete   STORM_dosage_pairw_corr_complete's float at the pair: the same bits (and, on rows
 *                                          without a 3, STORM_dosage_pairw_lag_corr's). Device scratch: 3 n x (3 L + 2)
 *                                          uint32 and three copies of the rows, kept by the device context
 * Host forms write columns [0, L) of every row (0 / +0.0f where i + 1 + d >= n); _device forms (`d_out` in device memory)
 * leave everything outside the layout untouched. One device slot and one process.
 * Returns 0; -1 NULL handle, -2 NULL out, -4 out_rows < n or out_ld < L (nothing is written), -3 device failure, an unknown
 * measure or max_lag 0 (STORM_hip_error says which), -5 several device slots in view. Fewer than two rows: 0, nothing
 * written. */
int STORM_dosage_pairw_lag_dot(STORM_dosage_t* h, uint64_t max_lag, uint32_t* out, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_pairw_lag_dot_device(STORM_dosage_t* h, uint64_t max_lag, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_pairw_lag_corr(STORM_dosage_t* h, int measure, uint64_t max_lag, float* out, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_pairw_lag_corr_device(STORM_dosage_t* h, int measure, uint64_t max_lag, float* d_out, uint64_t out_rows,
                                       uint64_t out_ld);
int STORM_dosage_pairw_lag_nobs(STORM_dosage_t* h, uint64_t max_lag, uint32_t* out, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_pairw_lag_nobs_device(STORM_dosage_t* h, uint64_t max_lag, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld);
int STORM_dosage_pairw_lag_corr_complete(STORM_dosage_t* h, int measure, uint64_t max_lag, float* out, uint64_t out_rows,
                                         uint64_t out_ld);
int STORM_dosage_pairw_lag_corr_complete_device(STORM_dosage_t* h, int measure, uint64_t max_lag, float* d_out, uint64_t out_rows,
                                                uint64_t out_ld);

/* Per-variant LD scores — the input of LD-score regression — from the rows within max_lag on BOTH sides of every row, reduced
 * on the device: n floats leave it instead of the n x L matrix of STORM_dosage_pairw_lag_corr. With n the rows held and
 * L = min(max_lag, n - 1), row i's neighbours are the rows j with 1 <= |i - j| <= L. For a pair (i, j) let rho be the FLOAT
 * that STORM_dosage_pairw_lag_corr writes for it under STORM_DOSAGE_R2 (the _complete calls: the float of
 * STORM_dosage_pairw_lag_corr_complete, 3 = STORM_DOSAGE_MISSING), widened to double. The pair's term t is
 *   STORM_LDSCORE_R2      t = rho
 *   STORM_LDSCORE_R2_ADJ  t = rho - (1 - rho) / (N - 2) in double, the small-sample correction of LDSC; N is the container's
 *                         n_samples, and in the _complete calls N(i, j), the samples both rows have (what
 *                         STORM_dosage_pairw_lag_nobs returns)
 * and a pair is NOT summed when rho is NaN (a constant row; _complete: no variance on the shared samples) or when stat is
 * _ADJ and N < 3. Then
 *   score[i]   = the sum of the terms of row i's summed pairs, accumulated in double, rounded once to float; +0.0f when no
 *                pair is summed. The variant itself is not included: LDSC's l_i is 1 + score[i].
 *   n_pairs[i] = the number of pairs summed (n_pairs may be NULL).
 * Exactly elements [0, n) of either output are written (out_len >= n is the length of both), in host memory or, for the
 * _device forms, in device memory (complete on return); nothing behind n is touched. Two calls on unchanged rows return identical bits: the
 * additions have one fixed order, no floating-point atomics. Device scratch: the n x L floats of r^2 and the scratch of
 * the corr call beneath. No CPU fallback. One device slot and one process.
 * Returns 0; -1 NULL handle, -2 NULL score, -3 max_lag 0 (said before the size check, even on an empty container), -4
 * out_len < n (nothing is written), -3 an unknown stat (before any device is asked for), _ADJ with n_samples < 3, or a
 * device failure (STORM_hip_error says which), -5 several device slots in view. Fewer than two rows: 0, nothing written. */
#define STORM_LDSCORE_R2 0
#define STORM_LDSCORE_R2_ADJ 1
int STORM_dosage_lag_ldscore(STORM_dosage_t* h, int stat, uint64_t max_lag, float* score, uint32_t* n_pairs, uint64_t out_len);
int STORM_dosage_lag_ldscore_device(STORM_dosage_t* h, int stat, uint64_t max_lag, float* d_score, uint32_t* d_n_pairs,
                                    uint64_t out_len);
int STORM_dosage_lag_ldscore_complete(STORM_dosage_t* h, int stat, uint64_t max_lag, float* score, uint32_t* n_pairs,
                                      uint64_t out_len);
int STORM_dosage_lag_ldscore_complete_device(STORM_dosage_t* h, int stat, uint64_t max_lag, float* d_score, uint32_t* d_n_pairs,
                                             uint64_t out_len);

/* Stratified LD scores in a distance window — what `ldsc --l2 --ld-wind-cm / --ld-wind-kb --annot` computes — reduced on the
 * device: n x n_annot floats leave it instead of the n x L matrix. With the terms t(i, j), the rule which pairs are summed
 * and the statistics of STORM_dosage_lag_ldscore above,
 *   score[i * score_ld + c] = the sum over row i's window W(i) of t(i, j) * annot[j * annot_ld + c], accumulated in double
 *                             (the products are not rounded on their own), rounded once to float; +0.0f when no pair of the
 *                             window is summed.
 *   n_pairs[i]              = the number of pairs summed for row i (one number per row; n_pairs may be NULL).
 * The variant itself is not summed (its r^2 is 1): LDSC's l(i, c) is annot[i][c] + score[i][c].
 * The window W(i):
 *   pos == NULL               the rows j with 1 <= |i - j| <= min(max_lag, n - 1); max_dist is ignored.
 *   pos given (n doubles, HOST memory in every form, not decreasing; equal positions are allowed)
 *                             the rows j != i with |pos[j] - pos[i]| <= max_dist (max_dist >= 0; +inf: every row). The band
 *                             is computed at the lag the windows need, max_i max(i - lo[i], hi[i] - i)
 *                             (STORM_ldscore_window_lag), when max_lag is 0; with max_lag > 0 the call REFUSES when the
 *                             windows need more than max_lag rows — it never clips a window silently — and otherwise
 *                             computes the band at max_lag.
 *   Positions are per chromosome: make one call per chromosome, or offset the chromosomes by more than max_dist.
 * annot: n rows of n_annot floats (1 .. STORM_LDSCORE_MAX_ANNOT), pitch annot_ld >= n_annot; score: out_rows >= n rows of
 * pitch score_ld >= n_annot; columns [n_annot, score_ld) are not touched, columns [n_annot, annot_ld) not read. The host
 * forms refuse an annotation that is not finite, naming the first (row, column); in the _device forms annot, score and
 * n_pairs are DEVICE memory (complete on return) and finite annotations are the caller's obligation (a NaN or an infinity
 * spreads over its column's window). A column has the same bits whatever other columns are passed with it, and two calls on
 * unchanged rows return identical bits. Device work and scratch are O(n L (1 + n_annot / 64)) and O(n (L + n_annot)). No
 * CPU fallback. One device slot and one process.
 * Returns 0; -1 NULL handle, -2 NULL score or annot, -3 max_lag 0 without positions (said before the size check), -4
 * out_rows < n (nothing is written), -3 an unknown stat, _ADJ with n_samples < 3, n_annot outside its range, -4 annot_ld or
 * score_ld < n_annot, -3 a negative or NaN max_dist, a position that is not finite or decreases, windows that need more
 * than max_lag (the message names both numbers), an annotation that is not finite (host forms), or a device failure
 * (STORM_hip_error says which), -5 several device slots in view. Nothing is written on a refusal. Fewer than two rows: 0,
 * nothing written.
 * STORM_ldscore_window_lag: the lag the windows of `pos` (n doubles) need under max_dist, for sizing buffers before the
 * call; host only. 0; -2 NULL argument; -3 the refusals of the positions and max_dist above. */
#define STORM_LDSCORE_MAX_ANNOT 1024
int STORM_ldscore_window_lag(const double* pos, uint64_t n, double max_dist, uint64_t* lag);
int STORM_dosage_lag_ldscore_annot(STORM_dosage_t* h, int stat, uint64_t max_lag, const double* pos, double max_dist,
                                   const float* annot, uint64_t n_annot, uint64_t annot_ld, float* score, uint64_t score_ld,
                                   uint32_t* n_pairs, uint64_t out_rows);
int STORM_dosage_lag_ldscore_annot_device(STORM_dosage_t* h, int stat, uint64_t max_lag, const double* pos, double max_dist,
                                          const float* d_annot, uint64_t n_annot, uint64_t annot_ld, float* d_score,
                                          uint64_t score_ld, uint32_t* d_n_pairs, uint64_t out_rows);
int STORM_dosage_lag_ldscore_annot_complete(STORM_dosage_t* h, int stat, uint64_t max_lag, const double* pos, double max_dist,
                                            const float* annot, uint64_t n_annot, uint64_t annot_ld, float* score, uint64_t score_ld,
                                            uint32_t* n_pairs, uint64_t out_rows);
int STORM_dosage_lag_ldscore_annot_complete_device(STORM_dosage_t* h, int stat, uint64_t max_lag, const double* pos, double max_dist,
                                                   const float* d_annot, uint64_t n_annot, uint64_t annot_ld, float* d_score,
                                                   uint64_t score_ld, uint32_t* d_n_pairs, uint64_t out_rows);

/* Greedy LD pruning and clumping, resolved on the device: n bytes leave it instead of the n x L matrix of
 * STORM_dosage_pairw_lag_corr. Both are ONE definition — the lexicographically first maximal independent set of a graph:
 *   vertices  the n rows held.
 *   edges     rows i < j are adjacent when j - i <= L = min(max_lag, n - 1), j lies in i's window — pos == NULL: the lag
 *             alone; pos given (n doubles, HOST memory in every form): |pos[j] - pos[i]| <= max_dist, with max_lag 0 taking
 *             the lag the windows need and a max_lag the windows exceed REFUSED, never clipped: the rule and the planner of
 *             STORM_dosage_lag_ldscore_annot above — and rho > min_r2, where rho is the FLOAT that
 *             STORM_dosage_pairw_lag_corr writes for the pair under STORM_DOSAGE_R2 (the _complete calls: the float of
 *             STORM_dosage_pairw_lag_corr_complete, 3 = STORM_DOSAGE_MISSING). The comparison is between floats and
 *             strict: a pair exactly at the threshold is not an edge, and a NaN rho is never an edge.
 *   order     priority: n floats in HOST memory in every form, or NULL. Higher priority comes first, ties go to the lower
 *             row index; NULL means row order. +-inf is allowed, a NaN priority is refused (the message names the first
 *             such row). Clumping: priority = -log10(p) or -p. Pruning: NULL, or the minor allele frequency.
 *   result    walk the rows in that order; a row is KEPT exactly when no already-kept row is adjacent to it.
 *               keep[i]  = 1 or 0.
 *               owner[i] = i for a kept row; for a removed row the kept row adjacent to it that comes first in the order —
 *                          the clump the row belongs to. owner may be NULL; keep is the same bytes either way.
 * A row without any edge is always kept — also a CONSTANT row, whose pairs are all NaN (_complete: a row with fewer than
 * two calls, or constant on them): drop monomorphic rows with STORM_dosage_row_sums before or after. With exactly one row,
 * keep[0] = 1 and owner[0] = 0; with none, nothing is written.
 * This is the greedy of clumping tools and of priority pruning. It is NOT PLINK's --indep-pairwise, which slides a window
 * by a step and removes by MAF inside it, and the r^2 here is this library's float: no bit-equality with any outside tool
 * is claimed. The answer is unique: two calls on unchanged rows return identical bytes.
 * Exactly elements [0, n) of keep and owner are written (out_len >= n is the length of both), in host memory or, for the
 * _device forms, in DEVICE memory (complete on return; pos and priority stay host memory). Nothing is written on a
 * refusal. At most STORM_PRUNE_MAX_ROWS rows: the device resolves the order in one workgroup with a bit per row in its
 * local memory; more are refused, never truncated. Device scratch: the n x L floats of r^2, n x (2 ceil(L / 32) + 2) words
 * of adjacency masks and the scratch of the corr call beneath. No CPU fallback. One device slot and one process.
 * Returns 0; -1 NULL handle, -2 NULL keep, -3 max_lag 0 without positions (said before the size check), -4 out_len < n
 * (nothing is written), -3 a NaN min_r2, more than STORM_PRUNE_MAX_ROWS rows, a negative or NaN max_dist, a position that
 * is not finite or decreases, windows that need more than max_lag (the message names both numbers), a NaN priority, or a
 * device failure (STORM_hip_error says which), -5 several device slots in view. */
#define STORM_PRUNE_MAX_ROWS 1048576
int STORM_dosage_lag_prune(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist,
                           const float* priority, uint8_t* keep, uint32_t* owner, uint64_t out_len);
int STORM_dosage_lag_prune_device(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist,
                                  const float* priority, uint8_t* d_keep, uint32_t* d_owner, uint64_t out_len);
int STORM_dosage_lag_prune_complete(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist,
                                    const float* priority, uint8_t* keep, uint32_t* owner, uint64_t out_len);
int STORM_dosage_lag_prune_complete_device(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist,
                                           const float* priority, uint8_t* d_keep, uint32_t* d_owner, uint64_t out_len);

/* The sparse LD report, compacted on the device: the pairs of STORM_dosage_pairw_lag_corr's n x L matrix whose r^2 passes a
 * threshold (PLINK's --r2 --ld-window N --ld-window-kb K --ld-window-r2 T), instead of the matrix. The list is exactly the
 * edge set STORM_dosage_lag_prune above walks, forward pairs only (i < j):
 *   listed    i < j with j - i <= L = min(max_lag, n - 1), j in i's window — pos == NULL: the lag alone; pos given (n doubles,
 *             HOST memory in every form): the windows, max_lag 0 and the refusal of a max_lag the windows exceed as in
 *             STORM_dosage_lag_prune — and rho > min_r2, where rho is the FLOAT STORM_dosage_pairw_lag_corr[_complete] writes
 *             for the pair under STORM_DOSAGE_R2. The comparison is between floats and STRICT: a pair exactly at the
 *             threshold is NOT listed (PLINK's filter is >=: pass the next float below T for that), and a NaN rho is never
 *             listed. A negative min_r2 lists every pair of the window whose rho is a number.
 *   layout    CSR: row i's pairs are col[row_start[i] .. row_start[i + 1]), col holds j ascending within a row, val the
 *             pair's rho — the same 32 bits as out[i * ld + (j - i - 1)] of the corr call. row_start has n + 1 entries of 64
 *             bits (out_rows >= n + 1 is its length), row_start[n] is the total; col is 32 bits.
 *   capacity  the length of col and val. col == NULL && val == NULL with capacity 0 is the count-only call: row_start and
 *             *n_pairs alone. Host forms: a total above capacity returns -4 with row_start and *n_pairs valid, col / val
 *             unspecified, and the message naming both numbers. _device forms (d_row_start, d_col, d_val in DEVICE memory;
 *             no n_pairs): they return with their work queued and cannot know the total — d_row_start always holds the true
 *             offsets, only the first `capacity` pairs in (i, j) order are written, nothing is ever written at or beyond
 *             index capacity, and the caller compares d_row_start[n] with capacity. A _device form given pos waits before it
 *             returns (its windows are freed on return); without pos its outputs are final once the work queued on the
 *             container's stream is.
 * With no row, row_start[0] = 0 is written where out_rows >= 1; with one row, row_start[0] = row_start[1] = 0; the host
 * forms ask no device for either. There is no limit of STORM_PRUNE_MAX_ROWS rows here. Two calls on unchanged rows return
 * identical bytes. Device scratch: the n x L floats of r^2, n x ceil(L / 64) 64-bit mask words, and for a host form the staged
 * list; no CPU fallback. One device slot and one process.
 * Returns 0; -1 NULL handle, -2 NULL row_start (host forms: or NULL n_pairs), exactly one of col / val NULL, or a capacity
 * without them, -3 max_lag 0 without positions (said before the size check), -4 out_rows < n + 1 (nothing is written), -3 a
 * NaN min_r2, a negative or NaN max_dist, a position that is not finite or decreases, windows that need more than max_lag
 * (the message names both numbers), or a device failure (STORM_hip_error says which), -4 a capacity below the total (host
 * forms), -5 several device slots in view. */
int STORM_dosage_lag_corr_sparse(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist,
                                 uint64_t* row_start, uint64_t out_rows, uint32_t* col, float* val, uint64_t capacity,
                                 uint64_t* n_pairs);
int STORM_dosage_lag_corr_sparse_device(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist,
                                        uint64_t* d_row_start, uint64_t out_rows, uint32_t* d_col, float* d_val, uint64_t capacity);
int STORM_dosage_lag_corr_sparse_complete(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist,
                                          uint64_t* row_start, uint64_t out_rows, uint32_t* col, float* val, uint64_t capacity,
                                          uint64_t* n_pairs);
int STORM_dosage_lag_corr_sparse_complete_device(STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos,
                                                 double max_dist, uint64_t* d_row_start, uint64_t out_rows, uint32_t* d_col,
                                                 float* d_val, uint64_t capacity);

/* ------------------------------------------------------------- extensions (not in ref) ---
 * Device selection for the entry points above. By default device 0 computes everything.
 * STORM_hip_set_devices(n, ids): the pair space is sharded over the listed GPUs of this node
 * (one replica of the data per GPU, disjoint shards of the tile list) and the per-GPU partial
 * sums are added on the host. Multi-PROCESS runs (one rank per GPU, RCCL all-reduce) use
 * STORM_hip_set_shard(rank, world): each process then returns only its shard's partial. */
int STORM_hip_set_devices(int n_devices, const int* device_ids);
/* The containers keep a device copy of their rows between all-pairs calls. It follows every
 * change made through STORM_add / STORM_clear / STORM_contig_add / STORM_contig_clear, and for
 * STORM_t also edits made with the public per-row / per-block adders and clears directly on
 * h->conts[i] (a fingerprint of rows, blocks, set-bit counts and each block's stamp — the epoch of its
 * last change through those functions — is compared on every call: a clear and an add that give back
 * the same ids and counts are seen too). What it cannot
 * see is a caller writing into the public buffers in place (h->data, bitmaps[i].data: the
 * reference structs are not opaque): after such an edit call the matching function below, or the
 * next all-pairs call answers for the rows as they were. Returns 0, -1 for a NULL handle. */
int STORM_hip_invalidate(STORM_t* bitmap);
int STORM_contig_hip_invalidate(STORM_contiguous_t* bitmap);
/* Caller threads on distinct GPUs: after STORM_hip_set_devices(n, ids), a thread that calls
 * STORM_hip_set_thread_devices(first_slot, n_slots) drives only the device slots [first_slot, first_slot + n_slots)
 * with its all-pairs calls (n_slots = 0: all slots again) — the handles it uses keep their device mirrors there — and
 * only those slots are locked, so threads on distinct slots run side by side (one lock per device slot; the raw-buffer
 * STORM_wrapper_* calls keep one set of device matrices per process and lock all slots). Returns 0, -1 if the run of
 * slots is not inside the configuration. A handle is still for one thread at a time, as in the reference. */
int STORM_hip_set_thread_devices(int first_slot, int n_slots);
/* A context option (include/storm_hip.h: storm_hip_ctx_set_option — kernel forms, work-list shaping) for every device
 * context behind the handles, existing and future; the environment variable STORM_HIP_OPTIONS="key=value,key=value" does the
 * same. Tuning and A/B measurements: no option changes a result. 0, or -1 (unknown key / value out of range). */
int STORM_hip_set_option(const char* key, int64_t value);
int STORM_hip_set_shard(uint32_t shard_rank, uint32_t shard_count);
/* What the last all-pairs call ran, over this process's devices (storm_hip.h: storm_hip_last_pass_report):
 * out[0] mask of STORM_HIP_RAN_*, out[1] dense 64-bit word pairs, out[2] list-probe lookups, out[3] rows a
 * lookup stands for. For harnesses that price a row against the roof of the kernel that ran. */
int STORM_hip_last_pass(uint64_t out[4]);
const char* STORM_hip_error(void);
/* Multi-PROCESS runs, one process per GPU: every process sets its shard (STORM_hip_set_shard) and joins one
 * RCCL communicator; from then on every all-pairs entry point above returns the SUM over all processes (the
 * shard partials all-reduced over xGMI: ncclAllReduce of one uint64), so host code written for the reference
 * needs nothing else. Rank 0 obtains the 128-byte id and hands it to the other processes (pipe, file, MPI);
 * STORM_hip_comm_init is collective — every process calls it, after it was forked / started and before its
 * first all-pairs call. Return 0, or -1 with the reason in STORM_hip_error().
 * (tools/storm_benchmark.cpp --ranks N: fork before any HIP call, id through a pipe.) */
int STORM_hip_comm_unique_id(uint8_t id[128]);
int STORM_hip_comm_init(const uint8_t id[128]);
int STORM_hip_comm_finalize(void);
/* Threading. Like the reference (no locks anywhere in storm.c), a HANDLE is not thread-safe: one thread at a
 * time per STORM_t / STORM_contiguous_t. Different handles may be used from different threads: every entry point
 * that touches a device (the all-pairs calls, STORM_contig_pairw_matrix, the raw-buffer wrappers, the streaming of
 * STORM_contig_add) locks the device slots it drives — one lock per configured device, the contexts behind the
 * handles are shared — so concurrent passes are safe; threads whose views (STORM_hip_set_thread_devices) are
 * disjoint slots run side by side, threads on the same slots one after the other. The device selection
 * (STORM_hip_set_devices / _set_shard, the environment) is read on first use: change it only while no other
 * thread is inside the library.
 * STORM_hip_shutdown(): releases the wrappers' cached device matrices and every device context (handles that
 * still hold device copies re-create them on their next all-pairs call). Returns 0. */
int STORM_hip_shutdown(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* STORM_H_MI355X_DROPIN */
