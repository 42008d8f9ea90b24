// storm_hip_internal.h — shared between the .hip translation units of libstorm_hip.so.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <exception>
#include <cstring>
#include <new>
#include <optional>
#include <thread>
#include <utility>
#include <variant>
#include <vector>

#include "storm_hip.h"
#include "storm_hip_plan.h"   // the work-list records, their geometry and the planners (host-only: storm_hip_plan.cpp)

struct storm_hip_ctx_s;
typedef struct storm_hip_ctx_s storm_hip_ctx_t;
struct storm_hip_matrix_s;

namespace storm {

#define STORM_HIP_TRY(expr)                                                                  \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            ::storm::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),        \
                               __FILE__, __LINE__);                                          \
            return STORM_HIP_EHIP;                                                           \
        }                                                                                    \
    } while (0)

// No C++ exception may cross the C boundary: every extern "C" entry point that can reach a
// std::vector or operator new runs its body through this (bad_alloc -> STORM_HIP_ENOMEM).
template <typename Fn>
static inline int guarded(const char* what, Fn&& fn) noexcept {
    try {
        return fn();
    } catch (const std::bad_alloc&) {
        set_error("%s: out of host memory", what);
        return STORM_HIP_ENOMEM;
    } catch (const std::exception& e) {
        set_error("%s: %s", what, e.what());
        return STORM_HIP_EHIP;
    } catch (...) {
        set_error("%s: unknown C++ exception", what);
        return STORM_HIP_EHIP;
    }
}

// the first check of every entry point that takes a context
static inline int check_ctx(const storm_hip_ctx_t* ctx) {
    if (!ctx) {
        set_error("NULL context");
        return STORM_HIP_EINVAL;
    }
    return STORM_HIP_OK;
}

// A grow-only device buffer of the context's workspace, capacity in bytes. ensure() never shrinks and keeps the
// contents only when it does not reallocate (every caller refills); a failed allocation leaves the buffer empty.
// Reads as its pointer.
template <class T>
struct DevBuf {
    T* d = nullptr;
    size_t capacity = 0;
    operator T*() const { return d; }
    int ensure(size_t bytes, const char* what, size_t floor_bytes = 0) {
        if (bytes <= capacity) return STORM_HIP_OK;
        T* const old = d;
        d = nullptr;
        capacity = 0;
        if (old) STORM_HIP_TRY(hipFree(old));
        bytes = std::max(bytes, floor_bytes);
        if (hipMalloc(reinterpret_cast<void**>(&d), bytes) != hipSuccess) {
            d = nullptr;
            set_error("%s: hipMalloc of %zu bytes failed", what, bytes);
            return STORM_HIP_ENOMEM;
        }
        capacity = bytes;
        return STORM_HIP_OK;
    }
    void release() {
        if (d) (void)hipFree(d);
        d = nullptr;
        capacity = 0;
    }
};

// A work list planned on the host and kept on the device with the request it was planned from (DESIGN.md "One cached work
// list"): the record buffer, the key and the count. A launcher builds its request; a list that holds() it is launched as it
// stands; otherwise the launcher plans, checks its limits and put()s the new list, the one place where a list goes up and
// the host waits for it. forget() drops the key and the count and keeps the buffer; whoever overwrites a buffer that several
// lists share forgets the list it held. Rec void: a buffer of one record type at a time (put takes the records' type).
template <class Rec, class Key>
struct WorkList {
    DevBuf<Rec> d;
    std::optional<Key> key;   // the request the list was planned from (none: no list)
    uint32_t n = 0;           // records of that list
    const Rec* recs() const { return d.d; }
    bool holds(const Key& k) const { return d && key == k; }
    void forget() {
        key.reset();
        n = 0;
    }
    // forgets; grows the buffer (to floor_bytes at least when it grows); copies the records up on the context's stream and
    // waits for them (the host vector is pageable and leaves scope; nothing for an empty list); then count and key (none:
    // a list nobody asks for again). Every early return leaves the list forgotten. `what` names the list in the messages.
    template <class R>
    int put(storm_hip_ctx_t* ctx, std::optional<Key>&& k, const R* recs, size_t count, const char* what, size_t floor_bytes = 0);
    void release() {
        d.release();
        forget();
    }
};

// K1's segment table, of the context (the dense matrix) or of a sparse container (its block columns)
struct SegRequest {
    uint64_t n_rows;   // the dense matrix's rows; a sparse container's columns are its own: 0
    uint32_t shard_rank, shard_count, seg_len;
    bool operator==(const SegRequest& o) const {
        return n_rows == o.n_rows && shard_rank == o.shard_rank && shard_count == o.shard_count && seg_len == o.seg_len;
    }
};
struct SegList : WorkList<Seg, SegRequest> {
    uint64_t row_sum = 0;   // sum over segments of (j_hi - j_lo)
};

// The item buffer of the tile kernels: ONE list at a time, of MfmaItem records (sum mode, matrix output) or of PartItem
// records (K2h). The key's alternative says which; `n` counts the list that is there, so a forgotten or another kind's list
// is zero items to every reader that has just ensured its own.
struct ItemList : WorkList<void, std::variant<TileSumRequest, MatrixTilesRequest, Tile128Request>> {
    MatrixPlan matrix_plan;   // of the matrix-output list
    template <class Rq>
    bool holds(const Rq& rq) const {   // (no variant is built for the comparison: a MatrixTilesRequest owns vectors)
        const Rq* have = key ? std::get_if<Rq>(&*key) : nullptr;
        return d && have && *have == rq;
    }
};

// The strip list of an all-pairs pass with the per-XCD queue bounds of its persistent form (plan_strips)
struct StripList : WorkList<StripItem, StripRequest> {
    uint32_t queue_base[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t queue_count[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

// The strip list of one row panel of launch_pairw_bits_upload, kept on the device between calls
struct PanelList {
    WorkList<StripItem, StripRequest> list;
    hipEvent_t landed = nullptr;   // the panel's rows have arrived
};

// Geometry of the dense kernel (see DESIGN.md "K1").
constexpr int kLanes = 64;                           // gfx950 wavefront
constexpr int kWaves = 4;                            // waves per workgroup
constexpr int kThreads = kLanes * kWaves;            // 256
// (kChunkWords = 64, the k-chunk of one 64-bit word per lane: storm_hip_plan.h)
constexpr int kRowsPerWave = 32;                     // A rows held in VGPRs by one wave
static_assert(kABlockRows == kWaves * kRowsPerWave, "128 A rows per workgroup (storm_hip_plan.h)");
constexpr int kRowPad = 256;                         // allocated rows: a multiple of this, zero beyond n_rows (a strip's A tile)
constexpr int kStageRows = 32;                       // B rows per LDS stage
constexpr int kSlots = 4096;  // partial-sum slots (uint64 each)
constexpr int kSlotsExtra = 8;  // words behind the slots: work-queue heads, zeroed by the fold

// (Seg, one (A block, B row range) segment of the upper triangle: storm_hip_plan.h)
// shared launcher of the dense kernel over an arbitrary segment table (dense + sparse paths)
int launch_pairw_segments(storm_hip_ctx_t* ctx, const uint64_t* X, uint64_t stride_words,
                          const Seg* d_segs, uint32_t n_segs, uint64_t seg_row_sum,
                          uint64_t* d_total);

}  // namespace storm

struct storm_hip_ctx_s {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t switch_ev = nullptr;          // storm_hip_ctx_set_stream: recorded on the stream that is left, waited for by the next one
    int n_cus = 0;
    // workspace
    unsigned long long* d_slots = nullptr;   // kSlots partial sums
    unsigned long long* d_scalar = nullptr;  // one uint64 result
    unsigned long long* h_scalar = nullptr;  // pinned host word the result is read back through
    // [r5] result mailbox: a pinned, device-visible host word the LAST kernel of a synchronous all-pairs call writes the
    // total into directly; the host polls it (sentinel ~0 = not there yet) instead of queueing an 8-byte copy behind the
    // kernel and sleeping in hipStreamSynchronize — 5 - 7 us of a call that is 18 - 30 us at the sparse end and at LD-window
    // row counts. Option result_mailbox (1 on / 0 off: the copy + synchronize of rounds 1 - 4).
    unsigned long long* h_mail = nullptr;
    unsigned long long* d_mail = nullptr;    // the same word as the device sees it
    int result_mailbox = 1;
    int sync_poll_us = 0;                    // [r6] synchronous matrix-output calls poll hipStreamQuery this long before they park in hipStreamSynchronize (0: park at once)
    bool mail_armed = false;                 // the call in flight was launched into the mailbox
    // [r6] device / pinned allocations whose release (hipFree waits for the device: ~0.2 ms each, eleven of them behind an
    // arena build) is put off until the call AFTER the one that made them obsolete, or the context's end
    std::vector<void*> deferred_free, deferred_host_free;
    uint32_t deferred_age = 0;
    hipEvent_t stage_ev[3] = {nullptr, nullptr, nullptr};   // the ring's rotation lives in the context: one Stager after another continues it and waits for the copy that last left a buffer
    bool stage_used[3] = {false, false, false};
    int stage_next = 0;
    void* h_stage_ring = nullptr;            // pinned staging ring of the sparse arena builder (storm_hip_sparse.hip: Stager), allocated on first use
    storm::SegList segs;                     // K1: segment table of the last geometry
    // options
    int variant = -1;       // -1 auto, 0/1/2 popcount kernel (B path), 3 MFMA tiles, 4 MFMA strips
    int variant_used = 2;   // what the last dense launch ran
    int probe_bundle = -1;  // [r6] list-probe kernel: -1 / 1 = one group of 128 rows per workgroup (probe_lists_kernel), 4 = bundles of four groups per workgroup (probe_lists_fat_kernel: a quarter of the loads and workgroups, measured 5 - 25 % SLOWER at every c4 load, profiles/r06_*_probe_bundle.txt)
    int sparse_probe = -1;  // sparse container: list-probe kernel for columns of short lists (-1 auto, 0 never, 1 always)
    int matrix_lists = -1;  // per-pair matrix of a list-only sparse container from its lists (K5, storm_hip_lists.hip): -1 by density, 0 never, 1 whenever eligible
    int matrix_lists_kernel = 0;  // K5: 0 = by the row length, 1 = lists_matrix_kernel (windows), 2 = lists_hash_kernel where a group fits the table
    int matrix_lists_hash_min_log2 = 6;  // ... the hash kernel from this group size on (log2 of 8 .. 64 rows)
    int matrix_lists_debug = 0;   // timing ablations of lists_matrix_kernel (wrong results): 1 no element loads, 4 no barriers, 8 no stores, 16 no steps
    int matrix_lists_permille_x10 = 80;  // ... the crossover density in 1/10000 of the dense replica's bits ([r6] 60 -> 80: the window kernel takes 5.2 ms at 0.8 % where the dense replica takes 6.4; level at 0.95 %)
    int seg_rows = 256;
    int chunks_per_item = 0;
    // info of the last dense launch
    uint64_t last_info[4] = {0, 0, 0, 0};
    uint64_t sparse_census[4] = {0, 0, 0, 0};
    // What the last all-pairs pass ran (storm_hip_last_pass_report): [0] kernels, a mask of STORM_HIP_RAN_*;
    // [1] 64-bit word pairs multiplied on the matrix cores or by the popcount kernel (this shard's share,
    // algorithmic: pairs x words); [2] positions the list-probe kernel streamed = its lookups; [3] rows one
    // lookup stands for (128). A harness prices every row against the roof of the kernel that ran.
    uint64_t pass_report[4] = {0, 0, 0, 0};
    // K2 (MFMA FP4) state: nibble-expanded shadow of the matrix + item table
    storm::DevBuf<uint8_t> d_x4;
    storm::ItemList items;           // the tile kernels' list: one at a time (sum mode, matrix output or K2h)
    std::vector<storm::PanelList> panel_lists;   // work lists of the row panels of storm_hip_pairw_dense_upload
    hipStream_t copy_stream = nullptr;   // ... its copies travel here while ctx->stream multiplies the panel before
    storm::StripList strips;         // the strip list of the last all-pairs pass; the rectangle (launch_square_mfma) overwrites it without a key
    int k2_stages_per_item = 32;
    int k2_max_run = 0;     // strips: B stages per item at most; 0 = 64 / 96 / 128, whichever list schedules shortest (ensure_strip_items)
    int k2_ring = 4;        // K2s: LDS ring depth (3, 4 or 5)
    int k2_shadow_budget_mb = 96 * 1024;  // K2s: FP4 shadow above this many MiB -> k-chunked passes (0 = never)
    int k2_strip_operands = 0;  // strips: 0 = K2b; 5 = bit operands, FP4 image of every B stage built in the LDS (strip16_bits_kernel, K2b); 2 = bit operands, one stage stream per workgroup, one launch (bitstream_kernel, K2q); 4 = FP4 shadow (strip16_fp4_kernel / strip_fp4_kernel); 1 = bit operands, one item per workgroup (stripbits_kernel)
    int k2_stream_max_rows = 8192;  // auto: matrices up to this many rows take K2q
    int k2_shard_pairs = 0;         // ownership among shards: 0 = whole k-slices first (leftover slices along the pair space), 1 = every slice along the pair space
    int k2_matrix_pad = -1;         // matrices created from now on: rows that are a multiple of 1 KiB get this many 512-byte chunks more of pitch (0: dense pitch; -1: by the pitch, pitch_pad_chunks)
    int k2_fold_inline = -1;        // K2b: the workgroup dispatched last folds the partial sums inside the launch: -1 = for short launches (<= 4096 workgroups, where the fold launch and its gaps are a fifth of a pass), 1 = always (level at N = 10000), 0 = never (a fold launch behind the strips); profiles/r05_c_fold_ab.jsonl
    int k2_operands_used = 4;       // what the last strip launch ran: 4 = FP4, 5 = K2b (64 or 128 A rows per wave: k2_strip_rows_used), 6 = K2b on 512-row A tiles, 2 = K2q; tools build: 1, 3 (choose_pass, storm_hip_plan.h)
    int k2_strip_rows = 0;          // K2b: A rows per wave: 64 = strip16_bits_kernel (256-row A tiles, slices of a class pair of 512 bits), 128 = strip16_rows_kernel (512-row A tiles, slices of 128 bits) where the matrix's zero rows reach the next multiple of 512 (otherwise 64), 0 = by the rule (choose_pass, storm_hip_plan.cpp)
    int k2_strip_rows_used = 64;    // what the last K2b launch ran: 64 or 128
    int k2_tile_shape = 0;  // write-mode tile kernel: 0 = by the matrix (5 for a dense matrix, 2 for the dense replica of a sparse container: sparse operands let tilebits8_kernel, which sits at the socket's power cap, clock higher; crossover near 20 % density, profiles/r05_g_*); 5 = tilering_kernel (both operands as FP4 images in the LDS, 16x16x128); 2 = tilebits8_kernel (bit operands inflated in registers, 32x32x64); 3 / 4 = K2tb; 1 / 16 / 32: tools build
    int k2_wave_below = 400;      // [r6] k2_tile_shape 0: matrices (bands, rectangles) of fewer 256 x 256 tiles than this take tile128_kernel (K2h: 128 x 128 tiles, cut along k where they are too few, the parts' sums meeting inside the launch; no window clearing, no atomics into the output)
    int k2_part_slots = 0;        // K2h: segments per CU the tiles' chunk stream is cut into: 0 = two once that leaves segments of 4 x k2_part_min_chunks, else one; 1 / 2: forced
    int k2_part_min_chunks = 8;   // K2h: a k-part is at least this many 512-bit chunks
    int k2_part_narrow = 1;       // K2h: windows of 16-bit counts where every part of a tile covers fewer than 2^16 bits of k (half the bytes the part that ends the tile has to read)
    int k2_part_cost_diag = 80;   // K2h: what a chunk of a tile on the diagonal costs next to one of a full tile, percent
    storm::DevBuf<uint32_t> d_tickets;   // K2h: one arrival counter per tile (zero between launches)
    bool tickets_dirty = false;   // a launch failed: clear the tickets before the next one
    int k2_tile_shape_eff = 2;  // what the call in flight runs (set by launch_pairw_matrix / launch_square_matrix)
    int k2_ring_sync = 0;   // tilering_kernel: 0 = one s_barrier per stage; 1 = arrival counters in the LDS (waves may drift a stage apart; measured 2 % slower)
    int k2_ring_cost_diag = 78, k2_ring_cost_ragged = 40;  // the same for tilering_kernel (k2_tile_shape = 5)
    int k2_tile_cost_diag = 63, k2_tile_cost_ragged = 30;  // percent of a full tile (tilebits8_kernel): what the planner assumes when it cuts the last round
    int k2_shape = 16;      // K2s: MFMA shape of the default strip kernel: 16 = 16x16x128 (default), 32 = 32x32x64
    int k2_persistent = 0;  // K2s: workgroups pull items from per-XCD queues (0: one item per workgroup)
    // "keep_shadow": reuse the FP4 shadow across all-pairs calls while (matrix, generation, shard,
    // layout) are unchanged. Only valid if the matrix is modified through the library alone.
    int keep_shadow = 0;
    uint64_t x4_key[4] = {0, 0, 0, 0};
    int k2_matrix_split = 1; // matrix output: cut the last round's tiles along k to fill the CUs
    int k2_matrix_parts = 0;  // ... 0: the parts add into the cleared output with atomics; 1: every part writes its own window and reduce_parts_kernel adds them up (round 5: the tile kernel gets 10 us faster at 1024 rows, the second kernel costs more than the clearing and the atomics did: profiles/r05_k_matrix_sizes.jsonl)
    storm::DevBuf<uint32_t> d_parts;   // the parts' windows (256 x 256 uint32 each)
    int k2_matrix_min_part = 32;  // ... into parts of at least this many 128-bit stages (a multiple of 4)
    int k2_pitch_pad = -1;  // K2/K2s: extra bytes per row of the FP4 shadow (multiple of 128; -1 = auto)
    int k2_lds_pad = 0;     // K2s: bytes of unused dynamic LDS per workgroup (caps workgroups per CU)
    int k2_lpt_rounds = 6;  // K2s: XCD lists of at most this many rounds of 128 items are sorted longest-first
    int k2_tail_slices = 3; // K2s: last slices of every XCD's list are cut into short runs ...
    int k2_tail_run = 32;   //      ... of at most this many stages, merged longest-first
    int k2_tail_set = 0;    // the caller has set k2_tail_slices or k2_tail_run: the 128-rows-per-wave form's planner then takes both as they are (otherwise it chooses them with the run length: choose_strip_shaping)
    int k2_max_run_used = 0, k2_tail_run_used = 0, k2_tail_slices_used = 0;   // the shaping of the strip list planned last (0: none yet)
    // "time_kernels" option: HIP event pairs around the dominant kernel of every pairwise launch
    // (the popcount kernel, the tile kernel or the strip kernel), read by storm_hip_kernel_time
    int time_kernels = 0;
    std::vector<hipEvent_t> kernel_events;  // begin/end alternating
    size_t kernel_events_used = 0;
    storm::DevBuf<uint32_t> d_band;     // device staging of the host-output matrix calls (band x n_rows uint32)
    storm::DevBuf<uint64_t> d_dosage_rows;   // dosage rows with missing genotypes: the split operands G, H, M (storm_hip_dosage.hip)
    storm::DevBuf<uint32_t> d_dosage_sums;   // ... and the products G M^T, H M^T and N of storm_hip_pairw_dosage_corr_complete
    storm::DevBuf<void> d_positions;    // staging of storm_hip_matrix_set_rows_from_positions: offsets, then positions
    storm::DevBuf<uint32_t> d_counts;   // row-count scratch of the matrix-output paths
    storm::DevBuf<unsigned long long> d_trace;  // k2_ring = 18: per-item schedule trace of the strip kernel
    uint32_t trace_items = 0;
    // K2q (bitstream_kernel): per-workgroup bounds + stage bases of the last geometry (never empty: it carries the key) and
    // the segment table planned with them
    storm::WorkList<uint32_t, storm::BitstreamRequest> bitfirst;
    storm::DevBuf<storm::BitSeg> d_bitsegs;
    uint32_t n_bit_groups = 0, n_bit_segs = 0, bit_max_stages = 0;
    uint64_t bit_stages = 0;
    int k2_stream_groups_per_cu = 0;  // K2q: workgroups per CU (0 = by the length of the stream: 1, 2 or 3)
    int k2_stream_min_piece = 6;      // K2q: stages a workgroup should at least have before a CU's share is cut further
    int k2_stream_min_run = 2;        // K2q: a cut leaves at least this many later blocks on either side
    // K2q: length of the shares of the second / third workgroup of a CU in percent of the first one's, when the
    // stream is one round of 3 workgroups per CU (build_bitstream: the SIMD arbiter serves the oldest wave)
    int k2_stream_w3_1 = 120, k2_stream_w3_2 = 60;
    int k2_wave_ring = 0;             // K2w: stages of a wave's private ring (0 = by workgroups per CU: 8 / 4 / 3)
    bool trace_is_stream = false;     // d_trace holds per-workgroup words of bitstream_kernel (no strip items)
    int k2_debug = 0;  // timing probes (wrong results): 1 = all items on tile (0,0), 2 = no XCD grouping
};

namespace storm {
// K2: all-pairs total of a dense matrix through v_mfma_f32_32x32x64_f8f6f4 (storm_hip_mfma.hip)
int launch_pairw_mfma(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, uint32_t shard_rank,
                      uint32_t shard_count, const PassChoice& pass, uint64_t* d_total);
int launch_pairw_mfma_ranges(storm_hip_ctx_t* ctx, const uint64_t* X, uint64_t stride_words,
                             uint64_t n_rows_src, uint64_t n_rows_dst,
                             const std::vector<RowRange>& ranges, uint32_t shard_rank,
                             uint32_t shard_count, int strip_mode, uint64_t* d_total,
                             uint64_t shadow_generation = 0, uint32_t n_words_logical = 0);
int launch_pairw_bits_upload(storm_hip_ctx_t* ctx, storm_hip_matrix_s* m, const uint64_t* host_rows,
                             uint64_t src_stride_words, const StripForm& form, uint64_t* d_total);   // storm_hip_mfma.hip
int stage_check_lists(const storm_hip_stage_s* stage, const std::vector<uint64_t>& ltable);   // storm_hip_sparse.hip: EINVAL for a token the stage cannot answer
int stage_gather_lists(storm_hip_ctx_t* ctx, storm_hip_stage_s* stage, const std::vector<uint64_t>& ltable, uint16_t* d_lists,
                       uint64_t** d_table);   // storm_hip_sparse.hip: staged list blocks -> a block-ordered list buffer
int launch_pairw_bits_ranges(storm_hip_ctx_t* ctx, const uint8_t* X, uint64_t pitch_bytes,
                             const std::vector<RowRange>& ranges, const StripForm& form, uint32_t n_words, uint32_t shard_rank,
                             uint32_t shard_count, uint64_t* d_total, bool slots_hold_sums = false);
// what choose_pass (storm_hip_plan.h) reads of the context
static inline PassOptions pass_options_of(const storm_hip_ctx_t* ctx) {
#ifdef STORM_HIP_PROBES
    constexpr bool tools = true;
#else
    constexpr bool tools = false;
#endif
    return {ctx->variant, ctx->k2_strip_operands, ctx->k2_strip_rows, ctx->k2_ring, ctx->k2_shape, ctx->k2_persistent, ctx->k2_debug, tools};
}
// pairs x words of a set of row ranges, divided among shard_count shards (the report's algorithmic word pairs)
static inline uint64_t ranges_word_pairs(const std::vector<RowRange>& ranges, uint64_t words, uint32_t shard_count) {
    uint64_t pairs = 0;
    for (const RowRange& rg : ranges) {
        const uint64_t n = rg.r1 - rg.r0, a = rg.a_end ? std::min(rg.a_end, rg.r1) - rg.r0 : n;
        pairs += a * (a - (a != 0)) / 2 + a * (n - a);
    }
    return pairs * words / (shard_count ? shard_count : 1);
}
// The per-pair launchers below only queue; pair_matrix_out (further down) is where a synchronous call waits.
int launch_pairw_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, int op, uint32_t* d_out,
                        uint64_t ld, uint64_t band_row0 = 0, uint64_t band_rows = ~0ull);
// the same for the pairs within max_lag rows of each other, in the lag layout (n x L instead of n x n): always K2h
int launch_pairw_lag_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, int op, uint64_t max_lag, uint64_t band_row0,
                            uint64_t band_rows, uint32_t* d_out, uint64_t ld);
// the dot products of rows of 2-bit values, upper triangle (K2h in its dosage form; storm_hip_dosage.hip finishes them)
int launch_pairw_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, uint32_t* d_out, uint64_t ld);
// ... for the pairs within max_lag rows of each other, in the lag layout (K2h in its lag and dosage form)
int launch_pairw_lag_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, uint64_t max_lag, uint64_t band_row0,
                                   uint64_t band_rows, uint32_t* d_out, uint64_t ld);
// the rectangle of two such matrices: every row of A against every row of B (K2h in its dosage form, rectangle)
int launch_square_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, uint32_t* d_out,
                                uint64_t ld);
int launch_square_mfma(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a,
                       const storm_hip_matrix_s* b, uint64_t* d_total);
int launch_square_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a,
                         const storm_hip_matrix_s* b, int op, uint32_t* d_out, uint64_t ld);
int launch_row_counts(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* m, uint32_t* d_counts);
// ---- the finishing pass (finish_tiles_kernel.inc; Stat: the statistic, brought by the file that includes it) ----
// a statistic's words per row, planar: one device array per word
template <int W>
struct StatWords {
    const uint32_t* w[W];
    bool all() const {   // none is NULL
        for (const uint32_t* p : w)
            if (!p) return false;
        return true;
    }
};
// can one launch hold the tiles of rows x cols entries? (64 x 256 entries a tile; grid (column tiles, row tiles))
static inline bool finish_tiles_fit(uint64_t rows, uint64_t cols) { return (rows + 63) / 64 <= 65535u && (cols + 255) / 256 <= 0x7fffffffu; }
// finish_tiles_kernel<Stat, triangle> over n_rows x n_cols entries at d_io, finish_lag_tiles_kernel<Stat> over the rows
// [row0, row0 + n_band_rows) of the lag layout (from output row 0; ~0: to the last row): the checks of the *_finish_device
// calls under the name `who`, then queued on the context's stream
template <typename Stat>
int launch_finish_tiles(storm_hip_ctx_t* ctx, const char* who, void* d_io, uint64_t ld, uint64_t n_rows, uint64_t n_cols,
                        StatWords<Stat::W> rows, StatWords<Stat::W> cols, bool triangle, int measure, uint64_t scale);
template <typename Stat>
int launch_finish_lag_tiles(storm_hip_ctx_t* ctx, const char* who, void* d_io, uint64_t ld, uint64_t n_rows, uint64_t row0,
                            uint64_t n_band_rows, uint64_t max_lag, StatWords<Stat::W> stats, int measure, uint64_t scale);
// what the lag calls refuse alike; *lag = L = min(max_lag, rows - 1) (0 for an empty matrix) (storm_hip_similarity.hip)
int check_lag(const char* who, const storm_hip_matrix_s* m, const void* out, uint64_t max_lag, uint64_t ld, uint64_t* lag);
// the bit statistics over a count matrix in device memory, asynchronous (storm_hip_similarity.hip; the checks of
// storm_hip_similarity_finish_device)
int launch_similarity_finish(storm_hip_ctx_t* ctx, void* d_io, uint64_t ld, uint64_t n_rows, uint64_t n_cols,
                             const uint32_t* d_counts_rows, const uint32_t* d_counts_cols, int triangle, int measure,
                             uint64_t n_bits);
// the same pass over the lag layout (rows [row0, row0 + n_band_rows) from output row 0)
int launch_similarity_finish_lag(storm_hip_ctx_t* ctx, void* d_io, uint64_t ld, uint64_t n_rows, uint64_t row0,
                                 uint64_t n_band_rows, uint64_t max_lag, const uint32_t* d_counts, int measure, uint64_t n_bits);
// lag_band_sums_kernel over a float matrix in the lag layout: per-row sums over both sides of the band, queued
// (storm_hip_ldscore.hip; the checks of storm_hip_lag_band_sums_device)
int launch_lag_band_sums(storm_hip_ctx_t* ctx, const float* d_vals, uint64_t ld, uint64_t n_rows, uint64_t max_lag, int stat,
                         uint64_t n_const, const uint32_t* d_nobs, uint64_t nobs_row_pitch, uint64_t nobs_col_stride,
                         float* d_score, uint32_t* d_n_pairs);
// lag_band_annot_sums_kernel: the band times an annotation matrix with a window per row (d_lo / d_hi: both or neither), queued
// (storm_hip_ldscore_annot.hip; the checks of storm_hip_lag_band_annot_sums_device)
constexpr uint32_t kLdscoreMaxAnnot = 1024;   // annotation columns of one call (the launch grid's y: 16 chunks of 64)
int launch_lag_band_annot_sums(storm_hip_ctx_t* ctx, const float* d_vals, uint64_t ld, uint64_t n_rows, uint64_t max_lag, int stat,
                               uint64_t n_const, const uint32_t* d_nobs, uint64_t nobs_row_pitch, uint64_t nobs_col_stride,
                               const uint32_t* d_lo, const uint32_t* d_hi, const float* d_annot, uint64_t annot_ld,
                               uint64_t n_annot, float* d_score, uint64_t score_ld, uint32_t* d_n_pairs);
// greedy pruning / clumping from a band in the lag layout (storm_hip_prune.hip): the checks the prune calls share behind
// their own NULL / max_lag / ld checks; the words of scratch the kernels need; the kernels themselves with that scratch at
// d_scratch, queued (n_rows >= 2, lag = min(max_lag, n_rows - 1); h_lo / h_hi / h_order are HOST arrays or NULL)
int check_lag_band_prune(const char* who, uint64_t n_rows, const uint32_t* h_lo, const uint32_t* h_hi, float min_r2);
size_t lag_band_prune_scratch_words(uint64_t n_rows, uint64_t lag, bool windows, bool order);
int launch_lag_band_prune(storm_hip_ctx_t* ctx, const char* who, const float* d_vals, uint64_t ld, uint64_t n_rows, uint64_t lag,
                          float min_r2, const uint32_t* h_lo, const uint32_t* h_hi, const uint32_t* h_order, uint8_t* d_keep,
                          uint32_t* d_owner, uint32_t* d_scratch);
// the sparse pair list of a band in the lag layout (storm_hip_lag_sparse.hip): the checks the sparse calls share behind their
// own NULL / max_lag / ld checks; the 32-bit words of scratch the kernels need; the kernels themselves with that scratch at
// d_scratch (8-byte aligned), queued (n_rows >= 2, lag = min(max_lag, n_rows - 1); h_lo / h_hi are HOST arrays or NULL;
// d_col / d_val NULL: the offsets alone)
int check_lag_band_sparse(const char* who, uint64_t n_rows, const uint32_t* h_lo, const uint32_t* h_hi, float min_r2,
                          const void* col, const void* val, uint64_t capacity);
size_t lag_band_sparse_scratch_words(uint64_t n_rows, uint64_t lag, bool windows);
int launch_lag_band_sparse(storm_hip_ctx_t* ctx, const float* d_vals, uint64_t ld, uint64_t n_rows, uint64_t lag, float min_r2,
                           const uint32_t* h_lo, const uint32_t* h_hi, uint64_t* d_row_start, uint32_t* d_col, float* d_val,
                           uint64_t capacity, uint32_t* d_scratch);
void release_mfma_state(storm_hip_ctx_t* ctx);
// releases what was put off (storm_hip_ctx_s::deferred_free); `aged`: only what an earlier call left behind
void drain_deferred(storm_hip_ctx_t* ctx, bool aged);
// one empty launch per translation unit (storm_hip_ctx_create): loads the TU's code object ahead of the first real call
void warm_mfma_code(hipStream_t stream);
void warm_sparse_code(hipStream_t stream);
void warm_lists_code(hipStream_t stream);
// ctx->d_scalar -> *h_total through the context's pinned word; synchronises the stream (storm_hip.hip)
int fetch_result_word(storm_hip_ctx_t* ctx, uint64_t* h_total);
// where a synchronous call launches its total: the mailbox (armed with the sentinel) or, without one, ctx->d_scalar
uint64_t* result_target(storm_hip_ctx_t* ctx);
// the armed mailbox's value once it has arrived (polls; falls back to a stream synchronize); STORM_HIP_EHIP if it never does
int wait_mailbox(storm_hip_ctx_t* ctx, uint64_t* value);
// folds ctx->d_slots into *d_total (device pointer) and re-zeroes the slots (storm_hip.hip)
int launch_fold_slots(storm_hip_ctx_t* ctx, uint64_t* d_total);
// record the next event of the "time_kernels" series on the launch stream (no-op when off)
void kernel_time_mark(storm_hip_ctx_t* ctx);
uint64_t next_matrix_generation();
// Host data -> device through a small ring of pinned buffers: the pieces of a chunk are packed by a few threads
// while the previous chunk's copy is in flight (pageable uploads of 1.7 GB were 0.15 s of c4's first call).
struct Piece { const void* src; size_t bytes; size_t dst_off; size_t zero_after = 0; };  // dst_off: byte offset from the chunk's device base; zero_after: bytes of zeros behind the piece
struct Stager {
    static constexpr size_t kBuf = 8u << 20;  // 8 MiB per buffer: 0.16 ms of PCIe time each
    static constexpr int kBufs = 3;
    storm_hip_ctx_t* ctx;
    hipEvent_t (&ev)[kBufs];   // (state of the context: see stage_ev)
    bool (&used)[kBufs];
    int& next;
    explicit Stager(storm_hip_ctx_t* c) : ctx(c), ev(c->stage_ev), used(c->stage_used), next(c->stage_next) {}
    static_assert(kBuf * kBufs == ((size_t)24 << 20), "storm_hip_ctx_reserve_staging allocates the same ring");
    int init() {
        if (!ctx->h_stage_ring) {
            if (hipHostMalloc(&ctx->h_stage_ring, kBuf * kBufs, hipHostMallocDefault) != hipSuccess) {
                ctx->h_stage_ring = nullptr;
                set_error("sparse_create: hipHostMalloc of the %zu-byte staging ring failed", kBuf * kBufs);
                return STORM_HIP_ENOMEM;
            }
        }
        for (int i = 0; i < kBufs; ++i)
            if (!ev[i] && hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) return STORM_HIP_EHIP;
        return STORM_HIP_OK;
    }
    // pieces[p0, p1): consecutive in the device destination (dst_off ascending from 0, no gaps beyond `span`)
    int send(uint8_t* d_base, const Piece* pieces, size_t n, size_t span) {
        uint8_t* buf = static_cast<uint8_t*>(ctx->h_stage_ring) + (size_t)next * kBuf;
        if (used[next] && hipEventSynchronize(ev[next]) != hipSuccess) return STORM_HIP_EHIP;
        const unsigned parts = span >= (1u << 20) ? 4u : 1u;   // (2 / 4 / 8 / 12 packers: 31 / 24 / 28 / 32 ms for c4's 420 MB of lists)
        auto pack = [&](unsigned part) {
            for (size_t i = n * part / parts; i < n * (part + 1) / parts; ++i) {
                memcpy(buf + pieces[i].dst_off, pieces[i].src, pieces[i].bytes);
                if (pieces[i].zero_after) memset(buf + pieces[i].dst_off + pieces[i].bytes, 0, pieces[i].zero_after);
            }
        };
        if (parts > 1) {
            std::thread helpers[3];
            for (unsigned t = 1; t < parts; ++t) helpers[t - 1] = std::thread(pack, t);
            pack(0);
            for (unsigned t = 1; t < parts; ++t) helpers[t - 1].join();
        } else {
            pack(0);
        }
        if (hipMemcpyAsync(d_base, buf, span, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
            hipEventRecord(ev[next], ctx->stream) != hipSuccess)
            return STORM_HIP_EHIP;
        used[next] = true;
        next = (next + 1) % kBufs;
        return STORM_HIP_OK;
    }
    // Rows of `stride` bytes from d_base, the first `bytes` of each from one host piece, zeros behind (whole rows per
    // chunk: stride <= kBuf).
    int send_rows(uint8_t* d_base, const std::vector<const void*>& rows, size_t bytes, size_t stride) {
        const size_t per_chunk = kBuf / stride;
        std::vector<Piece> chunk;
        for (size_t r0 = 0; r0 < rows.size(); r0 += per_chunk) {
            const size_t n = std::min(per_chunk, rows.size() - r0);
            chunk.clear();
            for (size_t i = 0; i < n; ++i) chunk.push_back({rows[r0 + i], bytes, i * stride, stride - bytes});
            if (int rc = send(d_base + r0 * stride, chunk.data(), n, n * stride)) return rc;
        }
        return STORM_HIP_OK;
    }
    // A run of pieces that is contiguous on the device from d_base (piece i starts where piece i - 1 ended),
    // cut into chunks of at most one buffer. A single piece larger than a buffer is cut as well.
    int send_run(uint8_t* d_base, const std::vector<std::pair<const void*, size_t>>& run) {
        std::vector<Piece> chunk;
        size_t chunk_base = 0, at = 0, fill = 0;
        auto flush = [&]() -> int {
            if (chunk.empty()) return STORM_HIP_OK;
            const int rc = send(d_base + chunk_base, chunk.data(), chunk.size(), fill);
            chunk.clear();
            chunk_base = at;
            fill = 0;
            return rc;
        };
        for (const auto& pc : run) {
            const uint8_t* src = static_cast<const uint8_t*>(pc.first);
            size_t left = pc.second;
            while (left) {
                if (fill == kBuf)
                    if (int rc = flush()) return rc;
                const size_t take = std::min(left, kBuf - fill);
                chunk.push_back({src, take, fill});
                src += take;
                left -= take;
                fill += take;
                at += take;
            }
        }
        return flush();
    }
};

// A host table -> device memory on the context's stream. Small ones as they are (the runtime stages them); from 512 KiB on
// through the pinned ring when the context has one: a large pageable source that is unmapped soon after an asynchronous copy —
// a std::vector freed at the end of a build — made the next wide kernel start 10 - 30 ms late (LAB_NOTES "the late kernel").
inline int upload_bytes(storm_hip_ctx_t* ctx, void* d_dst, const void* h_src, size_t bytes) {
    if (bytes == 0) return STORM_HIP_OK;
    if (bytes < (512u << 10) || !ctx->h_stage_ring)
        return hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, ctx->stream) == hipSuccess ? STORM_HIP_OK : STORM_HIP_EHIP;
    Stager stager(ctx);
    if (int rc = stager.init()) return rc;
    return stager.send_run(static_cast<uint8_t*>(d_dst), {{h_src, bytes}});
}

template <class Rec, class Key>
template <class R>
int WorkList<Rec, Key>::put(storm_hip_ctx_t* ctx, std::optional<Key>&& k, const R* recs, size_t count, const char* what,
                            size_t floor_bytes) {
    forget();
    if (int rc = d.ensure(count * sizeof(R), what, floor_bytes)) return rc;
    if (count) {
        if (int rc = upload_bytes(ctx, d.d, recs, count * sizeof(R))) {
            if (rc == STORM_HIP_EHIP) set_error("%s: the copy to the device failed", what);
            return rc;
        }
        STORM_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    n = (uint32_t)count;
    key = std::move(k);
    return STORM_HIP_OK;
}

// the end of a synchronous call: polls for sync_poll_us, then parks in hipStreamSynchronize (storm_hip_mfma.hip)
hipError_t wait_stream(storm_hip_ctx_t* ctx);

// The one output path of the per-pair matrix calls, whose two forms are one body each: `queued(d, d_ld)` queues the call's
// kernels for a rows x cols matrix of 32-bit entries at d, pitch d_ld. The device form hands it the caller's matrix; the
// host form the context's band buffer at pitch cols (cleared first where the kernels leave entries alone: a triangle's
// i >= j, the lag layout's corner; +0.0f is the same zero bits), which then goes to `out` at pitch ld in one 2-D copy:
// entries [cols, ld) of the caller's rows are never touched. `what` = "<who>: <the buffer>" names the allocation; a wait
// that fails reports "<who>: HIP failure" and has the next K2h launch clear its tickets (a launch that died may have left
// some behind). wait = false: queued only (storm_hip_pairw_matrix_band_begin).
template <typename Queued>
static inline int pair_matrix_out(storm_hip_ctx_t* ctx, const char* what, uint64_t rows, uint64_t cols, void* out, uint64_t ld,
                                  bool host, bool clear, bool wait, Queued&& queued) {
    STORM_HIP_TRY(hipSetDevice(ctx->device));
    uint32_t* d = static_cast<uint32_t*>(out);
    uint32_t* const h_out = host ? d : nullptr;
    if (h_out) {
        const size_t need = (size_t)rows * cols * sizeof(uint32_t);
        if (int rc = ctx->d_band.ensure(need, what)) return rc;
        if (clear) STORM_HIP_TRY(hipMemsetAsync(ctx->d_band, 0, need, ctx->stream));
        d = ctx->d_band;
    }
    if (int rc = queued(d, h_out ? cols : ld)) return rc;
    if (h_out)
        STORM_HIP_TRY(hipMemcpy2DAsync(h_out, ld * sizeof(uint32_t), d, cols * sizeof(uint32_t), cols * sizeof(uint32_t), rows,
                                       hipMemcpyDeviceToHost, ctx->stream));
    if (wait && wait_stream(ctx) != hipSuccess) {
        ctx->tickets_dirty = true;
        set_error("%.*s: HIP failure", (int)strcspn(what, ":"), what);
        return STORM_HIP_EHIP;
    }
    return STORM_HIP_OK;
}


}  // namespace storm

// Pad of a row pitch that is a multiple of 1 KiB, in 512-byte chunks. The bit-operand strips (K2b) read 64-byte
// pieces of 64 consecutive rows: at a power-of-two pitch they fall into a handful of L2 sets and memory channels.
// Measured per pass (profiles/r04_a_pitch_pad.txt, r04_k_pitch_pad.jsonl), pad 0 / 1 / 2 / 4 chunks:
//   10000 rows x  8 KiB (the headline shape)   0.766 / 0.756 / 0.758 / 0.758 ms    (16 and 32 KiB rows: all the same)
//   10000 rows x 64 KiB                        6.57  / 6.22  / 5.97  / 5.99
//   20000 rows x 128 KiB                          -  / 46.1  / 57.9  / 46.0       (2^k + 2^(k-7) bytes is the bad pitch)
// so: one chunk below 64 KiB of pitch (6 % of memory at the headline shape), four from there on.
static inline uint64_t pitch_pad_chunks(int option, uint64_t stride_words) {
    if (option == 0 || stride_words % 128 != 0) return 0;
    return option > 0 ? (uint64_t)option : stride_words >= 8192 ? 4u : 1u;
}

struct storm_hip_matrix_s {
    uint64_t* d = nullptr;
    uint64_t n_rows = 0;        // logical rows
    uint64_t n_rows_pad = 0;    // allocated rows (multiple of kABlockRows)
    uint32_t n_words = 0;       // logical words per row
    uint64_t stride_words = 0;  // allocated words per row (multiple of kChunkWords)
    uint64_t generation = 0;    // changes with every mutation through the library (see "keep_shadow")
    bool sparse_origin = false; // the dense replica of a sparse container (storm_hip_matrix_create_from_blocks): mostly zeros
};

namespace storm {

// what choose_pass reads of a dense matrix
static inline PassShape pass_shape_of(const storm_hip_matrix_s* m, uint32_t shard_count) {
    PassShape s;
    s.n_rows = m->n_rows;
    s.n_rows_pad = m->n_rows_pad;
    s.stride_words = m->stride_words;
    s.n_words = m->n_words;
    s.shard_count = shard_count;
    return s;
}

// ---- what the dosage top-k calls (storm_hip_topk.hip) take from storm_hip_dosage.hip ----
// the refusals the dosage calls share: n_samples that does not fill the rows; the rectangle's NULL arguments, widths that
// differ, ld < b's rows, rows of more than 2^24 values
int check_samples(const char* who, const storm_hip_matrix_s* m, uint64_t n_samples);
int check_square(const char* who, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, const void* out, uint64_t ld);
// the sums of both matrices' rows in the context's row-count scratch, 2 (n_a + n_b) words: A's s and q, then B's; queued
struct SquareSums {
    const uint32_t *a_sum, *a_sq, *b_sum, *b_sq;
};
int dosage_square_sums_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, SquareSums* out);
// The split operands of a matrix with missing genotypes: G, H and M as matrices of rows128 = n_rows up to the next multiple
// of 128 rows each (zero rows behind n_rows), adjacent in that order, so that [G ; H] and [G ; H ; M] are one matrix each.
struct DosageSplit {
    storm_hip_matrix_s g, m, gh, ghm;   // views into the scratch (never destroyed)
    uint64_t rows128;
};
// the splits of both matrices side by side in ctx->d_dosage_rows (one split when b is a: *sb = *sa), queued
int dosage_split_pair_queued(storm_hip_ctx_t* ctx, const storm_hip_matrix_s* a, const storm_hip_matrix_s* b, uint64_t n_samples,
                             DosageSplit* sa, DosageSplit* sb);

}  // namespace storm
