// storm_hip_plan.h — the work lists of the matrix-core kernels (K2*) and of the sparse arena (column layout, K4's items,
// K1's segments over the pool): the records the planners write and the kernels read, the geometry both sides need, and
// the planners themselves (storm_hip_plan.cpp: plain C++, no device, no HIP runtime). storm_hip_internal.h includes this
// header; the planners see nothing of the context.
//
// Every planner takes ONE request struct that holds all it reads besides the row ranges (which travel next to it and
// are part of the request by their hash). The launchers cache an uploaded list under the request it was planned from
// and compare requests for equality, so an option the planner reads cannot be missing from the key.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>

namespace storm {

void set_error(const char* fmt, ...);   // storm_hip.hip
bool timing_env();                      // STORM_HIP_TIMING is set (read once)

// A request is compared bytewise: it must have no padding (every member a 32- or 64-bit integer).
template <class T>
inline bool same_request(const T& a, const T& b) {
    static_assert(std::has_unique_object_representations_v<T>, "a request struct with padding cannot be compared with memcmp");
    return !memcmp(&a, &b, sizeof(T));
}

constexpr int kChunkWords = 64;        // K1's k-chunk, one 64-bit word per lane: a row's stride is a multiple of it

// ---- K2 tiles (pairw_fp4_kernel and the write-mode tile kernels) ----
constexpr int kTile = 256;             // rows per tile side
constexpr int kStageBytes = 64;        // bytes of one row per stage = 128 nibbles = 128 bits of k
constexpr uint32_t kGroupStages = 32;  // multi-GPU ownership unit along k: 32 stages = 64 words

struct MfmaItem {
    uint16_t I, J;       // row-block indices, I <= J
    uint32_t stage0;     // first stage of the k-slice
    uint32_t n_stages;   // stages in this k-slice
};
static_assert(sizeof(MfmaItem) == 12, "read by device code");

// ---- K2s / K2b strips ----
constexpr uint32_t kOwnSlices = 4;                       // strips: k-slices per ownership unit
constexpr int kStripRowBytes = 128;                      // 256 bits of k as nibbles
constexpr int kStripBRows = 64;                          // B rows per stage
constexpr int kStripWaves = 4;                           // waves per workgroup = A tile / 64 rows
constexpr int kStripATile = 64 * kStripWaves;            // A rows per workgroup (256; 8 waves / 512 rows measured slower)
// the third strip form (strip16_rows_kernel: 128 A rows per wave): A tiles of 512 rows, k-slices of 16 bytes = 2 words of every
// row; the 8 slices of a 128-byte line stay on one XCD (kStripRows below holds the form's other numbers)
constexpr uint32_t kStripRowsATile = 512;
constexpr uint32_t kStripRowsXcdGroup = 8;
// ... and the schedule of its diagonal phase (the A tile's 8 blocks of 64 rows among themselves: block b against every
// block d > b whole, against itself as the strict upper triangle). Wave w of the 4 keeps two blocks, its HALVES: the low
// half is block w, the high half block 7 - w, so that every wave owes 7 whole block products and 2 triangles. The wave
// walks the blocks d upwards from its first one; at block d a half skips (d in front of its block), multiplies its own
// triangle (d is its block) or multiplies whole. The kernel takes its loop bounds from these functions and
// tests/strip_rows_diag/driver.cpp checks them on the host.
constexpr uint32_t kStripRowsBlocks = kStripRowsATile / (uint32_t)kStripBRows;   // 8
constexpr uint32_t kStripRowsWaves = 4;
enum StripRowsRole : uint32_t { kStripRowsSkip = 0, kStripRowsOwn = 1, kStripRowsWhole = 2 };
constexpr uint32_t strip_rows_block(uint32_t wave, uint32_t half) { return half ? kStripRowsBlocks - 1u - wave : wave; }
constexpr StripRowsRole strip_rows_role(uint32_t wave, uint32_t half, uint32_t d) {
    return d < strip_rows_block(wave, half) ? kStripRowsSkip : d == strip_rows_block(wave, half) ? kStripRowsOwn : kStripRowsWhole;
}
// the first block at which the wave has anything to multiply, and one past the last
constexpr uint32_t strip_rows_diag_begin(uint32_t wave) {
    return strip_rows_block(wave, 0) < strip_rows_block(wave, 1) ? strip_rows_block(wave, 0) : strip_rows_block(wave, 1);
}
constexpr uint32_t strip_rows_diag_end(uint32_t) { return kStripRowsBlocks; }
// MFMAs of a half at block d: a whole product is 4 x 4 sub-blocks of 16 x 16, an own block the 10 with i <= j
constexpr uint32_t strip_rows_role_mfmas(StripRowsRole r) { return r == kStripRowsWhole ? 16u : r == kStripRowsOwn ? 10u : 0u; }
// (the kernel's five runs — low own | low whole | low whole + high own | both whole, nothing skipped in between — need the
//  low half's block in front of the high half's for every wave)
static_assert(strip_rows_block(0, 0) < strip_rows_block(0, 1) && strip_rows_block(1, 0) < strip_rows_block(1, 1) &&
              strip_rows_block(2, 0) < strip_rows_block(2, 1) && strip_rows_block(3, 0) < strip_rows_block(3, 1),
              "strip16_rows_kernel walks the low half's own block first");

// ... and where the rows end (strip16_rows_kernel's argument n_rows: the r1 of a pass that is one plain range from row 0,
// kStripRowsNoTrim otherwise). The rows from n_rows up to the next multiple of 512 are zero, and the kernel issues no MFMA
// for what is zero in whole units — a 16-row fragment of an item's top B block, a 64-row block of the A tile's own eight:
//   * the top B block j1 - 1 of a run, when only 1 or 2 of its 4 fragments hold a row, becomes the run's LAST stage and
//     multiplies those fragments alone; with 3 or 4 the run is walked as without the argument;
//   * the diagonal phase stops at the tile's last block that holds a row, for both halves of every wave.
// Inside a fragment or a block nothing is trimmed. tests/strip_rows_trim/driver.cpp checks these functions on the host.
constexpr uint32_t kStripRowsNoTrim = 0xFFFFFFFFu;
// fragments of 16 rows of B block `blk` that hold a row below n_rows: 0 .. 4
constexpr uint32_t strip_rows_real_frags(uint32_t blk, uint32_t n_rows) {
    const uint32_t row0 = blk * (uint32_t)kStripBRows;   // (row indices are 32-bit: blk < 2^26)
    return n_rows <= row0 ? 0u : n_rows - row0 >= (uint32_t)kStripBRows ? 4u : (n_rows - row0 + 15u) / 16u;
}
// blocks of 64 rows of the A tile at a_row0 that hold a row below n_rows: 0 .. 8
constexpr uint32_t strip_rows_real_blocks(uint32_t a_row0, uint32_t n_rows) {
    return n_rows <= a_row0 ? 0u : n_rows - a_row0 >= kStripRowsATile ? kStripRowsBlocks
                                                                     : (n_rows - a_row0 + (uint32_t)kStripBRows - 1u) / (uint32_t)kStripBRows;
}
// does the run [j0, j1) end in a block that is multiplied last and in part? (its fragments: strip_rows_real_frags(j1 - 1))
constexpr bool strip_rows_top_trimmed(uint32_t j0, uint32_t j1, uint32_t n_rows) {
    return j1 > j0 && strip_rows_real_frags(j1 - 1u, n_rows) - 1u < 2u;
}
// MFMAs the four waves of an item issue: a stage is 4 fragments x 8 A fragments per wave, the diagonal phase the roles
// above at the blocks d < nb of the halves whose own block lies below nb
constexpr uint32_t strip_rows_item_mfmas(uint32_t a_row0, uint32_t diag, uint32_t j0, uint32_t j1, uint32_t n_rows) {
    const uint32_t T = j1 - j0;
    uint32_t n = strip_rows_top_trimmed(j0, j1, n_rows)
                     ? kStripRowsWaves * 8u * (4u * (T - 1u) + strip_rows_real_frags(j1 - 1u, n_rows))
                     : kStripRowsWaves * 8u * 4u * T;
    if (diag) {
        const uint32_t nb = strip_rows_real_blocks(a_row0, n_rows);
        for (uint32_t w = 0; w < kStripRowsWaves; ++w)
            for (uint32_t half = 0; half < 2u; ++half)
                for (uint32_t d = 0; d < nb; ++d)
                    if (strip_rows_block(w, half) < nb) n += strip_rows_role_mfmas(strip_rows_role(w, half, d));
    }
    return n;
}

struct StripItem {
    uint32_t a_row0;  // first row of the A tile (kStripATile rows, multiple of 64)
    uint32_t diag;    // 1: the item starts with the stages of its own tile (strict upper part)
    uint32_t j0, j1;  // then the later B stages: 64-row blocks [j0, j1), walked downwards
    uint32_t ks;      // k-slice index (128 bytes of the nibble rows each)
};
static_assert(sizeof(StripItem) == 20, "read by device code");

// ---- the scheduling model of the 128-rows-per-wave form ----
// What one XCD makes of its list, in STAGE units (the time a compute unit's matrix pipe takes for one stage of one
// workgroup: 128 MFMAs). The XCD has n_cus compute units of slots_per_cu workgroup slots. It hands its list out in order:
// an item goes to a free slot as soon as there is one, on the compute unit that holds the fewest workgroups (the lowest
// index among equals). A workgroup first waits start_latency without using the pipe (its launch, the A rows, the first
// images), then has work; a compute unit's pipe does one stage per unit of time, shared equally among its workgroups that
// have work. The answer is the time at which the last item ends, counted from `t0`, the time at which every slot is free.
// tests/strip_rows_tail/driver.cpp checks it against schedules worked out by hand.
constexpr double kStripRowsStageMfmas = 128.0;   // 4 waves x 4 fragments x 8 A fragments
inline double strip_rows_item_cost(const StripItem& it, uint32_t n_rows) {   // trims and the resident diagonal included
    return (double)strip_rows_item_mfmas(it.a_row0, it.diag, it.j0, it.j1, n_rows) / kStripRowsStageMfmas;
}
inline double strip_rows_makespan(const double* cost, size_t n_items, uint32_t n_cus, uint32_t slots_per_cu, double start_latency,
                                  double t0 = 0.0, const double* resident = nullptr) {
    // resident (may be NULL; n_cus x slots_per_cu, a compute unit's slots together): work that the slots still hold at t0
    // from what ran before the list (0: the slot is free) — the middle of a launch instead of its start
    if (n_cus == 0 || slots_per_cu == 0 || (n_items == 0 && !resident)) return t0;
    constexpr double kNever = 1e300, kDone = 1e-9;
    const size_t n_slots = (size_t)n_cus * slots_per_cu;
    // per slot: the work left (< 0: free) and the time from which the workgroup works; per compute unit: the time up to
    // which `left` is accounted, the time at which its next workgroup ends, the groups it holds
    std::vector<double> left(n_slots, -1.0), ready(n_slots, t0), last(n_cus, t0), next(n_cus, kNever), tmp(slots_per_cu);
    std::vector<uint32_t> held(n_cus, 0u);
    // One step of a compute unit's own time line from `cur`, over the work `l`: up to `until`, or to the next start of a
    // waiting group if that comes first; the pipe's work in between comes off the working groups in equal shares. Returns
    // the time reached and says through `end` when the first working group would end if nothing started before.
    auto step = [&](const double* r, double* l, double cur, double until, double* end) {
        uint32_t working = 0;
        double wake = kNever, least = kNever;
        for (uint32_t s = 0; s < slots_per_cu; ++s) {
            if (l[s] < 0.0) continue;
            if (r[s] <= cur) {
                ++working;
                if (l[s] < least) least = l[s];
            } else if (r[s] < wake)
                wake = r[s];
        }
        *end = working ? cur + least * (double)working : kNever;
        const double to = wake < until ? wake : until;
        if (working && to > cur && to < kNever) {
            const double each = (to - cur) / (double)working;
            for (uint32_t s = 0; s < slots_per_cu; ++s)
                if (l[s] >= 0.0 && r[s] <= cur) l[s] = l[s] > each ? l[s] - each : 0.0;   // (never below 0: that marks a free slot)
        }
        return to;
    };
    // bring compute unit c to time t (no later than its next end)
    auto advance = [&](uint32_t c, double t) {
        double end;
        for (double cur = last[c]; cur < t;) cur = step(&ready[(size_t)c * slots_per_cu], &left[(size_t)c * slots_per_cu], cur, t, &end);
        last[c] = t;
    };
    // when its next workgroup ends: its time line walked ahead on a copy, through the starts of its waiting groups
    auto next_end = [&](uint32_t c) {
        const double* r = &ready[(size_t)c * slots_per_cu];
        for (uint32_t s = 0; s < slots_per_cu; ++s) tmp[s] = left[(size_t)c * slots_per_cu + s];
        for (double cur = last[c];;) {
            double end;
            const double to = step(r, tmp.data(), cur, kNever, &end);
            if (end <= to) return end;   // (also: nothing held, both never)
            cur = to;
        }
    };
    uint32_t free_slots = (uint32_t)n_slots;
    if (resident)
        for (uint32_t c = 0; c < n_cus; ++c) {
            for (uint32_t s = 0; s < slots_per_cu; ++s)
                if (resident[(size_t)c * slots_per_cu + s] > kDone) {
                    left[(size_t)c * slots_per_cu + s] = resident[(size_t)c * slots_per_cu + s];
                    ++held[c];
                    --free_slots;
                }
            next[c] = next_end(c);
        }
    size_t k = 0;
    double now = t0;
    constexpr uint32_t kNone = ~0u;
    uint32_t only = kNone;   // the one compute unit that has free slots, where that is known
    // the groups of compute unit c that end at `now` leave
    auto let_go = [&](uint32_t c) {
        advance(c, now);
        double* l = &left[(size_t)c * slots_per_cu];
        uint32_t gone = 0;
        for (uint32_t s = 0; s < slots_per_cu; ++s)
            if (l[s] >= 0.0 && l[s] <= kDone && ready[(size_t)c * slots_per_cu + s] <= now) {
                l[s] = -1.0;
                ++gone;
            }
        held[c] -= gone;
        free_slots += gone;
        return gone;
    };
    for (;;) {
        while (k < n_items && free_slots) {   // hand out: the emptiest compute unit first
            uint32_t c = only != kNone ? only : 0u;
            if (only == kNone)
                for (uint32_t i = 1; i < n_cus; ++i)
                    if (held[i] < held[c]) c = i;
            advance(c, now);
            double* l = &left[(size_t)c * slots_per_cu];
            uint32_t s = 0;
            while (l[s] >= 0.0) ++s;
            l[s] = cost[k] > kDone ? cost[k] : 2.0 * kDone;   // (an item of no work still takes its start)
            ++k;
            ready[(size_t)c * slots_per_cu + s] = now + start_latency;
            ++held[c];
            --free_slots;
            next[c] = next_end(c);
        }
        only = kNone;
        uint32_t first = 0, ties = 1;
        for (uint32_t i = 1; i < n_cus; ++i)
            if (next[i] < next[first]) {
                first = i;
                ties = 1;
            } else
                ties += next[i] == next[first];
        if (next[first] >= kNever) return now;   // nothing is held and nothing is left
        now = next[first];
        // every group that ends at this time leaves before the next item is handed out
        if (ties == 1) {
            // (items left: every slot was taken, the free ones are all here, and this unit's next end is found when it has them)
            if (let_go(first) && k < n_items)
                only = first;
            else
                next[first] = next_end(first);
            continue;
        }
        for (uint32_t c = first; c < n_cus; ++c)
            if (next[c] <= now) {
                let_go(c);
                next[c] = next_end(c);
            }
    }
}
inline double strip_rows_makespan(const StripItem* list, size_t n_items, uint32_t n_rows, uint32_t n_cus, uint32_t slots_per_cu,
                                  double start_latency) {
    std::vector<double> cost(n_items);
    for (size_t k = 0; k < n_items; ++k) cost[k] = strip_rows_item_cost(list[k], n_rows);
    return strip_rows_makespan(cost.data(), n_items, n_cus, slots_per_cu, start_latency);
}

// ---- K2q (bitstream_kernel) ----
struct BitSeg {
    uint32_t a_blk;     // first 64-row block of the A tile (4 blocks; absolute block index)
    uint32_t ks;        // k-slice: 64 bytes of every bit row
    uint32_t b_first;   // first later block, relative to range_b0, cyclic over range_nb
    uint32_t n_b;       // later blocks = stages behind the tile's own four
    uint32_t range_b0;  // first block of the all-pairs problem (row range) the tile belongs to
    uint32_t range_nb;  // blocks of that problem: the cyclic order wraps here
    uint32_t flags;     // bit 0: the tile's own four stages are multiplied (else they only bring A in); bits 8-9: rotation
    uint32_t pad;
};
static_assert(sizeof(BitSeg) == 32, "read by device code");
constexpr uint32_t kBsDiag = 1u;
constexpr uint32_t kBsMaxStages = 8192;      // per workgroup: accumulators stay below 2^22 (in halves: 2^23)

// ---- K2h (tile128_kernel) ----
constexpr uint32_t kThTile = 128u;
struct PartItem {
    uint16_t I, J;               // tile indices in units of 128 (virtual) rows
    uint32_t stage0, n_stages;   // the item's k range in 128-bit stages (multiples of 4)
    uint32_t tile;               // the tile's index among the launch's tiles: its ticket
    uint32_t win0;               // the first of the tile's n_parts windows in `parts` (part p: win0 + p)
    uint16_t part, n_parts;      // this item is part `part` of `n_parts` of its tile; bit 15 of `part`: the tile's windows hold
                                 // 16-bit counts (every part of the tile covers fewer than 2^16 bits of k)
};
static_assert(sizeof(PartItem) == 24, "read by device code");
constexpr uint16_t kThNarrow = 0x8000u;
constexpr uint32_t kThWeightBits = 512u;           // 512 products of 1
constexpr uint32_t kThWeightDosage = 9u * 256u;    // 256 products of two values 0 .. 3

// A "range" is a run of rows [r0, r1) that forms one all-pairs problem: the whole matrix for the dense container, one
// block column of the pool for the sparse one. r0 is a multiple of the A tile (256 rows; 512 for the wide strips) and
// the rows from r1 up to the next multiple of it are zero.
struct RowRange {
    uint64_t r0, r1;     // rows [r0, r1) form one all-pairs problem; r0 is a multiple of the A tile (256; 512 for wide strips)
    uint64_t a_end = 0;  // 0: the whole triangle. Otherwise only the pairs with the EARLIER row below a_end (a
                         // multiple of the A tile from r0, or >= r1): the rows [r0, a_end) among themselves and
                         // against everything behind them — a block column's bitmap rows, with its list rows,
                         // which the list-probe kernel pairs with each other, behind them
    uint64_t back_from = ~0ull;  // != ~0: a row PANEL [back_from, r1) that has just arrived (a multiple of the A tile): only the
                                 // pairs whose LATER row lies in the panel — every A tile of the panel against all the blocks in
                                 // front of it (from r0) plus its own triangle (popcount(a & b) is symmetric: the new rows are the
                                 // stationary operand, the rows already there stream past in long runs)
};
uint64_t ranges_hash(const std::vector<RowRange>& ranges);

// Ownership of the strip work among shard_count shards (multi-GPU ranks; reference loop being
// sharded: storm.c:1199-1238). Two levels:
//   * whole k-slices (256 bits of every row), in units of 4 (1024 bits = one 128-byte line of the bit
//     matrix, so that a shard's expansion reads whole lines): the first (n_units / G) * G units go
//     to shard unit % G, so a shard expands and multiplies only its own columns — 1/G of the O(N*M)
//     expansion and of the pair work, equal shares whatever N is;
//   * the remaining slices ("leftover", fewer than 4 G) are cut along the PAIR space: their items
//     (A tile x run of B blocks) are dealt to the shards longest-first onto the least loaded one
//     (deterministic, every shard computes the same deal), every shard expands those few slices.
// Hence any G balances to within one short item per leftover slice (c2 at G = 3: 85 1/3 slices
// each), and a matrix with fewer slices than shards (M <= 256 * G bits) still splits G ways.
inline uint32_t strip_modulo_slices(uint32_t n_kslices, uint32_t shard_count) {
    return n_kslices / kOwnSlices / shard_count * shard_count * kOwnSlices;  // whole units, a multiple of G
}
inline bool strip_owns_slice(uint32_t ks, uint32_t shard_rank, uint32_t shard_count) {
    return (ks / kOwnSlices) % shard_count == shard_rank;
}

// ---- the summing tile kernel's list (pairw_fp4_kernel) ----
struct TileSumRequest {
    uint64_t ranges_hash;
    uint32_t total_stages, shard_rank, shard_count;
    uint32_t stages_per_item;   // option k2_stages_per_item
    uint32_t diag_only;
    uint32_t one_tile_probe;    // k2_debug & 3 == 1, timing probe only: every item reads one tile
    bool operator==(const TileSumRequest& o) const { return same_request(*this, o); }
};
int plan_tile_sum(const TileSumRequest& rq, const std::vector<RowRange>& ranges, std::vector<MfmaItem>& items);

// ---- strips ----
// The options a strip list is shaped by (context options of the same names), as the caller states them: max_run 0 = the
// run length is chosen by the list-scheduling estimate.
struct StripOptions {
    int32_t max_run = 0, tail_run = 32, tail_slices = 3, lpt_rounds = 6;   // the context's defaults (storm_hip_internal.h)
    int32_t shard_pairs = 0;
    int32_t n_cus = 256;
    int32_t xcd_group = 1;         // consecutive slices that share an XCD (2 for the bit-operand strips: slices 2j, 2j + 1 read the same bits)
    int32_t persistent = 0;        // k2_persistent: one contiguous queue per XCD
    int32_t one_slice_probe = 0;   // k2_debug & 16 (timing probe, wrong results): every XCD re-reads one k-slice
    int32_t rows_form = 0;         // the list is strip16_rows_kernel's (128 A rows per wave): its items cost what strip_rows_item_mfmas counts
    int32_t tail_auto = 0;         // the caller has set neither tail_run nor tail_slices: for one device's whole pass of the rows form
                                   // they are chosen with the run length (kStripRowsShapings), otherwise they hold as they stand
};
// The shaping a list was cut with: what the automatic choices came to, the caller's values where there was no choice.
struct StripChoice {
    int max_run = 0, tail_run = 0, tail_slices = 0;
};
// The candidates of the rows form's automatic choice next to the shaping the pass always had (the run length chosen as
// for every form, the last 3 slices in runs of 32): the three run lengths with a long tail of the same runs and with a
// tail of shorter runs. One is taken only where the model (strip_rows_makespan) has it at least 0.5 % shorter than the
// choice so far. With a run length the caller has set, the two tails are tried on that run length.
constexpr StripChoice kStripRowsShapings[6] = {{96, 32, 12}, {96, 24, 8}, {64, 32, 12}, {64, 24, 8}, {128, 32, 12}, {128, 24, 8}};
// A workgroup's start in stage units (strip_rows_makespan's start_latency): about 1.8 us at the 0.23 us a stage takes when
// a compute unit's pipe is busy — the launch of a workgroup, its A rows and the first two images. Not fitted to a device.
constexpr double kStripRowsStartStages = 8.0;
struct StripRequest {
    StripOptions opt;
    uint32_t n_kslices, shard_rank, shard_count, a_tile;
    uint32_t unused = 0;   // (no padding in front of the 64-bit member: same_request)
    uint64_t ranges_hash;
    bool operator==(const StripRequest& o) const { return same_request(*this, o); }
};
StripRequest strip_request(const StripOptions& opt, const std::vector<RowRange>& ranges, uint32_t n_kslices,
                           uint32_t shard_rank, uint32_t shard_count, uint32_t a_tile);
// The list in launch order and, for the persistent form, the per-XCD queue bounds; chosen: the shaping in use.
void plan_strips(const StripRequest& rq, const std::vector<RowRange>& ranges, std::vector<StripItem>& items,
                 uint32_t queue_base[8], uint32_t queue_count[8], StripChoice* chosen = nullptr);

// ---- how an all-pairs pass chooses its form ----
// One record per strip form: the ONLY place where a form's numbers are written down. The launchers, the panels of
// storm_hip_pairw_dense_upload, the sparse pass and storm_hip_strip_plan3 read them from here.
enum class StripKernel : uint32_t { Fp4, Bits, BitsWide, Rows };
struct StripForm {
    StripKernel kernel;          // strip16_fp4_kernel | strip16_bits_kernel | strip16_bits2_kernel | strip16_rows_kernel
    uint32_t a_tile;             // A rows per workgroup: the rows up to the next multiple of it must exist and be zero
    uint32_t waves;              // a workgroup is 64 x waves threads
    uint32_t chunk_words;        // a row's words are taken in chunks of this many ...
    uint32_t slices_per_chunk;   // ... of this many k-slices each (bits: the two class pairs of a 512-bit chunk)
    int32_t xcd_group;           // consecutive slices that share an XCD
    uint64_t wave_sum_max;       // the most a wave adds to a slot (the fold inside the launch): A rows per wave x
                                 // (4096 stages x 64 + the tile's own) rows x bits per slice; 0: the form never folds inline
    int32_t operands_report;     // k2_operands_used
    int32_t rows_report;         // k2_strip_rows_used; 0: not a K2b form
    int32_t plan_form;           // storm_hip_strip_plan3's `form`; -1: none
    constexpr uint32_t threads() const { return 64u * waves; }
    constexpr uint32_t chunks(uint32_t n_words) const { return (n_words + chunk_words - 1u) / chunk_words; }
    constexpr uint32_t kslices(uint32_t n_words) const { return slices_per_chunk * chunks(n_words); }   // slices that hold data
    constexpr uint32_t slice_words() const { return chunk_words / slices_per_chunk; }                   // the pass report's unit
    constexpr bool rows_form() const { return kernel == StripKernel::Rows; }
};
constexpr StripForm kStripFp4 = {StripKernel::Fp4, (uint32_t)kStripATile, (uint32_t)kStripWaves, 4u, 1u, 1, 0ull, 4, 0, 0};
constexpr StripForm kStripBits = {StripKernel::Bits, (uint32_t)kStripATile, (uint32_t)kStripWaves, 8u, 2u, 2,
                                  64ull * (4096ull * 64ull + 256ull) * 256ull, 5, 64, 1};
constexpr StripForm kStripBitsWide = {StripKernel::BitsWide, 512u, 8u, 8u, 2u, 2, kStripBits.wave_sum_max, 6, 64, -1};
constexpr StripForm kStripRows = {StripKernel::Rows, kStripRowsATile, kStripRowsWaves, 2u, 1u, (int32_t)kStripRowsXcdGroup,
                                  128ull * (4096ull * 64ull + 512ull) * 128ull, 5, 128, 2};
static_assert(kStripRows.kslices(1023) == 512u && kStripBits.kslices(1024) == 256u && kStripFp4.kslices(5) == 2u, "slices that hold data");
static_assert(kStripBits.slice_words() == 4u && kStripRows.slice_words() == 2u, "a slice is 256 bit-MACs per pair, the rows form's 128");
constexpr const StripForm* strip_form_of_plan(int form) {   // storm_hip_strip_plan3's forms 0 / 1 / 2
    return form == kStripFp4.plan_form ? &kStripFp4 : form == kStripBits.plan_form ? &kStripBits
         : form == kStripRows.plan_form ? &kStripRows : nullptr;
}

// Which kernel an all-pairs pass runs, on which form: ONE pure function of the selecting options, the shape and the
// caller (storm_hip_plan.cpp, with the measurements behind its rules). Every pass asks it once and switches on the answer.
constexpr int kStripRingDefault = 4;
enum class PassCaller : uint32_t { Dense, DenseUpload, SparsePool };
enum class PassKernel : uint32_t {
    Popcount,        // K1
    Fp4Tiles,        // pairw_fp4_kernel over the FP4 shadow (variant 3)
    Fp4Strips,       // the FP4 strips, 256-row A tiles (also where the bit operands cannot run: the chunked shadow path)
    Fp4StripsWide,   // ... 512-row A tiles (variant 5)
    Bitstream,       // K2q
    Strips,          // K2b: `form` says which
    ToolsStripBits,  // k2_strip_operands 1 (stripbits_kernel): tools build; the shipped library refuses at the launch
    ToolsBitwave,    // k2_strip_operands 3 (K2w): tools build
};
struct PassOptions {   // context options of the same names
    int32_t variant, k2_strip_operands, k2_strip_rows, k2_ring, k2_shape, k2_persistent, k2_debug;
    bool tools_build;
};
struct PassShape {
    uint64_t n_rows = 0, n_rows_pad = 0, stride_words = 0;   // dense and dense-upload: the matrix
    uint32_t n_words = 0, shard_count = 1;
    // sparse pool: the pool rows the matrix cores multiply up to the next multiple of 512, the rows the pool holds, and
    // the widest block column (variant -1 decides by it)
    uint64_t rows_dst = 0, pool_rows_ready = 0, widest = 0;
};
struct PassChoice {
    PassKernel kernel;
    const StripForm* form;   // Strips: the form; NULL otherwise
    int32_t variant_used;
    int32_t operands_used;   // k2_operands_used; 0: the pass does not write it (popcount, the pool's FP4 paths)
    int32_t strip_mode;      // launch_pairw_mfma_ranges' (the FP4 kernels): 0 tiles, 1 strips, 2 wide strips
    bool in_panels;          // dense-upload: the pass runs panel by panel behind the copies (always kStripBits, runs of
                             // 128); false: the copy, then the dense pass, which the other members describe
};
PassChoice choose_pass(PassCaller caller, const PassOptions& o, const PassShape& s);

// ---- write-mode tiles of 256 x 256 ----
// Launch order of the tiles [i0, i1) x [j0, j1) (upper triangle only when `triangle`) for L2 reuse: appended to `out`.
void xcd_grouped_tiles(uint32_t i0, uint32_t i1, uint32_t j0, uint32_t j1, bool triangle,
                       std::vector<std::pair<uint16_t, uint16_t>>& out);
struct MatrixTilesRequest {
    std::vector<std::pair<uint16_t, uint16_t>> tiles;   // in launch order
    std::vector<float> cost;    // empty, or one per tile (1 = a full tile): what the planner assumes when it cuts the last round
    uint32_t total_stages = 0;
    uint32_t n_cus = 1;
    int32_t split = 1;          // option k2_matrix_split
    int32_t min_part = 32;      // option k2_matrix_min_part
    bool operator==(const MatrixTilesRequest& o) const {
        return total_stages == o.total_stages && n_cus == o.n_cus && split == o.split && min_part == o.min_part &&
               tiles == o.tiles && cost == o.cost;
    }
};
struct MatrixPlan {  // item table of one matrix-output launch
    uint32_t n_items = 0;  // workgroups to launch
    uint32_t n_full = 0;   // items [0, n_full) are whole tiles; the rest are k-parts that add into a cleared window
    uint32_t n_cut = 0;    // tiles that are cut into parts: behind the items the table holds one record per such tile
                           // (what zero_tiles_kernel walks: one workgroup column per window, not one per part)
};
void plan_matrix_tiles(const MatrixTilesRequest& rq, std::vector<MfmaItem>& items, MatrixPlan* plan);

// ---- K2h ----
struct Tile128Request {
    uint32_t ia0, ia1, jb0, jb1;   // tiles of 128 rows: A [ia0, ia1) x B [jb0, jb1)
    uint32_t triangle;
    uint32_t total_stages;
    uint32_t n_cus;
    int32_t slots_per_cu, min_chunks, diag_cost_pct;   // options k2_part_slots, k2_part_min_chunks, k2_part_cost_diag
    uint32_t narrow_windows;                           // option k2_part_narrow
    uint32_t lag;   // 0: none. Triangle only: just the tiles that hold a pair i < j with j - i <= lag (the lag layout's list)
    uint32_t chunk_weight;   // the most one 512-bit chunk adds to an accumulator: kThWeightBits, or kThWeightDosage for rows of
                             // 2-bit values. An item stays at chunks x weight <= 2^24 (f32 accumulators), a narrow window's
                             // part at <= 65535
    bool operator==(const Tile128Request& o) const { return same_request(*this, o); }
};
struct Tile128Plan {
    std::vector<PartItem> items;
    uint32_t n_tiles = 0, n_windows = 0;
};
void plan_tile128(const Tile128Request& rq, Tile128Plan* plan);

// ---- K2q ----
struct BitstreamShaping {
    int32_t groups_per_cu = 0;  // 0 = by the length of the stream: 1, 2 or 3
    int32_t min_piece = 6;      // stages a workgroup should have at least before a CU's share is cut further
    int32_t min_run = 2;        // a cut leaves at least this many later blocks on either side of it
    int32_t long_piece = 80;    // stages per workgroup once the stream is longer than the chip's slots x this
    // one round of 3 workgroups per CU: the later workgroups' shares in percent of the first one's (build_bitstream) ...
    int32_t w3_1 = 120, w3_2 = 60;
    int32_t weighted_min = 16;       // ... from this many stages per share (shorter ones: equal shares)
    int32_t single_round_max = 220;  // stages per slot up to which the stream is ONE round of weighted shares
};
struct BitstreamRequest {
    BitstreamShaping sh;
    uint32_t n_kslices, shard_rank, shard_count, n_cus;
    uint64_t pitch_bytes;
    uint64_t ranges_hash;
    bool operator==(const BitstreamRequest& o) const { return same_request(*this, o); }
};
struct BitstreamPlan {
    std::vector<BitSeg> segs;
    std::vector<uint32_t> bases;        // per stage, workgroup by workgroup: where its 64 rows x 64 B start (64-byte units)
    std::vector<uint32_t> first_stage;  // workgroup w's stages are bases[first_stage[w] .. first_stage[w + 1])
    std::vector<uint32_t> first;
    uint32_t groups = 0;
    uint64_t stages = 0;      // multiplied + operand-only stages of this shard, after cutting
    uint32_t max_stages = 0;  // longest workgroup
};
BitstreamRequest bitstream_request(const BitstreamShaping& sh, const std::vector<RowRange>& ranges, uint32_t n_kslices,
                                   uint32_t shard_rank, uint32_t shard_count, uint32_t n_cus, uint64_t pitch_bytes);
void build_bitstream(const BitstreamRequest& rq, const std::vector<RowRange>& ranges, BitstreamPlan& plan);

// ---- the sparse arena (storm_hip_sparse.hip): block-column layout, K4's work lists, K1's segments ----
constexpr uint32_t kBlockWords = 1024;      // 65536 bits
constexpr uint32_t kMaxBlockId = 65536;     // uint32 positions / 65536 bits per block
constexpr int kABlockRows = 128;            // K1: A rows per workgroup (storm_hip_internal.h: kWaves * kRowsPerWave)
// (256 rows x 4096 positions — half the passes over the elements, two 16-byte reads per lookup — is slower:
//  4.57 against 3.67 ms at c4's 20971 draws; the LDS reads are the larger half of the time)
constexpr uint32_t kProbeRows = 128;        // A rows per item
constexpr uint32_t kProbeOctBits = 13;      // positions per table: 2^13 of the block's 2^16 (table = 2^13 x 16 B)
constexpr uint32_t kProbeOctants = 1u << (16 - kProbeOctBits);
constexpr uint32_t kFatGroups = 4;          // groups per workgroup of probe_lists_fat_kernel

struct Seg {            // one (A block, B row range) segment of the upper triangle (K1)
    uint32_t a_row0;    // first A row of the block (kABlockRows rows are loaded from here)
    uint32_t a_end;     // A rows >= a_end are treated as all-zero (block-column / matrix edge)
    uint32_t j_lo;      // B rows [j_lo, j_hi)
    uint32_t j_hi;      // j_lo == a_row0 marks a diagonal segment: count only pairs i < j
};
static_assert(sizeof(Seg) == 16, "read by device code");

struct ProbeItem {            // probe_lists_kernel: one group of kProbeRows rows x one octant x one chunk of the far stream
    uint32_t a_begin, a_end;  // elements of the A rows [a0, a0 + 128) in this octant
    uint32_t n_begin, n_end;  // "near" elements: the A rows' own (row-tagged, masked); first chunk only
    uint32_t b_begin, b_end;  // chunk of the elements of the rows behind the group (positions only)
    uint32_t a0;              // first A row (row index within the column)
};
static_assert(sizeof(ProbeItem) == 28, "read by device code");
struct ProbeFatItem {              // probe_lists_fat_kernel: a bundle of kFatGroups consecutive groups
    uint32_t at[kFatGroups + 1];   // elements of group k of the bundle in this octant: [at[k], at[k + 1])
    uint32_t b_begin, b_end;       // chunk of the elements of the rows behind the bundle
    uint32_t first;                // 1: the bundle's own pairs (inside and between its groups) belong to this item
};
static_assert(sizeof(ProbeFatItem) == 32, "read by device code");
struct ProbeRegion { uint32_t e_begin, e_end, pool_row0, octant; };   // expand_probe_kernel: four uint32 per region
static_assert(sizeof(ProbeRegion) == 16, "read by device code");

// The flat block description of storm_hip.h: rows -> blocks (CSR), per block its column id, kind (0 list, 1 bitmap),
// list length and data.
struct ArenaBlocks {
    uint64_t n_rows = 0, n_blocks = 0;
    const uint64_t* row_block_offset = nullptr;
    const uint32_t* block_id = nullptr;
    const uint8_t* block_kind = nullptr;
    const uint32_t* block_n = nullptr;
    const void* const* block_ptr = nullptr;
};

// STORM_HIP_TIMING: the host time since the last lap, to stderr
struct ArenaLaps {
    int64_t t0_ns;
    ArenaLaps();
    void lap(const char* what);
};

// What the arena keeps of its column layout.
struct ArenaColumns {
    std::vector<RowRange> cols;      // pool-row range [r0, r1) of each non-empty column; every r0
                                     // is a multiple of 512 and the gap up to it is zero rows
    uint64_t census[4] = {0, 0, 0, 0};
    uint64_t n_pool_rows = 0;        // rows of the whole layout: columns the list-probe kernel cannot take first, ...
    uint64_t pool_rows_ready = 0;    // ... and only those exist until a dense pass over a probe column is asked for
    // list-probe path (K4): columns whose blocks are all short lists
    std::vector<uint64_t> col_list0; // per entry of `cols`: first pool row of the column's LIST blocks (its bitmap
                                     // blocks come first, the lists on the next multiple of 512 rows)
    std::vector<uint8_t> col_probe;  // per entry of `cols`: 1 = has probe data (its list blocks among themselves)
    std::vector<uint32_t> col_avg_len;  // per entry of `cols`: mean list length (probe columns)
};
// ... and what only the build reads: the pool row of every block (rows are visited in order => row order inside a column)
struct ArenaRows {
    std::vector<uint32_t> list_row, list_len, dense_row;   // list blocks that own a pool row (and are not empty); bitmap blocks
    std::vector<uint64_t> list_blk, dense_blk;             // the blocks behind those rows
    std::vector<uint64_t> probe_blocks;                    // the list blocks of probe columns, in row order
    std::vector<int64_t> col_entry;                        // column id -> index into `cols` (-1: no block), ids 0 .. max id + 1
};
// Validates the description (the texts and codes of storm_hip_sparse_create*) and lays the block columns out.
int plan_arena_columns(const ArenaBlocks& in, ArenaColumns* cols, ArenaRows* rows, ArenaLaps& laps);

// K4's work: what the arena keeps ...
struct ProbeWork {
    std::vector<ProbeRegion> probe_regions;  // (column, octant) element ranges: how ensure_full_pool expands the lists
    // both lists hold the same work for all eligible columns, in launch order (family by family on 8 queues); *_col: the
    // item's entry of `cols`, by which a launch filters them
    std::vector<ProbeItem> items;          // one group per workgroup (probe_lists_kernel)
    std::vector<uint32_t> item_col;
    std::vector<ProbeFatItem> fat_items;   // [r6] bundles of kFatGroups groups (probe_lists_fat_kernel)
    std::vector<uint32_t> fat_col;
};
// ... and where the build's kernels put the elements
struct ProbeLayout {
    size_t n_probe_elems = 0;
    std::vector<uint32_t> run_dst;       // per probe block and octant: where the octant's run starts in the element arrays
    std::vector<uint32_t> block_local;   // the block's row inside its column's list rows
    std::vector<uint32_t> atoms;         // {first element, end} of every atom of the far stream
};
// run_end: per probe block and octant, the end of the octant's run inside the list (probe_run_end_kernel).
int plan_arena_probe(const ArenaBlocks& in, const ArenaColumns& cols, const ArenaRows& rows, const std::vector<uint32_t>& run_end,
                     ProbeWork* work, ProbeLayout* layout, ArenaLaps& laps);

// One launch of K4: this shard's view of the items of the columns in use.
struct ProbeLaunchRequest {
    uint32_t shard_rank = 0, shard_count = 0;
    int32_t bundle = 0;                  // 1: ProbeWork::items (probe_lists_kernel), kFatGroups: fat_items
    std::vector<uint8_t> use_probe;      // per entry of `cols`
    bool operator==(const ProbeLaunchRequest& o) const {
        return shard_rank == o.shard_rank && shard_count == o.shard_count && bundle == o.bundle && use_probe == o.use_probe;
    }
};
struct ProbeLaunchPlan {
    std::vector<ProbeItem> mine;         // the records to upload: one of the two lists is filled
    std::vector<ProbeFatItem> fat;
    uint32_t n_probe_launch = 0, n_probe_cols_launch = 0;
    uint64_t probe_lookups_launch = 0;   // positions the launched items stream + their own rows' elements (this shard)
};
void plan_probe_launch(const ProbeWork& work, const ProbeLaunchRequest& rq, ProbeLaunchPlan* plan);

// K1 over the pool: the upper triangle of every block column; shard = every shard_count-th segment.
void plan_sparse_segments(const std::vector<RowRange>& cols, uint32_t seg_len, uint32_t shard_rank, uint32_t shard_count,
                          std::vector<Seg>* mine, uint64_t* seg_row_sum);

// ---- the block stage's list space (storm_hip_sparse.hip: storm_hip_stage_add_list and the staged builders) ----
// The staged lists are one byte stream: position p = list chunk p / kStageListChunk, offset p % kStageListChunk. They
// leave the host in buffers of at most kStageListBuf bytes, one copy each, so a buffer — and with it every list — lies
// inside ONE chunk: a list that would run across a chunk's end starts the next chunk instead, and the bytes between
// the last list of a chunk and the chunk's end (the gap) are never written. A list's token is its position.
constexpr uint64_t kStageListBuf = 4u << 20, kStageListChunk = 64u << 20;
constexpr uint32_t kStageMaxList = 65536;   // positions of a list block at most
struct StageListPlace {
    uint64_t lbase;   // where the current buffer starts once the list is in it
    uint64_t token;   // the list's position
    uint32_t send;    // 1: the current buffer [lbase, lbase + lfill) leaves first
    uint32_t pad = 0;
};
// Where a list of n positions (1 .. kStageMaxList) goes when the current buffer starts at lbase and holds lfill bytes.
StageListPlace stage_place_list(uint64_t lbase, uint32_t lfill, uint32_t n);
// written[c] = the bytes of list chunk c that hold lists (they lie back to back from the chunk's start): the record
// stage_list_readable answers from. Called for every list placed, in order.
void stage_note_list(std::vector<uint64_t>* written, uint64_t token, uint32_t n);
// Do all 2 n bytes at `token` lie inside bytes the stage wrote, within one chunk? No for an odd token, a token beyond the
// stage, a token in a gap and a list that would run across its chunk's end or past what the chunk holds. (A token that
// points into the middle of a staged list is in bounds: yes.)
bool stage_list_readable(const std::vector<uint64_t>& written, uint64_t token, uint64_t n);

// ---- the row panels of the dosage top-k calls (storm_hip_topk.hip: dosage_topk_queued) ----
// A panel's planes hold `plane_words_per_row` uint32 per panel row: dosage_topk_plane_words — the plain form's one plane of
// ld = n_b up to the next multiple of 4 words; the complete form's P, the two planes G_p M_b and H_p M_b of the same pitch
// and M_p x [G_b ; H_b ; M_b] of 2 rows128_b + ld words (rows128_b: n_b up to the next multiple of 128), about 6 n_b.
constexpr uint64_t kTopkPanelBytes = 256ull << 20;
uint64_t dosage_topk_plane_words(uint64_t n_b, bool complete);
// Rows per panel: `panel_rows` as given (a multiple of 256: the caller has checked), or for 0 the largest multiple of 256
// whose planes hold at most kTopkPanelBytes, at least 256; never more than n_rows rounded up to 256.
uint64_t dosage_topk_panel_rows(uint64_t panel_rows, uint64_t n_rows, uint64_t plane_words_per_row);

}  // namespace storm
