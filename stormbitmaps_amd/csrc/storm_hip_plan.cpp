// storm_hip_plan.cpp — the planners of the matrix-core kernels' work lists and of the sparse arena: pure host computation,
// no device, no HIP runtime (storm_hip_plan.h). The launchers in storm_hip_mfma.hip and storm_hip_sparse.hip compare a
// request with the one their cached list was planned from, call the planner, and upload; the exported storm_hip_*_plan
// functions at the end show the K2 plans to the CPU tests (tests/test_dist_cpu.py), tests/arena_plan/driver.cpp the arena's.
#include "storm_hip_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <exception>

#include "storm_hip.h"

namespace storm {

bool timing_env() {
    static const bool on = getenv("STORM_HIP_TIMING") != nullptr;   // (read once, not per call)
    return on;
}

uint64_t ranges_hash(const std::vector<RowRange>& ranges) {
    uint64_t h = 1469598103934665603ull;
    for (const RowRange& r : ranges) {
        h = (h ^ r.r0) * 1099511628211ull;
        h = (h ^ r.r1) * 1099511628211ull;
        h = (h ^ r.a_end) * 1099511628211ull;
        h = (h ^ r.back_from) * 1099511628211ull;
    }
    return h;
}

// ---- K2 tiles, sum mode: the tiles of every range's upper triangle x this shard's k-slices ----
int plan_tile_sum(const TileSumRequest& rq, const std::vector<RowRange>& ranges, std::vector<MfmaItem>& items) {
    const uint32_t total_stages = rq.total_stages, shard_rank = rq.shard_rank, shard_count = rq.shard_count;
    const uint32_t spi = std::max(1u, rq.stages_per_item);
    const bool diag_only = rq.diag_only != 0;
    // tiles of every range's upper triangle, in groups of 4 (I) x 8 (J) row blocks
    std::vector<std::pair<uint16_t, uint16_t>> tiles;
    for (const RowRange& rg : ranges) {
        const uint32_t b0 = (uint32_t)(rg.r0 / kTile);
        const uint32_t nT = (uint32_t)((rg.r1 - rg.r0 + kTile - 1) / kTile);
        // (a_end: only the tile rows below it)
        const uint32_t nTa = rg.a_end ? (uint32_t)std::min<uint64_t>(nT, (std::min(rg.a_end, rg.r1) - rg.r0 + kTile - 1) / kTile) : nT;
        for (uint32_t gi = 0; gi < nTa; gi += 4)
            for (uint32_t gj = gi / 8 * 8; gj < nT; gj += 8)
                for (uint32_t i = gi; i < std::min(gi + 4, nTa); ++i)
                    for (uint32_t j = std::max(gj, i); j < std::min(gj + 8, nT); ++j)
                        if (!diag_only || i == j)
                            tiles.emplace_back((uint16_t)(b0 + i), (uint16_t)(b0 + j));
    }
    // Sharding is by k-group (kGroupStages stages = 64 words of k), the same ownership rule as
    // the strips and the expand kernel; k-slices are cut so that none straddles two groups.
    std::vector<std::pair<uint32_t, uint32_t>> slices;  // (first stage, stages) owned by this shard
    for (uint32_t g0 = 0; g0 < total_stages; g0 += kGroupStages) {
        if ((g0 / kGroupStages) % shard_count != shard_rank) continue;
        const uint32_t g1 = std::min(total_stages, g0 + kGroupStages);
        for (uint32_t s0 = g0; s0 < g1; s0 += spi) slices.emplace_back(s0, std::min(spi, g1 - s0));
    }
    // k-slice major; within a slice, runs of 32 consecutive tiles go to one XCD. Block b runs
    // on XCD b % 8 (observed round-robin dispatch; only speed depends on it), so each chunk of
    // 256 tiles (8 runs of 32) is emitted interleaved: position-major, run-minor.
    items.clear();
    const size_t n = tiles.size();
    for (const auto& sl : slices) {
        const uint32_t s0 = sl.first, ns = sl.second;
        for (size_t c = 0; c < n; c += 256)
            for (size_t pos = 0; pos < 32; ++pos)
                for (size_t x = 0; x < 8; ++x) {
                    const size_t L = c + x * 32 + pos;
                    if (L >= n) continue;
                    if (rq.one_tile_probe)  // timing probe only: every item reads one tile
                        items.push_back({tiles[0].first, tiles[0].first, s0, ns});
                    else
                        items.push_back({tiles[L].first, tiles[L].second, s0, ns});
                }
    }
    if (items.size() != slices.size() * n) {
        set_error("K2 item table construction lost tiles (%zu != %zu)", items.size(),
                  slices.size() * n);
        return STORM_HIP_EINVAL;
    }
    if (items.size() >= (1ull << 31)) {
        set_error("K2: %zu tile items exceed the grid limit", items.size());
        return STORM_HIP_EINVAL;
    }
    return STORM_HIP_OK;
}

// ---- strips ----
static inline uint32_t strip_item_cost(const StripItem& it, uint32_t per_tile) {
    return (it.j1 - it.j0) + it.diag * per_tile + 10u;  // stages + ~10 stages' worth of prologue
}

// Strip items for this shard; the shard's slices are dealt to the 8 XCDs (block b runs on XCD
// b % 8 — observed, speed only), and inside an XCD's list the items of one slice are consecutive,
// longest run first.
struct StripShaping {  // work-list shaping knobs: StripOptions with the run length decided
    int max_run = 128, tail_run = 32, tail_slices = 3, lpt_rounds = 6;
    int xcd_group = 1;  // consecutive slices that share an XCD (2 for the bit-operand strips: slices 2j, 2j + 1 read the same bits)
    bool persistent = false, one_slice_probe = false;
    // Ownership among the shards: false = whole k-slices first, the leftover slices cut along the pair space
    // (above); true = EVERY slice is cut along the pair space (north_star's literal split: a shard multiplies
    // its share of the tile pairs over all of k). Option k2_shard_pairs; rehearsed side by side in
    // tools/bench_shards.py.
    bool pair_space = false;
    // The rows form with its tail chosen (choose_strip_shaping): longest first means by what the kernel issues for an item
    // below n_rows (strip_rows_item_mfmas: a resident diagonal is 4 1/8 stages, not 8), and the estimate is strip_rows_makespan.
    bool rows_cost = false;
    uint32_t n_rows = kStripRowsNoTrim;
};
// One slice = every A tile against the B blocks behind it; `max_run` caps the stages per item.
static void emit_strip_slice(const std::vector<RowRange>& ranges, uint32_t a_tile, uint32_t ks_data, uint32_t max_run,
                             std::vector<StripItem>& dst) {
    const uint32_t kPerTile = a_tile / kStripBRows;
    for (const RowRange& rg : ranges) {
        if (rg.back_from != ~0ull) {   // a row panel that has just arrived: its tiles against everything in front of them
            const uint32_t blk0 = (uint32_t)(rg.r0 / kStripBRows);
            for (uint64_t a0 = rg.back_from; a0 < rg.r1; a0 += a_tile) {
                const uint32_t a_row0 = (uint32_t)a0, end = (uint32_t)(a0 / kStripBRows);
                if (end <= blk0) {
                    dst.push_back({a_row0, 1, end, end, ks_data});
                    continue;
                }
                for (uint32_t j0 = blk0; j0 < end; j0 += max_run)
                    dst.push_back({a_row0, (uint32_t)(j0 == blk0), j0, std::min(end, j0 + max_run), ks_data});
            }
            continue;
        }
        // A tiles of a_tile rows from the start of the range (the rows between r1 and
        // the end of its last A tile are zero: the caller pads ranges accordingly)
        const uint64_t a_rows = (rg.a_end ? std::min(rg.a_end, rg.r1) : rg.r1) - rg.r0;  // A tiles only below a_end
        const uint32_t nA = (uint32_t)((a_rows + a_tile - 1) / a_tile);
        const uint32_t jend = (uint32_t)((rg.r1 + kStripBRows - 1) / kStripBRows);  // absolute
        for (uint32_t i = 0; i < nA; ++i) {
            const uint32_t a_row0 = (uint32_t)rg.r0 + i * a_tile;
            const uint32_t first = a_row0 / (uint32_t)kStripBRows + kPerTile;
            if (first >= jend) {  // last tile of the range: only its own triangle
                dst.push_back({a_row0, 1, first, first, ks_data});
                continue;
            }
            for (uint32_t j0 = first; j0 < jend; j0 += max_run)
                dst.push_back({a_row0, (uint32_t)(j0 == first), j0,
                               std::min(jend, j0 + max_run), ks_data});
        }
    }
}
// Pure host computation (no device): the list, in launch order, and for the persistent form the
// per-XCD queue bounds.
static void build_strip_items(const StripShaping& sh, const std::vector<RowRange>& ranges,
                              uint32_t n_kslices, uint32_t shard_rank, uint32_t shard_count,
                              uint32_t a_tile, std::vector<StripItem>& items,
                              uint32_t queue_base[8], uint32_t queue_count[8], double* makespan = nullptr,
                              uint32_t slots_per_xcd = 128) {
    // stages per item: <= 4096 keeps the f32 accumulators exact; shorter runs trade one more A
    // load per run for a shorter tail at the end of the launch
    const uint32_t kMaxRun = (uint32_t)std::min(4096, std::max(1, sh.max_run));
    const uint32_t kTailRun = (uint32_t)std::min(4096, std::max(1, sh.tail_run));
    const uint32_t kPerTile = a_tile / kStripBRows;
    // The slices of this shard, dealt to the XCDs in turn.
    std::vector<std::vector<uint32_t>> slices_of(8);
    uint32_t local = 0;
    const bool pair_mode = sh.pair_space && shard_count > 1;
    const uint32_t modulo_slices = pair_mode ? n_kslices : strip_modulo_slices(n_kslices, shard_count);
    const uint32_t xg = (uint32_t)std::max(1, sh.xcd_group);
    for (uint32_t ks = 0; ks < modulo_slices; ++ks)
        if (pair_mode || strip_owns_slice(ks, shard_rank, shard_count)) slices_of[(local++ / xg) % 8].push_back(ks);
    std::vector<uint64_t> pair_load(shard_count, 0);  // pair mode: stages dealt to every shard so far
    auto emit_slice_all = [&](uint32_t ks, uint32_t max_run, std::vector<StripItem>& dst) {
        // k2_debug & 16 (timing probe, wrong results): every XCD re-reads one k-slice, i.e. the
        // launch as it would run if nothing ever missed in L2
        emit_strip_slice(ranges, a_tile, sh.one_slice_probe ? ks % 8u : ks, max_run, dst);
    };
    // Every slice holds the same items but for its slice number: the list of one slice is built (and, for the long runs,
    // sorted longest first) ONCE per run length and copied with the number filled in — built and sorted slice by slice,
    // three candidate run lengths and the final list cost the first call at the headline shape 1.4 ms of host time, a first
    // call at 10000 x 524288 twenty times that [r6].
    const uint32_t kTailLen = std::min(kMaxRun, kTailRun);
    std::vector<StripItem> proto_main, proto_tail;
    bool have_main = false, have_tail = false;
    // (rows_cost: MFMAs; a diagonal's by the tile's blocks that hold a row, counted once per block count)
    uint32_t diag_mfmas[kStripRowsBlocks + 1] = {};
    if (sh.rows_cost)
        for (uint32_t nb = 0; nb <= kStripRowsBlocks; ++nb) diag_mfmas[nb] = strip_rows_item_mfmas(0, 1, 0, 0, nb * (uint32_t)kStripBRows);
    auto length_of = [&](const StripItem& p) -> uint32_t {
        if (!sh.rows_cost) return (p.j1 - p.j0) + p.diag * kPerTile;
        return strip_rows_item_mfmas(p.a_row0, 0, p.j0, p.j1, sh.n_rows) + (p.diag ? diag_mfmas[strip_rows_real_blocks(p.a_row0, sh.n_rows)] : 0u);
    };
    auto by_length = [&](const StripItem& p, const StripItem& q) { return length_of(p) > length_of(q); };
    auto longest_first = [&](std::vector<StripItem>& v) {
        if (!sh.rows_cost) return std::stable_sort(v.begin(), v.end(), by_length);
        // (what an item costs in the model is worked out once per item, not once per comparison)
        std::vector<std::pair<uint32_t, uint32_t>> order(v.size());
        for (size_t k = 0; k < v.size(); ++k) order[k] = {length_of(v[k]), (uint32_t)k};
        std::stable_sort(order.begin(), order.end(), [](const auto& p, const auto& q) { return p.first > q.first; });
        std::vector<StripItem> sorted(v.size());
        for (size_t k = 0; k < v.size(); ++k) sorted[k] = v[order[k].second];
        v.swap(sorted);
    };
    auto emit_copy = [&](uint32_t ks, uint32_t max_run, std::vector<StripItem>& dst) {
        std::vector<StripItem>& proto = max_run == kMaxRun ? proto_main : proto_tail;
        bool& have = max_run == kMaxRun ? have_main : have_tail;
        if (!have) {
            emit_slice_all(0u, max_run, proto);
            if (max_run == kMaxRun) longest_first(proto);
            have = true;
        }
        const uint32_t ks_data = sh.one_slice_probe ? ks % 8u : ks;
        const size_t at = dst.size();
        dst.insert(dst.end(), proto.begin(), proto.end());
        for (size_t k = at; k < dst.size(); ++k) dst[k].ks = ks_data;
    };
    // pair mode: this shard's share of the slice — the slice's items, longest first onto the least loaded shard
    // (every shard walks the slices in the same order and computes the same deal)
    auto emit_slice = [&](uint32_t ks, uint32_t max_run, std::vector<StripItem>& dst) {
        if (!pair_mode) return (max_run == kMaxRun || max_run == kTailLen) ? emit_copy(ks, max_run, dst) : emit_slice_all(ks, max_run, dst);
        std::vector<StripItem> all;
        emit_slice_all(ks, max_run, all);
        std::stable_sort(all.begin(), all.end(), [&](const StripItem& p, const StripItem& q) {
            return strip_item_cost(p, kPerTile) > strip_item_cost(q, kPerTile);
        });
        for (const StripItem& it : all) {
            const uint32_t r = (uint32_t)(std::min_element(pair_load.begin(), pair_load.end()) - pair_load.begin());
            pair_load[r] += strip_item_cost(it, kPerTile);
            if (r == shard_rank) dst.push_back(it);
        }
    };
    // An XCD runs its list in order on ~128 workgroup slots. Long items keep the per-item cost
    // (A fragments, ring fill, diagonal phase) low, but whatever is still running when the list
    // runs dry sets the tail: with whole-length items the last slices leave most slots idle for
    // up to one 157-stage item (10 % of the launch at the headline shape, by list-scheduling
    // simulation and by measurement). So the LAST k2_tail_slices slices of every XCD are cut into
    // short runs and merged longest-first, which lets the list end on many small items.
    // leftover slices: short runs, dealt to the shards by longest-processing-time-first
    std::vector<std::vector<StripItem>> leftover_of(8);
    if (modulo_slices < n_kslices) {
        std::vector<uint64_t> load(shard_count, 0);
        for (uint32_t ks = modulo_slices; ks < n_kslices; ++ks) {
            std::vector<StripItem> all;
            emit_slice_all(ks, std::min(kMaxRun, kTailRun), all);
            std::stable_sort(all.begin(), all.end(), [&](const StripItem& p, const StripItem& q) {
                return strip_item_cost(p, kPerTile) > strip_item_cost(q, kPerTile);
            });
            const uint32_t xcd = (local++ / xg) % 8;  // one slice stays on one XCD's L2
            for (const StripItem& it : all) {
                const uint32_t r = (uint32_t)(std::min_element(load.begin(), load.end()) - load.begin());
                load[r] += strip_item_cost(it, kPerTile);
                if (r == shard_rank) leftover_of[xcd].push_back(it);
            }
        }
    }
    const uint32_t kTail = (uint32_t)std::max(0, sh.tail_slices);
    std::vector<std::vector<StripItem>> per_xcd(8);
    // (an estimate — `makespan` asked for — is made from the list of XCD 0 alone: the slices are dealt to the XCDs in turn
    //  from 0, so its list is as long as any; the other seven lists and the launch order are not built)
    const int n_lists = makespan ? 1 : 8;
    for (int x = 0; x < n_lists; ++x) {
        const std::vector<uint32_t>& sl = slices_of[x];
        const size_t n_main = sl.size() > kTail ? sl.size() - kTail : 0;
        // Within a slice, longest first: the XCD's dispatcher deals consecutive workgroups to its
        // shader engines in turn, so a list that alternates long and short items (the two runs of
        // one A tile) sends all the long ones to the same engines and leaves the others idle
        // (schedule trace: 60 % of the slots occupied; max_run = 64, 72 or 100 lost 10-25 %).
        for (size_t k = 0; k < n_main; ++k) {
            if (!pair_mode) {   // (the copy of the sorted list of one slice)
                emit_slice(sl[k], kMaxRun, per_xcd[x]);
                continue;
            }
            std::vector<StripItem> one;
            emit_slice(sl[k], kMaxRun, one);
            std::stable_sort(one.begin(), one.end(), by_length);
            per_xcd[x].insert(per_xcd[x].end(), one.begin(), one.end());
        }
        std::vector<StripItem> tail;
        for (size_t k = n_main; k < sl.size(); ++k) emit_slice(sl[k], std::min(kMaxRun, kTailRun), tail);
        tail.insert(tail.end(), leftover_of[x].begin(), leftover_of[x].end());
        longest_first(tail);
        per_xcd[x].insert(per_xcd[x].end(), tail.begin(), tail.end());
        // A short list (a few rounds of the XCD's ~128 slots: small N, or a 1/8 shard) is all
        // tail: order the whole of it longest-first. The L2 locality that slice-major order buys
        // is worth 1-2 %, the tail of a 2-round launch a third of its time (N = 2048: the
        // schedule trace showed the launch draining for 24 of its 66 us).
        if (per_xcd[x].size() <= (size_t)128 * (size_t)std::max(0, sh.lpt_rounds))
            longest_first(per_xcd[x]);
    }
    if (makespan) {
        // List-scheduling estimate of the launch, in stage times: an XCD hands its list, in order, to its workgroup
        // slots (4 per CU); an item costs its stages + ~5 for the prologue (A rows, two images) + 3 more for the
        // non-pipelined diagonal phase. Used to choose the run length (k2_max_run = 0).
        // [r6] Only the list of XCD 0 is walked (above), and of a long list only the last 16 rounds, behind an evenly loaded start: what decides
        // between the run lengths is the tail. The full walk of all eight lists took 2.5 ms of a first call at the
        // headline shape (three candidates), 25 ms at 10000 x 524288.
        auto cost_of = [&](const StripItem& it) { return (double)(it.j1 - it.j0) + (it.diag ? kPerTile + 3.0 : 0.0) + 5.0; };
        const std::vector<StripItem>& list = per_xcd[0];
        const size_t n_slots = std::max<uint32_t>(1, slots_per_xcd);
        const size_t start = list.size() > 16 * n_slots ? list.size() - 16 * n_slots : 0;
        double before = 0;
        for (size_t k = 0; k < start; ++k) before += cost_of(list[k]);
        std::vector<double> slot(n_slots, before / (double)n_slots);  // a min-heap of the slots' free times
        auto later = [](double p, double q) { return p > q; };
        for (size_t k = start; k < list.size(); ++k) {
            std::pop_heap(slot.begin(), slot.end(), later);
            slot.back() += cost_of(list[k]);
            std::push_heap(slot.begin(), slot.end(), later);
        }
        const double worst = *std::max_element(slot.begin(), slot.end());
        *makespan = worst;
        items.clear();
        return;
    }
    items.clear();
    if (sh.persistent) {  // one contiguous queue per XCD
        for (int x = 0; x < 8; ++x) {
            queue_base[x] = (uint32_t)items.size();
            queue_count[x] = (uint32_t)per_xcd[x].size();
            items.insert(items.end(), per_xcd[x].begin(), per_xcd[x].end());
        }
    } else {  // dispatcher order: block b runs on XCD b % 8
        size_t longest = 0;
        for (auto& v : per_xcd) longest = std::max(longest, v.size());
        for (size_t pos = 0; pos < longest; ++pos)
            for (int x = 0; x < 8; ++x)
                if (pos < per_xcd[x].size()) items.push_back(per_xcd[x][pos]);
    }
}

// The rows form's tail, chosen with the run length: one device's whole pass, neither k2_tail_run nor k2_tail_slices set.
// `now` is the shaping such a pass always had — the run length above (or the caller's), the last 3 slices in runs of 32 —
// and stays unless one of kStripRowsShapings models at least 0.5 % shorter than the choice so far (the near-tie rule of
// the run length). Where it stays the list is the one the pass always had, byte for byte; a list of another shaping is
// ordered by what its items cost in the model (rows_cost).
// The model (strip_rows_makespan, storm_hip_plan.h) walks the list of the XCD that gets the most slices, a compute unit
// holding 4 workgroups of the kernel. No list is built for it: a slice's items cut at the main and at the tail length,
// each sorted as the list will have them, give every position of the XCD's list — the main slices one behind another, then
// every item of the tail's sorted slice once per tail slice. Of a long list only the last kStripRowsWalkRounds rounds are
// walked, from the middle of a launch: everything in front of them is taken to have kept every pipe busy, and at the start
// of the walk every slot holds a workgroup whose work left is spread evenly up to an item of the walk's first round — on a
// compute unit whose four workgroups share the pipe, items of one length end a quarter of their time apart, and the compute
// units a fraction of that apart. (All slots free at once would walk the rounds in step, which no launch does behind its
// first.) A list whose front holds less than twice that work is walked whole, from an empty XCD.
constexpr size_t kStripRowsWalkRounds = 4;
static StripShaping choose_rows_tail(const StripShaping& now, const std::vector<RowRange>& ranges, uint32_t n_kslices, uint32_t a_tile,
                                     uint32_t slots_per_xcd, bool run_is_set) {
    const bool timing = timing_env();
    uint32_t n_rows = kStripRowsNoTrim;   // (where the launcher tells the kernel that the rows end)
    if (ranges.size() == 1 && ranges[0].r0 == 0 && ranges[0].a_end == 0 && ranges[0].back_from == ~0ull && ranges[0].r1 < (uint64_t)kStripRowsNoTrim)
        n_rows = (uint32_t)ranges[0].r1;
    // the slices of the XCD that gets the most: whole units in turn, the leftover ones (cut like the tail) behind them
    uint32_t whole[8] = {}, left_over[8] = {}, local = 0;
    const uint32_t modulo_slices = strip_modulo_slices(n_kslices, 1), xg = (uint32_t)std::max(1, now.xcd_group);
    for (uint32_t ks = 0; ks < n_kslices; ++ks) ++(ks < modulo_slices ? whole : left_over)[(local++ / xg) % 8];
    uint32_t x = 0;
    for (uint32_t i = 1; i < 8; ++i)
        if (whole[i] + left_over[i] > whole[x] + left_over[x]) x = i;
    // a slice cut at `run`, in the order of the list: what each item costs (stages), longest first by the list's key
    struct SliceCosts {
        uint32_t run;
        bool rows_cost;
        std::vector<double> cost;
        double sum;
    };
    std::vector<SliceCosts> slices;
    slices.reserve(16);
    auto slice_costs = [&](uint32_t run, bool rows_cost) -> const SliceCosts& {
        for (const SliceCosts& sc : slices)
            if (sc.run == run && sc.rows_cost == rows_cost) return sc;
        std::vector<StripItem> items;
        emit_strip_slice(ranges, a_tile, 0u, run, items);
        std::vector<std::pair<uint32_t, uint32_t>> keyed(items.size());   // (the list's key, MFMAs)
        for (size_t k = 0; k < items.size(); ++k) {
            const StripItem& it = items[k];
            const uint32_t mfmas = strip_rows_item_mfmas(it.a_row0, it.diag, it.j0, it.j1, n_rows);
            keyed[k] = {rows_cost ? mfmas : (it.j1 - it.j0) + it.diag * (a_tile / (uint32_t)kStripBRows), mfmas};
        }
        std::stable_sort(keyed.begin(), keyed.end(), [](const auto& p, const auto& q) { return p.first > q.first; });
        slices.push_back({run, rows_cost, {}, 0.0});
        SliceCosts& sc = slices.back();
        sc.cost.resize(keyed.size());
        for (size_t k = 0; k < keyed.size(); ++k) sc.sum += sc.cost[k] = (double)keyed[k].second / kStripRowsStageMfmas;
        return sc;
    };
    struct Walk {
        std::vector<double> cost, resident;
        double t0 = 0, makespan = 0;
    };
    std::vector<Walk> walks;   // (candidates whose lists end alike — a long tail behind any run length — are walked once)
    walks.reserve(8);
    const uint32_t n_cus = std::max<uint32_t>(1, slots_per_xcd / 4u), n_slots = n_cus * 4u;
    auto model = [&](const StripShaping& sh) {
        const uint32_t run = (uint32_t)std::min(4096, std::max(1, sh.max_run));
        const SliceCosts& main = slice_costs(run, sh.rows_cost);
        const SliceCosts& tail = slice_costs(std::min(run, (uint32_t)std::min(4096, std::max(1, sh.tail_run))), sh.rows_cost);
        const size_t n_main = whole[x] > (uint32_t)std::max(0, sh.tail_slices) ? whole[x] - (uint32_t)sh.tail_slices : 0;
        const size_t n_tail = whole[x] - n_main + left_over[x];
        const size_t in_main = n_main * main.cost.size(), n_list = in_main + n_tail * tail.cost.size();
        walks.emplace_back();
        Walk& w = walks.back();
        if (n_list == 0) return 0.0;
        auto at = [&](size_t k) { return k < in_main ? main.cost[k % main.cost.size()] : tail.cost[(k - in_main) / n_tail]; };
        size_t start = n_list > kStripRowsWalkRounds * (size_t)n_slots ? n_list - kStripRowsWalkRounds * (size_t)n_slots : 0;
        if (n_list <= (size_t)128 * (size_t)std::max(0, sh.lpt_rounds)) start = 0;   // (a short list: all of it longest first)
        for (int pass = 0; pass < 2; ++pass) {
            w.cost.resize(n_list - start);
            double walked = 0;
            for (size_t k = start; k < n_list; ++k) walked += w.cost[k - start] = at(k);
            if (start == 0) break;
            const double before = main.sum * (double)(n_main + n_tail) - walked;   // (a slice holds the same work however it is cut)
            double round = 0, held = 0;
            for (uint32_t k = 0; k < n_slots; ++k) round += w.cost[k];
            round /= (double)n_slots;
            w.resident.resize(n_slots);
            for (uint32_t c = 0; c < n_cus; ++c)
                for (uint32_t s = 0; s < 4u; ++s) held += w.resident[c * 4u + s] = round * ((double)s + (double)(c + 1u) / (double)n_cus) / 4.0;
            if (before >= 2.0 * held) {
                w.t0 = (before - held) / (double)n_cus;
                break;
            }
            w.resident.clear();
            start = 0;
        }
        if (n_list <= (size_t)128 * (size_t)std::max(0, sh.lpt_rounds)) std::sort(w.cost.begin(), w.cost.end(), std::greater<double>());
        for (size_t seen = 0; seen + 1 < walks.size(); ++seen)
            if (walks[seen].t0 == w.t0 && walks[seen].cost == w.cost && walks[seen].resident == w.resident) return w.makespan = walks[seen].makespan;
        return w.makespan = strip_rows_makespan(w.cost.data(), w.cost.size(), n_cus, 4u, kStripRowsStartStages, w.t0,
                                                w.resident.empty() ? nullptr : w.resident.data());
    };
    StripShaping best = now;
    double best_ms = model(now);
    if (timing)
        fprintf(stderr, "[strip plan] rows form, max_run %3d tail_run %2d tail_slices %2d (as it was): modelled makespan %.1f stages\n",
                now.max_run, now.tail_run, now.tail_slices, best_ms);
    for (const StripChoice& cand : kStripRowsShapings) {
        if (run_is_set && cand.max_run != kStripRowsShapings[0].max_run) continue;   // a set run length: the tails alone, once each
        StripShaping trial = now;
        trial.rows_cost = true;
        trial.n_rows = n_rows;
        if (!run_is_set) trial.max_run = cand.max_run;
        trial.tail_run = cand.tail_run;
        trial.tail_slices = cand.tail_slices;
        const double ms = model(trial);
        if (timing)
            fprintf(stderr, "[strip plan] rows form, max_run %3d tail_run %2d tail_slices %2d: modelled makespan %.1f stages\n",
                    trial.max_run, trial.tail_run, trial.tail_slices, ms);
        if (ms < best_ms * 0.995) {   // (ties and near-ties go to the earlier candidate)
            best = trial;
            best_ms = ms;
        }
    }
    return best;
}

// The shaping a pass runs with, from the options alone — NEVER from the calling rank. Where ownership is dealt along
// the pair space (k2_shard_pairs, and the leftover slices of the default mode) every rank replays the same deal of
// the same items, so every rank must cut the slices at the same run length: a choice made from one rank's own list
// gave ranks [64, 96, 96] at N = 6144 / world 3 and pairs were dropped or counted twice. The automatic
// run length (max_run = 0) is therefore the candidate whose SLOWEST rank schedules shortest; every rank evaluates
// all ranks' lists and arrives at the same answer. Shared (through plan_strips) by the device path (ensure_strip_items)
// and the host-only planner (storm_hip_strip_plan3), so that the plan the CPU tests partition is the plan the GPU launches.
static StripShaping choose_strip_shaping(const StripOptions& o, const std::vector<RowRange>& ranges, uint32_t n_kslices,
                                         uint32_t shard_count, uint32_t a_tile) {
    StripShaping sh;
    sh.tail_run = o.tail_run;
    sh.tail_slices = o.tail_slices;
    sh.lpt_rounds = o.lpt_rounds;
    sh.xcd_group = o.xcd_group;
    sh.persistent = o.persistent != 0;
    sh.one_slice_probe = o.one_slice_probe != 0;
    sh.pair_space = o.shard_pairs != 0;
    sh.max_run = o.max_run;
    const uint32_t slots = (uint32_t)std::max(1, o.n_cus / 8 * 4);
    const bool timing = timing_env();
    // (the rows form, one device's whole pass, no tail set: the tail is chosen too, behind the run length)
    const bool rows_tail = o.rows_form && o.tail_auto && shard_count == 1;
    if (o.max_run != 0) return rows_tail ? choose_rows_tail(sh, ranges, n_kslices, a_tile, slots, true) : sh;
    // auto: the run length whose list schedules shortest (the tail of the launch decides between them: N = 6144 is
    // 6 % faster with 64, N = 7168 / 8192 with 96, N = 3072 with 128; tools/archive/sweep_maxrun.py)
    double best = 0;
    for (int cand : {96, 64, 128}) {
        StripShaping trial = sh;
        trial.max_run = cand;
        double worst = 0;
        size_t n_items = 0;
        for (uint32_t r = 0; r < shard_count; ++r) {
            std::vector<StripItem> tmp;
            uint32_t qb[8], qc[8];
            double ms = 0;
            build_strip_items(trial, ranges, n_kslices, r, shard_count, a_tile, tmp, qb, qc, &ms, slots);
            worst = std::max(worst, ms);
            n_items += tmp.size();
        }
        if (timing)
            fprintf(stderr, "[strip plan] max_run %3d: %zu items over %u rank(s), predicted makespan %.0f stages\n", cand,
                    n_items, shard_count, worst);
        if (sh.max_run == 0 || worst < best * 0.995) {   // (ties and near-ties go to the earlier candidate)
            sh.max_run = cand;
            best = worst;
        }
    }
    return rows_tail ? choose_rows_tail(sh, ranges, n_kslices, a_tile, slots, false) : sh;
}

StripRequest strip_request(const StripOptions& opt, const std::vector<RowRange>& ranges, uint32_t n_kslices,
                           uint32_t shard_rank, uint32_t shard_count, uint32_t a_tile) {
    StripRequest rq;
    rq.opt = opt;
    rq.n_kslices = n_kslices;
    rq.shard_rank = shard_rank;
    rq.shard_count = shard_count;
    rq.a_tile = a_tile;
    rq.ranges_hash = ranges_hash(ranges);
    return rq;
}

void plan_strips(const StripRequest& rq, const std::vector<RowRange>& ranges, std::vector<StripItem>& items,
                 uint32_t queue_base[8], uint32_t queue_count[8], StripChoice* chosen) {
    const StripShaping sh = choose_strip_shaping(rq.opt, ranges, rq.n_kslices, rq.shard_count, rq.a_tile);
    if (chosen) *chosen = {sh.max_run, sh.tail_run, sh.tail_slices};
    build_strip_items(sh, ranges, rq.n_kslices, rq.shard_rank, rq.shard_count, rq.a_tile, items, queue_base, queue_count);
}

// ---- how an all-pairs pass chooses its form ----
// Which strips (option k2_strip_operands; 0 = the default: K2b unless a non-default ring or MFMA shape asks for the FP4
// strips; 6 = K2b with 512-row A tiles, a form of K2b taken where the matrix allows): ONE rule for the dense matrix, the
// panels of an upload and the pool rows of a sparse container. The default is by measurement (same box, M = 65536,
// tools/archive/sweep_k2b.py, profiles/r04_a_sweep_k2b.jsonl): the strips on bit operands with the FP4 image built in the
// LDS (K2b, strip16_bits_kernel) are ahead of the one-launch stream (K2q) and of the FP4 strips at every size —
// 8.2 / 9.5 / 14.9 us at N = 256, 17.1 / 20.2 / 31.8 at 1024, 41.9 / 43.4 / 60.4 at 2048, 142 / 143 / 169 at
// 4096, 537 / 539 / 591 at 8192, 752 / 809 / 817 at 10000 (K2q is ahead around N = 6144 only: 311 against
// 325) — and for the shards of a multi-GPU pass (an eighth of the headline matrix: 103 against 119 us).
static int strip_operands_of(const PassOptions& o) {
    if (o.k2_strip_operands == 6) return 5;
    if (o.k2_strip_operands != 0) return o.k2_strip_operands;
    return (o.k2_ring == kStripRingDefault && o.k2_shape == 16) ? 5 : 4;
}
// The bit operands are read where they lie: the zero rows of the allocation must reach the next multiple of the form's A
// tile (a matrix created before an option was set may lack them) and a B stage of 64 rows is addressed with 32-bit DMA
// offsets. The timing probes and the work queues exist for the FP4 strips only.
static bool rows_padded_to(const PassShape& s, uint64_t a_tile) { return (s.n_rows + a_tile - 1) / a_tile * a_tile <= s.n_rows_pad; }
static bool bit_operands_reach(const PassOptions& o, const PassShape& s) {
    return !o.k2_persistent && o.k2_debug == 0 && rows_padded_to(s, kStripBits.a_tile) &&
           s.stride_words * 8 * (uint64_t)kStripBRows < (1ull << 32);
}
// K2b's A rows per wave (option k2_strip_rows): 128 = strip16_rows_kernel, wherever the zero rows of the allocation reach the
// next multiple of 512 (its A tile; option 6's rule) — otherwise, and for 64, strip16_bits_kernel. 0 = by measurement
// (profiles/k2b_rows128_ab.txt: kernel time by HIP events, the forms alternating in one process, two rounds; 256-row form
// -> 128 rows per wave): 10000 x 65536 0.755 -> 0.721 ms, 10000 x 524288 6.11 -> 5.64, 8192 x 65536 0.512 -> 0.488,
// 4096 x 65536 0.1422 -> 0.1331, 2048 x 65536 0.0450 -> 0.0442 — ahead by 1.5 .. 7.7 %, everywhere more than three times the
// 256-row form's own spread between the rounds (0.1 .. 0.4 %). The rule takes the new form inside what was measured: one
// device's whole pass, from 2048 rows of 65536 bits up. Smaller matrices (the diagonal phase is 8 of an item's stages, not
// 4, and at 2048 rows the margin is down to 1.5 %), narrower rows (fewer than 512 slices for 8 XCDs in groups of 8) and the
// shards of a multi-GPU pass were not measured and keep the 256-row form. Where the 512-row tiles were asked for (6) the
// option is not read.
static const StripForm* dense_strip_form(const PassOptions& o, const PassShape& s) {
    const bool pad512 = rows_padded_to(s, kStripRows.a_tile);
    if (o.k2_strip_operands == 6) return pad512 ? &kStripBitsWide : &kStripBits;
    const bool by_rule = s.shard_count == 1 && s.n_rows >= 2048 && s.n_words >= 1024;
    return o.k2_strip_rows != 64 && pad512 && (o.k2_strip_rows == 128 || by_rule) ? &kStripRows : &kStripBits;
}
static PassChoice fp4_pass(int variant, int operands_used) {
    return {variant == 5 ? PassKernel::Fp4StripsWide : variant == 4 ? PassKernel::Fp4Strips : PassKernel::Fp4Tiles, nullptr, variant,
            operands_used, variant == 5 ? 2 : variant == 4 ? 1 : 0, false};
}
static PassChoice choose_dense_pass(const PassOptions& o, const PassShape& s) {
    // variant -1 = auto: the matrix-core strips at every size (rows beyond their 32-bit DMA offsets are multiplied k-chunk by
    // k-chunk over a compact shadow). Measured (tools/archive/bench_crossover.py): they beat the popcount kernel from N = 64
    // up (10-37 us vs its 42-84 us latency floor at N <= 256).
    const int variant = o.variant < 0 ? 4 : o.variant;
    if (variant < 3) return {PassKernel::Popcount, nullptr, variant, 0, 0, false};
    const int ops = strip_operands_of(o);
    if (variant != 4 || !(ops == 1 || ops == 2 || ops == 3 || ops == 5) || !bit_operands_reach(o, s)) return fp4_pass(variant, 4);
    if (ops == 5) {
        const StripForm* form = dense_strip_form(o, s);
        return {PassKernel::Strips, form, variant, form->operands_report, 0, false};
    }
    const PassKernel kernel = ops == 2 ? PassKernel::Bitstream : ops == 3 && o.tools_build ? PassKernel::ToolsBitwave : PassKernel::ToolsStripBits;
    return {kernel, nullptr, variant, ops, 0, false};
}
PassChoice choose_pass(PassCaller caller, const PassOptions& o, const PassShape& s) {
    switch (caller) {
    case PassCaller::Dense:
        return choose_dense_pass(o, s);
    case PassCaller::DenseUpload: {
        // the rows travel in panels behind which K2b multiplies (launch_pairw_bits_upload) from 2048 rows on; small matrices
        // and forced kernel forms: the copy, then the pass
        if ((o.variant < 0 || o.variant == 4) && strip_operands_of(o) == 5 && s.n_rows >= 2048 && bit_operands_reach(o, s))
            return {PassKernel::Strips, &kStripBits, 4, kStripBits.operands_report, 0, true};
        return choose_dense_pass(o, s);
    }
    case PassCaller::SparsePool: {
        // Matrix-core path when the columns are big enough to fill the chip (same rule as the dense container): every column
        // is an independent all-pairs problem over its pool rows.
        const int variant = o.variant < 0 ? (s.widest >= 64 ? 4 : 2) : o.variant;
        if (variant < 3) return {PassKernel::Popcount, nullptr, variant, 0, 0, false};
        // K2b multiplies the pool rows as they are: no FP4 shadow of the pool (2.6 GB at c4), no expansion pass. The rows
        // behind a column's last one up to the next multiple of 512 are zero in the pool (columns start on multiples of 512
        // and nothing writes between them). Always the 256-row form.
        if (variant == 4 && strip_operands_of(o) == 5 && o.k2_debug == 0 && !o.k2_persistent && s.rows_dst <= s.pool_rows_ready + 512)
            return {PassKernel::Strips, &kStripBits, variant, kStripBits.operands_report, 0, false};
        return fp4_pass(variant, 0);
    }
    }
    return {PassKernel::Popcount, nullptr, 2, 0, 0, false};   // (not reached)
}

// ---- write-mode tiles of 256 x 256 ----
// Launch order of write-mode tiles for L2 reuse. A tile item streams 8 MiB per operand at the
// headline shape (256 rows x all of k), twice an XCD's L2: in row-major order the 32 tiles an
// XCD works on at a time share their A rows and nothing else, and the kernel fetched 12.6 GB per
// launch from beyond L2 (47 % of its L2 requests missed; it ran at the HBM rate with the matrix
// pipe 44 % busy: profiles/r02_d_*). Here the tiles [i0, i1) x [j0, j1) (upper triangle only when
// `triangle`) are cut into groups of 4 x 8, group g goes to XCD g % 8 (block b runs on XCD b % 8:
// observed, speed only), so the 32 workgroups of an XCD — which start together and advance along k
// at the same pace — fetch 12 row-block slices per k-stage instead of 33.
void xcd_grouped_tiles(uint32_t i0, uint32_t i1, uint32_t j0, uint32_t j1, bool triangle,
                              std::vector<std::pair<uint16_t, uint16_t>>& out) {
    std::vector<std::vector<std::pair<uint16_t, uint16_t>>> per_xcd(8);
    uint32_t g = 0;
    for (uint32_t gi = i0; gi < i1; gi += 4)
        for (uint32_t gj = triangle ? std::max(j0, gi / 8 * 8) : j0; gj < j1; gj += 8) {
            std::vector<std::pair<uint16_t, uint16_t>>& dst = per_xcd[g % 8];
            const size_t before = dst.size();
            for (uint32_t i = gi; i < std::min(gi + 4, i1); ++i)
                for (uint32_t j = std::max(gj, triangle ? i + 1 : gj); j < std::min(gj + 8, j1); ++j)
                    dst.emplace_back((uint16_t)i, (uint16_t)j);
            if (dst.size() != before) ++g;
        }
    size_t longest = 0;
    for (auto& v : per_xcd) longest = std::max(longest, v.size());
    for (size_t pos = 0; pos < longest; ++pos)
        for (int x = 0; x < 8; ++x)
            if (pos < per_xcd[x].size()) out.push_back(per_xcd[x][pos]);
}

// The item table of a matrix-output launch. The tile kernel holds one workgroup per CU, so n tiles take ceil(n / CUs)
// rounds and a nearly empty last round costs a whole one. `cost` (optional, one per tile, 1 = a full tile): the tiles
// beyond the last full round of workgroups are cut along k into parts of about equal cost, as many as fill the CUs — a
// short tile (diagonal or ragged under tilebits8_kernel) into fewer parts than a full one.
void plan_matrix_tiles(const MatrixTilesRequest& rq, std::vector<MfmaItem>& items, MatrixPlan* plan) {
    const std::vector<std::pair<uint16_t, uint16_t>>& tiles = rq.tiles;
    const uint32_t total_stages = rq.total_stages;
    const size_t slots = (size_t)std::max(1u, rq.n_cus);
    size_t leftover = rq.split ? tiles.size() % slots : 0;
    // f32 accumulators hold exact integers below 2^24: an item may span at most kMaxExactStages
    // stages (128 bits each). Rows of 2^24 bits and more are therefore cut along k for EVERY tile;
    // the parts add into the cleared window like the parts of the last round do.
    constexpr uint32_t kMaxExactStages = (1u << 24) / 128u - 1u;
    uint32_t min_parts = 1;
    if (total_stages > kMaxExactStages) {
        leftover = tiles.size();
        min_parts = (total_stages + kMaxExactStages - 1) / kMaxExactStages;
    }
    const size_t n_full = tiles.size() - leftover;
    const uint32_t max_parts = std::max(min_parts, total_stages / (uint32_t)rq.min_part);
    auto cost_of = [&](size_t t) { return rq.cost.empty() ? 1.0f : std::max(0.05f, rq.cost[t]); };
    double left_cost = 0;
    for (size_t t = n_full; t < tiles.size(); ++t) left_cost += cost_of(t);
    const double per_part = left_cost / (double)slots;  // what one CU should get of the last round
    std::vector<uint32_t> parts_of(leftover, 1);
    size_t n_parts = 0;
    for (size_t t = n_full; t < tiles.size(); ++t) {
        const double want = per_part > 0 ? cost_of(t) / per_part : 1.0;
        n_parts += parts_of[t - n_full] = std::min(max_parts, std::max(min_parts, (uint32_t)want));
    }
    // rounding down leaves CUs without a part: give them to the tiles whose parts are longest (never
    // more parts than CUs — a 257th item would wait for a whole part)
    while (min_parts == 1 && n_parts < slots && leftover > 0) {
        size_t best = leftover;
        double longest = 0;
        for (size_t i = 0; i < leftover; ++i) {
            const double len = cost_of(n_full + i) / parts_of[i];
            if (parts_of[i] < max_parts && len > longest) longest = len, best = i;
        }
        if (best == leftover) break;
        ++parts_of[best];
        ++n_parts;
    }
    items.clear();
    for (size_t t = 0; t < n_full; ++t) items.push_back({tiles[t].first, tiles[t].second, 0, total_stages});
    for (size_t t = n_full; t < tiles.size(); ++t) {
        const uint32_t parts = parts_of[t - n_full];
        for (uint32_t p = 0; p < parts; ++p) {
            // cuts on multiples of 4 stages: the 16x16 kernel's stage is two of these (128 bytes of
            // an FP4 row), the bit-operand kernels' four (512 bits)
            const uint32_t s0 = (uint32_t)((uint64_t)(total_stages / 4) * p / parts) * 4u;
            const uint32_t s1 = (uint32_t)((uint64_t)(total_stages / 4) * (p + 1) / parts) * 4u;
            items.push_back({tiles[t].first, tiles[t].second, s0, s1 - s0});
        }
    }
    plan->n_items = (uint32_t)items.size();
    plan->n_full = (uint32_t)n_full;
    plan->n_cut = (uint32_t)leftover;
    for (size_t t = n_full; t < tiles.size(); ++t) items.push_back({tiles[t].first, tiles[t].second, 0u, 0u});   // the cut tiles once more: the windows to clear
}

// ---- K2h (tile128_kernel): 128 x 128 tiles for matrices of few 256 x 256 tiles, k-parts whose sums meet inside the launch ----
// The item list of a K2h launch. An item is one part of one tile; a tile of several parts has its sums meet in the launch
// (tile128_kernel). The chip offers `slots` places for workgroups, one or two per CU:
//   * whole rounds of tiles (slots tiles each) stay whole;
//   * the tiles beyond the last whole round — all of them where there are fewer tiles than slots — are cut along k into
//     EQUAL parts, together as many as there are slots: a tile gets its share of the slots rounded down, the slots left
//     over go to the tiles whose parts are longest (the longest part ends the launch; cutting the chunk stream at equal
//     distances across the tile boundaries leaves crumbs that must join a neighbour, and the parts so lengthened — 28
//     chunks where 18 were due at 1024 rows — ended the launch);
//   * one or two slots per CU: whichever loads a CU less, counting what an item costs besides its chunks.
// The tiles on the diagonal come last (they are the ones cut: beside a second workgroup their chunks are cheaper — one wave
// idle, one at three blocks of four — alone on a CU they take as long as any). Items longest first: the dispatcher hands
// the short ones to the slots that end first. Pure host computation.
void plan_tile128(const Tile128Request& rq, Tile128Plan* plan) {
    const uint32_t ia0 = rq.ia0, ia1 = rq.ia1, jb0 = rq.jb0, jb1 = rq.jb1, total_stages = rq.total_stages, n_cus = rq.n_cus;
    const bool triangle = rq.triangle != 0, narrow_windows = rq.narrow_windows != 0;
    const int slots_per_cu = rq.slots_per_cu, diag_cost_pct = rq.diag_cost_pct;
    int min_chunks = rq.min_chunks;
    struct T { uint16_t I, J; bool diag; };
    std::vector<T> tiles;
    // groups of 4 x 8 neighbouring tiles first (they share rows), the tiles on the diagonal last
    for (int pass = 0; pass < 2; ++pass)
        for (uint32_t gi = ia0; gi < ia1; gi += 4)
            for (uint32_t gj = jb0; gj < jb1; gj += 8)
                for (uint32_t i = gi; i < std::min(gi + 4, ia1); ++i)
                    for (uint32_t j = gj; j < std::min(gj + 8, jb1); ++j) {
                        if (triangle && j < i) continue;
                        // lag limit: the tile's nearest pair is (128 i + 127, 128 j): j <= (128 i + 127 + lag) / 128
                        if (triangle && rq.lag && (uint64_t)j > ((uint64_t)kThTile * i + kThTile - 1u + rq.lag) / kThTile) continue;
                        const bool diag = triangle && j == i;
                        if (diag != (pass == 1)) continue;
                        tiles.push_back({(uint16_t)i, (uint16_t)j, diag});
                    }
    const uint32_t nC = total_stages / 4u;
    plan->n_tiles = (uint32_t)tiles.size();
    plan->n_windows = 0;
    plan->items.clear();
    if (tiles.empty() || nC == 0) return;
    // f32 accumulators: an item's chunks x weight stay at or below 2^24 (bits: 32767 chunks, below 2^24 bits of k;
    // 2-bit values: 7281 chunks)
    const uint32_t weight = std::max(rq.chunk_weight, 1u);
    const uint32_t kMaxExactChunks = ((1u << 24) - 1u) / weight;
    const uint32_t max_narrow_chunks = 65535u / weight;   // 16-bit windows: 127 chunks of bits, 28 of 2-bit values
    constexpr double kItemChunks = 5.0;                             // what an item costs besides its chunks, in chunks
    min_chunks = std::max(min_chunks, (int)(nC / 32000u) + 1);      // (a tile has fewer than 2^15 parts: PartItem::part)
    const uint32_t min_parts = (nC + kMaxExactChunks - 1) / kMaxExactChunks;
    const uint32_t max_parts = std::max(min_parts, nC / (uint32_t)min_chunks);
    const size_t nT = tiles.size();
    std::vector<uint32_t> parts_of(nT), best_parts;
    double best_load = 0;
    for (int spc = 1; spc <= 2; ++spc) {
        if (slots_per_cu > 0 && spc != slots_per_cu) continue;
        const size_t slots = (size_t)n_cus * spc;
        const double dcost = spc >= 2 ? diag_cost_pct / 100.0 : 1.0;
        auto cost_of = [&](size_t t) { return tiles[t].diag ? dcost : 1.0; };
        const size_t n_whole = min_parts > 1 ? 0 : nT / slots * slots;
        std::fill(parts_of.begin(), parts_of.end(), 1u);
        double rest = 0;
        for (size_t t = n_whole; t < nT; ++t) rest += cost_of(t) * nC;
        const double seg = rest / (double)slots;
        size_t n_items = n_whole;
        for (size_t t = n_whole; t < nT; ++t)
            n_items += parts_of[t] = std::min(max_parts, std::max(min_parts, (uint32_t)(cost_of(t) * nC / std::max(seg, 1e-9))));
        while (n_items < n_whole + slots) {   // the slots left over: to the tiles whose parts are longest
            size_t best = nT;
            double longest = 0;
            for (size_t t = n_whole; t < nT; ++t) {
                const double len = cost_of(t) * nC / parts_of[t];
                if (parts_of[t] < max_parts && len > longest) longest = len, best = t;
            }
            if (best == nT) break;
            ++parts_of[best];
            ++n_items;
        }
        double longest = 0;
        for (size_t t = n_whole; t < nT; ++t) longest = std::max(longest, cost_of(t) * std::ceil((double)nC / parts_of[t]));
        // a CU's load: its slots' whole tiles and one part each, and what its items cost besides
        const double load = spc * ((double)(n_whole / slots) * nC + longest) + kItemChunks * (double)n_items / n_cus;
        if (best_parts.empty() || load < best_load) best_load = load, best_parts = parts_of;
    }
    for (uint32_t t = 0; t < nT; ++t) {
        const uint32_t np = best_parts[t];
        // windows of 16-bit counts while every part of the tile stays below 2^16 (bits: 127 chunks of k)
        const uint16_t narrow = (np > 1 && (nC + np - 1) / np <= max_narrow_chunks && narrow_windows) ? kThNarrow : (uint16_t)0;
        for (uint32_t p = 0; p < np; ++p) {
            const uint32_t c0 = (uint32_t)((uint64_t)nC * p / np), c1 = (uint32_t)((uint64_t)nC * (p + 1) / np);
            plan->items.push_back({tiles[t].I, tiles[t].J, c0 * 4u, (c1 - c0) * 4u, t, np > 1 ? plan->n_windows : 0u,
                                   (uint16_t)((uint16_t)p | narrow), (uint16_t)np});
        }
        if (np > 1) plan->n_windows += np;
    }
    std::stable_sort(plan->items.begin(), plan->items.end(),
                     [](const PartItem& a, const PartItem& b) { return a.n_stages > b.n_stages; });
}

// ---- K2q work decomposition: the stage stream of bitstream_kernel, cut into equal shares ----
// `groups` workgroups; workgroup w walks segs[first[w] .. first[w+1]).
BitstreamRequest bitstream_request(const BitstreamShaping& sh, const std::vector<RowRange>& ranges, uint32_t n_kslices,
                                   uint32_t shard_rank, uint32_t shard_count, uint32_t n_cus, uint64_t pitch_bytes) {
    return {sh, n_kslices, shard_rank, shard_count, n_cus, pitch_bytes, ranges_hash(ranges)};
}
void build_bitstream(const BitstreamRequest& rq, const std::vector<RowRange>& ranges, BitstreamPlan& plan) {
    const BitstreamShaping& sh = rq.sh;
    const uint32_t n_kslices = rq.n_kslices, shard_rank = rq.shard_rank, shard_count = rq.shard_count, n_cus = rq.n_cus;
    const uint64_t pitch_bytes = rq.pitch_bytes;
    // natural segments, k-slice major: every A tile of every range with the later tiles dealt cyclically
    struct Nat {
        BitSeg s;
        uint64_t start;  // position of its first stage in the stream
    };
    std::vector<Nat> nat;
    uint64_t L = 0;
    for (uint32_t ks = 0; ks < n_kslices; ++ks)
        for (const RowRange& rg : ranges) {
            if (rg.r1 < rg.r0 + 2) continue;
            const uint32_t b0 = (uint32_t)(rg.r0 / kStripBRows);
            const uint32_t nb = (uint32_t)((rg.r1 - rg.r0 + kStripBRows - 1) / kStripBRows);
            const uint32_t nT = (nb + 3u) / 4u;
            auto blocks_of = [&](uint32_t J) { return std::min(4u, nb - 4u * J); };
            for (uint32_t I = 0; I < nT; ++I) {
                // tile I takes the (nT - 1) / 2 tiles behind it (cyclically); with an even number of
                // tiles the opposite one goes to the lower tile on even k-slices, to the upper on odd ones
                uint32_t take = (nT - 1u) / 2u;
                if (nT > 1u && nT % 2u == 0u && ((I < nT / 2u) == ((ks & 1u) == 0u))) ++take;
                uint32_t n_b = 0;
                for (uint32_t d = 1; d <= take; ++d) n_b += blocks_of((I + d) % nT);
                BitSeg s = {};
                s.a_blk = b0 + 4u * I;
                s.ks = ks;
                s.b_first = (I + 1u == nT) ? 0u : 4u * (I + 1u);
                s.n_b = n_b;
                s.range_b0 = b0;
                s.range_nb = nb;
                s.flags = kBsDiag | (((I + ks) & 3u) << 8);
                nat.push_back({s, L});
                L += 4u + n_b;
            }
        }
    plan.segs.clear();
    plan.first.clear();
    plan.bases.clear();
    plan.first_stage.clear();
    plan.stages = 0;
    plan.max_stages = 0;
    // this shard's part of the stream (contiguous: a shard touches a contiguous range of k-slices)
    const uint64_t lo = L * shard_rank / shard_count, hi = L * (shard_rank + 1ull) / shard_count;
    const uint64_t Ls = hi - lo;
    // workgroups: as many per CU as the share of a CU is worth cutting, and never a workgroup
    // beyond the accumulators' exact range
    uint32_t per_cu = (uint32_t)sh.groups_per_cu;
    if (per_cu == 0) {
        const uint64_t share = Ls / std::max(1u, n_cus);
        per_cu = share >= 3ull * (uint64_t)sh.min_piece ? 3u : share >= 2ull * (uint64_t)sh.min_piece ? 2u : 1u;
    }
    uint64_t G = (uint64_t)n_cus * per_cu;
    // A long stream is cut into MORE shares than the chip holds workgroups (three per CU): the waves of a SIMD
    // do not advance evenly (its arbiter prefers the oldest), so equal shares end at very different times and
    // the last ones run alone, at a lone wave's 60 % of the pipe; with shares of ~80 stages a CU that finishes
    // one early simply gets the next (headline shape: 883 us with 768 shares, 821 with 6144; N = 6144: 341 ->
    // 317; from ~30 stages down the four stages that bring a continued segment's A rows in cost more than the
    // tail does: N = 2048 is fastest with 768). Never a share beyond the accumulators' exact range.
    // Whole rounds of the chip's slots only: 870 shares on 768 slots leave a fourth share to 102 CUs (N = 4096:
    // 185 us against 152 with 768 or 1536).
    if (sh.groups_per_cu == 0 && per_cu == 3u) {
        const uint64_t slots = (uint64_t)n_cus * 3u;
        const uint64_t rounds = (Ls + slots * (uint64_t)std::max(1, sh.long_piece) / 2) /
                                (slots * (uint64_t)std::max(1, sh.long_piece));
        // up to ~220 stages per slot ONE round of weighted shares (below) is faster than the dynamic deal, which
        // pays four operand-only stages per cut (N = 6144: 308 against 314 us; N = 8192: 545 against 538)
        G = slots * (Ls <= slots * (uint64_t)sh.single_round_max ? 1ull : std::max<uint64_t>(1, rounds));
    }
    G = std::max<uint64_t>(G, (Ls + kBsMaxStages / 2 - 1) / (kBsMaxStages / 2));
    G = std::max<uint64_t>(1, std::min<uint64_t>(G, std::max<uint64_t>(1, Ls / 4)));
    if (Ls == 0) G = 0;
    plan.groups = (uint32_t)G;
    if (G == 0) {
        plan.first.push_back(0);
        plan.first_stage.push_back(0);
        return;
    }
    // cut positions, snapped: never inside a tile's own four stages, never leaving a stub of a run
    auto seg_at = [&](uint64_t p) {  // natural segment holding stream position p (< L)
        size_t a = 0, b = nat.size();
        while (b - a > 1) {
            const size_t m = (a + b) / 2;
            if (nat[m].start <= p) a = m; else b = m;
        }
        return a;
    };
    // Shares of ONE round are not equal. The waves of a SIMD do not take turns: its arbiter issues for the oldest
    // wave that can go, and a wave alone reaches ~60 % of the matrix pipe (one instruction every four cycles). Of
    // three equal shares per CU the first-dispatched workgroup ends after 0.55 of the kernel, the second at 0.75,
    // the third runs the last quarter nearly alone (N = 2048: 24 / 33 / 42 us; tools/archive/stream_trace.py, end by
    // dispatch round; workgroup w is dispatched in round w / n_cus, one per CU per round). Shares in the proportion
    // 100 : 120 : 60 let the three end closer together: -3 % at N = 2048, -6 % at 3072 ... 4096, -2 % at 6144
    // against the dynamic deal (profiles/r03_e_stream_weights.txt; the optimum is flat: 100 : 100 : 50 and
    // 100 : 125 : 65 are within 1 %). Shares shorter than ~16 stages keep equal lengths: start-up and drain
    // dominate them, and whole segments as shares (no cut, no operand-only stages, but two workgroups per CU) lose
    // 15 % at N = 1024.
    std::vector<uint32_t> weight(G, 100u);
    if (G == (uint64_t)n_cus * 3u && n_cus % 8u == 0u && Ls >= G * (uint64_t)sh.weighted_min) {
        const uint32_t wr[3] = {100u, (uint32_t)sh.w3_1, (uint32_t)sh.w3_2};
        for (uint64_t p = 0; p < G; ++p) weight[p] = std::max(1u, wr[(p % (G / 8)) / (n_cus / 8u)]);
    }
    std::vector<uint64_t> cum(G + 1, 0);
    for (uint64_t p = 0; p < G; ++p) cum[p + 1] = cum[p] + weight[p];
    std::vector<uint64_t> cut(G + 1);
    for (uint64_t k = 0; k <= G; ++k) {
        uint64_t c = lo + (uint64_t)((unsigned __int128)Ls * cum[k] / cum[G]);
        if (c < L) {
            const Nat& n = nat[seg_at(c)];
            const uint64_t off = c - n.start, len = 4ull + n.s.n_b;
            if (off > 0 && off < 4ull + (uint64_t)sh.min_run) c = n.start;
            else if (off > 0 && len - off < (uint64_t)sh.min_run) c = n.start + len;
        }
        cut[k] = c;
    }
    for (uint64_t k = 1; k <= G; ++k) cut[k] = std::max(cut[k], cut[k - 1]);
    // piece p of the stream goes to workgroup w with p = (w % 8) * (G / 8) + w / 8: block w runs on XCD
    // w % 8 (observed; speed only), so an XCD's workgroups hold one contiguous eighth of the stream
    std::vector<uint32_t> piece_of(G);
    for (uint64_t w = 0; w < G; ++w) piece_of[w] = (uint32_t)(G % 8 == 0 ? (w % 8) * (G / 8) + w / 8 : w);
    for (uint64_t w = 0; w < G; ++w) {
        const uint64_t p = piece_of[w];
        plan.first.push_back((uint32_t)plan.segs.size());
        uint64_t c0 = cut[p], c1 = cut[p + 1];
        uint32_t mine = 0;
        while (c0 < c1) {
            const Nat& n = nat[seg_at(c0)];
            const uint64_t len = 4ull + n.s.n_b, off = c0 - n.start;
            const uint64_t end = std::min(c1, n.start + len);
            BitSeg s = n.s;
            if (off == 0) {
                s.n_b = (uint32_t)(end - n.start - 4ull);
            } else {  // continues a cut segment: its four blocks only bring the A rows in
                const uint32_t skip = (uint32_t)(off - 4ull);
                s.flags &= ~kBsDiag;
                s.b_first = (n.s.b_first + skip) % n.s.range_nb;
                s.n_b = (uint32_t)(end - c0);
            }
            plan.segs.push_back(s);
            mine += 4u + s.n_b;
            c0 = end;
        }
        plan.stages += mine;
        plan.max_stages = std::max(plan.max_stages, mine);
    }
    plan.first.push_back((uint32_t)plan.segs.size());
    // the DMA's view of the same stream: the start of every stage's 64 rows x 64 B, in 64-byte units from the
    // matrix ((ks * 64 + blk * 64 * pitch) / 64; the pitch is a multiple of 64 bytes)
    plan.bases.reserve(plan.stages);
    for (uint64_t w = 0; w < G; ++w) {
        plan.first_stage.push_back((uint32_t)plan.bases.size());
        for (uint32_t si = plan.first[w]; si < plan.first[w + 1]; ++si) {
            const BitSeg& sg = plan.segs[si];
            for (uint32_t i = 0; i < 4u + sg.n_b; ++i) {
                uint32_t blk;
                if (i < 4u) {
                    blk = sg.a_blk + i;
                } else {
                    uint32_t rel = sg.b_first + (i - 4u);
                    if (rel >= sg.range_nb) rel -= sg.range_nb;
                    blk = sg.range_b0 + rel;
                }
                plan.bases.push_back((uint32_t)((uint64_t)sg.ks + (uint64_t)blk * pitch_bytes));
            }
        }
    }
    plan.first_stage.push_back((uint32_t)plan.bases.size());
}

// ---- the sparse arena ----
static int64_t steady_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
ArenaLaps::ArenaLaps() : t0_ns(steady_ns()) {}
void ArenaLaps::lap(const char* what) {
    if (!timing_env()) return;
    const int64_t t = steady_ns();
    fprintf(stderr, "[build_arena] %-28s %8.1f ms\n", what, (double)(t - t0_ns) * 1e-6);
    t0_ns = t;
}

// The texts and codes of storm_hip_sparse_create*; max_id: the largest block id.
static int check_arena_blocks(const ArenaBlocks& in, uint32_t* max_id_out) {
    const uint64_t n_rows = in.n_rows, n_blocks = in.n_blocks;
    const uint64_t* const row_block_offset = in.row_block_offset;
    const uint32_t* const block_id = in.block_id;
    const uint8_t* const block_kind = in.block_kind;
    const uint32_t* const block_n = in.block_n;
    const void* const* const block_ptr = in.block_ptr;
    if (n_blocks > 0 && (!row_block_offset || !block_id || !block_kind || !block_ptr || !block_n)) {
        set_error("sparse_create: NULL descriptor array");
        return STORM_HIP_EINVAL;
    }
    if (n_blocks >= (1ull << 32) - kABlockRows) {
        set_error("sparse_create: too many blocks");
        return STORM_HIP_EINVAL;
    }
    // ---- validate + count blocks per column ----
    if (n_blocks > 0 && n_rows == 0) {
        set_error("sparse_create: %llu blocks but no rows", (unsigned long long)n_blocks);
        return STORM_HIP_EINVAL;
    }
    if (n_rows > 0 && (!row_block_offset || row_block_offset[0] != 0 || row_block_offset[n_rows] != n_blocks)) {
        set_error("sparse_create: row_block_offset must run from 0 to n_blocks = %llu", (unsigned long long)n_blocks);
        return STORM_HIP_EINVAL;
    }
    uint32_t max_id = 0;
    for (uint64_t r = 0; r < n_rows; ++r) {
        if (row_block_offset[r] > row_block_offset[r + 1] || row_block_offset[r + 1] > n_blocks) {
            set_error("sparse_create: row_block_offset is not a CSR over %llu blocks", (unsigned long long)n_blocks);
            return STORM_HIP_EINVAL;
        }
        for (uint64_t b = row_block_offset[r]; b < row_block_offset[r + 1]; ++b) {
            if (b > row_block_offset[r] && block_id[b] <= block_id[b - 1]) {
                set_error("sparse_create: block ids of row %llu are not ascending", (unsigned long long)r);
                return STORM_HIP_EINVAL;
            }
            if (block_id[b] >= kMaxBlockId) {  // positions are uint32: ids stop at 2^32 / 65536
                set_error("sparse_create: block id %u out of range", block_id[b]);
                return STORM_HIP_EINVAL;
            }
            if (block_kind[b] > 1) {
                set_error("sparse_create: block kind %u", block_kind[b]);
                return STORM_HIP_EINVAL;
            }
            if (block_kind[b] == 0 ? (block_n[b] > 65536u || (block_n[b] && (!block_ptr[b] || ((uintptr_t)block_ptr[b] & 1))))
                                   : !block_ptr[b]) {
                set_error("sparse_create: block %llu has no data (or a list that is too long or not 2-byte aligned)",
                          (unsigned long long)b);
                return STORM_HIP_EINVAL;
            }
            max_id = std::max(max_id, block_id[b]);
        }
    }
    *max_id_out = max_id;
    return STORM_HIP_OK;
}

int plan_arena_columns(const ArenaBlocks& in, ArenaColumns* cols, ArenaRows* rows, ArenaLaps& laps) {
    uint32_t max_id = 0;
    if (int rc = check_arena_blocks(in, &max_id)) return rc;
    const uint64_t n_blocks = in.n_blocks;
    const uint32_t* const block_id = in.block_id;
    const uint8_t* const block_kind = in.block_kind;
    const uint32_t* const block_n = in.block_n;
    std::vector<uint64_t> per_col((size_t)max_id + 2, 0), n_list_col((size_t)max_id + 2, 0);
    for (uint64_t b = 0; b < n_blocks; ++b) {
        per_col[block_id[b]]++;
        if (block_kind[b] == 0) n_list_col[block_id[b]]++;
    }
    // Which columns the list-probe kernel (K4) can take: all blocks lists, 2 .. 65535 rows, element offsets
    // within 32 bits (8 octants x up to 7 elements of alignment each). Their pool rows come LAST in the
    // layout and are not materialised at all unless a dense pass over them is asked for (sparse_probe = 0,
    // the popcount variants): a column of short lists costs its listed positions, not 8 KiB per block.
    std::vector<uint64_t> col_elems((size_t)max_id + 2, 0);
    for (uint64_t b = 0; b < n_blocks; ++b)
        if (block_kind[b] == 0) col_elems[block_id[b]] += block_n[b];
    std::vector<uint8_t> probe_c((size_t)max_id + 2, 0);
    {
        uint64_t total = 0;
        for (uint32_t c = 0; c <= max_id; ++c) {
            const uint64_t n_l = n_list_col[c];
            if (n_l >= 2 && n_l <= 65535 && col_elems[c] > 0 && total + col_elems[c] + 64 < (1ull << 32) - (1u << 20)) {  // (the probe kernel's element indices run up to 12 x 8192 past an item's end)
                probe_c[c] = 1;
                total += col_elems[c] + 64;
            }
        }
    }
    // Layout of a column: its bitmap blocks, then — on the next multiple of 512 rows — its list blocks (the kind
    // dispatch of storm.c:618-656, once per block: list x list pairs go to the probe kernel, every pair with a
    // bitmap block to the matrix cores, which then need the bitmap rows alone as A rows). Columns made of lists
    // only come last: they need no pool rows at all.
    std::vector<uint64_t> start((size_t)max_id + 2, 0), list0((size_t)max_id + 2, 0), col_end((size_t)max_id + 2, 0);
    uint64_t run = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (uint32_t c = 0; c <= max_id; ++c) {
            const bool lists_only = probe_c[c] && n_list_col[c] == per_col[c];
            if (per_col[c] && (int)lists_only == pass) {
                const uint64_t n_b = per_col[c] - n_list_col[c];
                start[c] = run;
                list0[c] = n_b && n_list_col[c] ? (run + n_b + 511) / 512 * 512 : run + n_b;
                col_end[c] = list0[c] + n_list_col[c];
                run = (col_end[c] + 511) / 512 * 512;  // next column starts on a 512-row A tile
            }
        }
        if (pass == 0) cols->pool_rows_ready = run;
    }
    for (uint32_t c = 0; c <= max_id; ++c)
        if (per_col[c]) {
            cols->cols.push_back({start[c], col_end[c]});
            cols->col_list0.push_back(list0[c]);
            const uint64_t nl = n_list_col[c], nb = per_col[c] - nl;
            cols->census[0] += nl * (nl - (nl != 0)) / 2;
            cols->census[1] += nl * nb;
            cols->census[2] += nb * (nb - (nb != 0)) / 2;
            cols->census[3] += 1;
        }
    cols->n_pool_rows = run;
    if (cols->n_pool_rows >= (1ull << 32) - 512) {
        set_error("sparse_create: block pool too large");
        return STORM_HIP_EINVAL;
    }

    laps.lap("validate");
    // ---- pool row of every block (rows are visited in order => row order inside a column)
    std::vector<uint32_t>&list_row = rows->list_row, &dense_row = rows->dense_row, &list_len = rows->list_len;
    std::vector<uint64_t>&list_blk = rows->list_blk, &dense_blk = rows->dense_blk;   // the blocks behind those rows
    {
        std::vector<uint64_t> next_bitmap(start), next_list(list0);
        for (uint64_t b = 0; b < n_blocks; ++b) {
            const uint32_t pr = (uint32_t)(block_kind[b] == 0 ? next_list[block_id[b]]++ : next_bitmap[block_id[b]]++);
            if (block_kind[b] == 0) {
                if (block_n[b] && pr < cols->pool_rows_ready) {
                    list_row.push_back(pr);
                    list_blk.push_back(b);
                    list_len.push_back(block_n[b]);
                }
            } else {
                dense_row.push_back(pr);
                dense_blk.push_back(b);
            }
        }
    }
    // ---- probe data (K4): columns whose blocks are all lists and that have at most 65535 rows
    std::vector<uint64_t>& probe_blocks = rows->probe_blocks;
    for (uint64_t b = 0; b < n_blocks; ++b)
        if (block_kind[b] == 0 && probe_c[block_id[b]]) probe_blocks.push_back(b);
    {
        std::vector<int64_t>& col_entry = rows->col_entry;
        col_entry.assign((size_t)max_id + 2, -1);  // column id -> index into cols->cols
        cols->col_probe.assign(cols->cols.size(), 0);
        cols->col_avg_len.assign(cols->cols.size(), 0);
        size_t entry = 0;
        for (uint32_t c = 0; c <= max_id; ++c) {
            if (!per_col[c]) continue;
            col_entry[c] = (int64_t)entry;
            if (probe_c[c]) {
                cols->col_probe[entry] = 1;
                cols->col_avg_len[entry] = (uint32_t)(col_elems[c] / n_list_col[c]);
            }
            ++entry;
        }
    }
    return STORM_HIP_OK;
}

namespace {

// One (probe column, octant) stream: the elements of the column's list rows in that octant, in row order. Atom t is the
// part of rows [128 t, 128 t + 128): the group of those rows reads it as its own elements, every group in front of it as
// far positions.
struct ProbeStream {
    std::vector<uint32_t> row_start;   // first element of every list row of the column, then the end of the octant
    uint32_t col = 0;                  // index into ArenaColumns::cols
    uint32_t n_rows() const { return (uint32_t)row_start.size() - 1u; }
    uint32_t n_atoms() const { return (n_rows() + kProbeRows - 1) / kProbeRows; }
    uint32_t atom_start(uint32_t t) const { return row_start[std::min(t * kProbeRows, n_rows())]; }
    uint32_t end() const { return row_start.back(); }
};

// a list that is not ascending may give ends that run backwards: refused here, before they are laid out
// (ascending ends that disagree with the values are caught by probe_fill_kernel)
int check_run_ends(const ArenaBlocks& in, const std::vector<uint64_t>& probe_blocks, const std::vector<uint32_t>& run_end) {
    for (size_t pb = 0; pb < probe_blocks.size(); ++pb) {
        uint32_t from = 0;
        for (uint32_t o = 0; o < kProbeOctants; ++o) {
            const uint32_t end = run_end[pb * kProbeOctants + o];
            if (end < from || end > in.block_n[probe_blocks[pb]]) {
                set_error("sparse_create: a list block is not strictly ascending");
                return STORM_HIP_EINVAL;
            }
            from = end;
        }
    }
    return STORM_HIP_OK;
}

// Where every run of a list goes: count per (probe column, octant), the octants one after the other, each on a 16-byte
// boundary of the uint16 position array; then, rows visited in order, the element offset of every row per octant.
std::vector<ProbeStream> lay_out_streams(const ArenaBlocks& in, const ArenaColumns& cols, const ArenaRows& rows,
                                         const std::vector<uint32_t>& run_end, ProbeWork* work, ProbeLayout* layout) {
    constexpr uint32_t kNoBlock = 0xffffffffu;
    const std::vector<uint64_t>& probe_blocks = rows.probe_blocks;
    const size_t n_e = cols.cols.size();
    std::vector<uint64_t> oct_count(n_e * kProbeOctants, 0), oct_base(n_e * kProbeOctants, 0);
    layout->run_dst.assign(probe_blocks.size() * kProbeOctants, 0);
    layout->block_local.assign(probe_blocks.size(), kNoBlock);
    for (size_t pb = 0; pb < probe_blocks.size(); ++pb) {
        const size_t e = (size_t)rows.col_entry[in.block_id[probe_blocks[pb]]];
        uint32_t from = 0;
        for (uint32_t o = 0; o < kProbeOctants; ++o) {
            oct_count[e * kProbeOctants + o] += run_end[pb * kProbeOctants + o] - from;
            from = run_end[pb * kProbeOctants + o];
        }
    }
    uint64_t at = 0;
    for (size_t i = 0; i < oct_count.size(); ++i) {
        at = (at + 7) & ~7ull;
        oct_base[i] = at;
        at += oct_count[i];
    }
    layout->n_probe_elems = (size_t)at + 8;
    for (size_t i = 0; i < oct_count.size(); ++i)
        if (oct_count[i])
            work->probe_regions.push_back({(uint32_t)oct_base[i], (uint32_t)(oct_base[i] + oct_count[i]),
                                           (uint32_t)cols.col_list0[i / kProbeOctants], (uint32_t)(i % kProbeOctants)});
    std::vector<uint64_t> cursor(oct_base);
    std::vector<uint64_t> next(rows.col_entry.size(), 0);  // list blocks of the column seen so far
    std::vector<ProbeStream> streams(n_e * kProbeOctants);
    for (size_t e = 0; e < n_e; ++e)
        if (cols.col_probe[e])
            for (uint32_t o = 0; o < kProbeOctants; ++o)
                streams[e * kProbeOctants + o].row_start.reserve((size_t)(cols.cols[e].r1 - cols.col_list0[e]) + 1);
    size_t pb = 0;
    for (uint64_t b = 0; b < in.n_blocks; ++b) {
        if (in.block_kind[b] != 0) continue;
        const uint32_t c = in.block_id[b];
        const uint64_t local = next[c]++;
        const int64_t e = rows.col_entry[c];
        if (e < 0 || !cols.col_probe[(size_t)e]) continue;
        layout->block_local[pb] = (uint32_t)local;
        uint32_t from = 0;
        for (uint32_t o = 0; o < kProbeOctants; ++o) {
            const size_t i = (size_t)e * kProbeOctants + o;
            streams[i].row_start.push_back((uint32_t)cursor[i]);
            layout->run_dst[pb * kProbeOctants + o] = (uint32_t)cursor[i];
            cursor[i] += run_end[pb * kProbeOctants + o] - from;
            from = run_end[pb * kProbeOctants + o];
        }
        ++pb;
    }
    // the streams of the probe columns, each closed by the end of its octant
    std::vector<ProbeStream> out;
    for (size_t i = 0; i < streams.size(); ++i)
        if (!streams[i].row_start.empty()) {
            streams[i].row_start.push_back((uint32_t)(oct_base[i] + oct_count[i]));
            streams[i].col = (uint32_t)(i / kProbeOctants);
            out.push_back(std::move(streams[i]));
        }
    return out;
}

// The items that read one chunk of a stream; the families of a launch and their deal onto the XCDs.
template <class Item>
struct Families {
    struct Family {
        uint64_t work = 0;
        uint32_t col = 0;
        std::vector<Item> items;
    };
    std::vector<Family> families;

    // families to XCDs: heaviest first onto the lightest queue; block b of the launch runs on XCD b % 8
    // (observed; speed only), so the launch order takes one item of every queue in turn
    void deal(std::vector<Item>* items, std::vector<uint32_t>* item_col) const {
        std::vector<size_t> order(families.size());
        for (size_t f = 0; f < order.size(); ++f) order[f] = f;
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return families[x].work > families[y].work; });
        std::vector<Item> queue[8];
        std::vector<uint32_t> queue_col[8];
        uint64_t load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (size_t f : order) {
            if (families[f].items.empty()) continue;
            int q = 0;
            for (int x = 1; x < 8; ++x)
                if (load[x] < load[q]) q = x;
            queue[q].insert(queue[q].end(), families[f].items.begin(), families[f].items.end());
            queue_col[q].insert(queue_col[q].end(), families[f].items.size(), families[f].col);
            load[q] += families[f].work;
        }
        size_t longest = 0;
        for (int x = 0; x < 8; ++x) longest = std::max(longest, queue[x].size());
        for (size_t pos = 0; pos < longest; ++pos)
            for (int x = 0; x < 8; ++x)
                if (pos < queue[x].size()) {
                    items->push_back(queue[x][pos]);
                    item_col->push_back(queue_col[x][pos]);
                }
    }
};

// The items of one stream, `per_item` groups to an item. chunk_first: the first atom of every chunk of the stream's grid,
// then n_atoms — the grid runs over atoms 1 .. (atom 0 is nobody's far part). An item's groups need the rest of the chunk
// their successor atom lies in and every later chunk: the first item of the groups takes their own pairs too, one item
// follows per later chunk; groups with nobody behind them go to the stream's last family. make(stream, g0, g1, first,
// b0, b1, &item) fills the item of groups [g0, g1) with the far piece [min(b0, b1), b1) and says whether it is needed.
template <class Item, class Make>
void plan_stream_items(const ProbeStream& st, const std::vector<uint32_t>& chunk_first, uint32_t per_item,
                       Families<Item>* fams, Make make) {
    const uint32_t n_atoms = st.n_atoms();
    const size_t fam0 = fams->families.size();
    fams->families.resize(fam0 + chunk_first.size());  // one per chunk (+ one for groups without a far part)
    for (size_t f = fam0; f < fams->families.size(); ++f) fams->families[f].col = st.col;
    auto emit = [&](size_t c, uint32_t g0, uint32_t g1, bool first, uint32_t b0, uint32_t b1) {
        Item it{};
        if (!make(st, g0, g1, first, b0, b1, &it)) return;
        fams->families[fam0 + c].items.push_back(it);
        // every item pays for the histograms of its groups
        fams->families[fam0 + c].work += (uint64_t)(b1 - std::min(b0, b1)) * (g1 - g0) + 8192u * (g1 - g0);
    };
    for (uint32_t g0 = 0; g0 < n_atoms; g0 += per_item) {
        const uint32_t g1 = std::min(g0 + per_item, n_atoms);
        const uint32_t own_end = st.atom_start(g1);
        if (own_end == st.atom_start(g0)) continue;  // no listed position of these rows in this octant
        if (g1 >= n_atoms) {  // the last groups have nobody behind them
            emit(chunk_first.size() - 1, g0, g1, true, own_end, own_end);
            continue;
        }
        size_t c = 0;
        while (c + 1 < chunk_first.size() && chunk_first[c + 1] <= g1) ++c;
        for (bool first = true; c + 1 < chunk_first.size(); ++c, first = false)
            emit(c, g0, g1, first, first ? own_end : st.atom_start(chunk_first[c]), st.atom_start(chunk_first[c + 1]));
    }
}

// probe_lists_kernel: one group per item; its first item carries the near range
bool make_thin_item(const ProbeStream& st, uint32_t g0, uint32_t g1, bool first, uint32_t b0, uint32_t b1, ProbeItem* it) {
    const uint32_t a_begin = st.atom_start(g0), a_end = st.atom_start(g1);
    const uint32_t n0 = first ? a_begin : 0u, n1 = first ? a_end : 0u;
    *it = {a_begin, a_end, n0, n1, std::min(b0, b1), b1, g0 * kProbeRows};
    return n1 > n0 || b1 > b0;
}
// [r6] probe_lists_fat_kernel: the same work in bundles of kFatGroups groups — atoms at[k] .. at[k + 1] of the groups of
// the bundle, the far piece, first = the bundle's near parts are this item's
bool make_fat_item(const ProbeStream& st, uint32_t g0, uint32_t g1, bool first, uint32_t b0, uint32_t b1, ProbeFatItem* it) {
    for (uint32_t k = 0; k <= kFatGroups; ++k) it->at[k] = st.atom_start(std::min(g0 + k, g1));
    it->b_begin = std::min(b0, b1);
    it->b_end = b1;
    it->first = first ? 1u : 0u;
    return first || b1 > it->b_begin;
}

}  // namespace

int plan_arena_probe(const ArenaBlocks& in, const ArenaColumns& cols, const ArenaRows& rows, const std::vector<uint32_t>& run_end,
                     ProbeWork* work, ProbeLayout* layout, ArenaLaps& laps) {
    if (int rc = check_run_ends(in, rows.probe_blocks, run_end)) return rc;
    if (rows.probe_blocks.empty()) return STORM_HIP_OK;
    const std::vector<ProbeStream> streams = lay_out_streams(in, cols, rows, run_end, work, layout);
    laps.lap("layout (prefix sums, row starts)");
    // atoms of the far stream (the elements of one group of kProbeRows rows in one octant): the device deals
    // the positions of every atom by LDS bank (probe_deal_kernel; why: see there)
    // far work of all groups -> positions per item: about 4096 items over all probe columns, between
    // 2^15 and 2^21 positions each (an item zeroes and scatters its 128 KiB table first)
    uint64_t far_work = 0;
    for (const ProbeStream& st : streams)
        for (uint32_t t = 0; t < st.n_atoms(); ++t) {
            layout->atoms.push_back(st.atom_start(t));
            layout->atoms.push_back(st.atom_start(t + 1));
            far_work += st.end() - st.atom_start(t + 1);
        }
    // Chunks of the far stream are the SAME for every group of a (column, octant) stream: a fixed grid of runs
    // of atoms, ~far_work / 2048 positions each and at most 2^23. A group needs the rest of the chunk its own
    // atom lies in and every later chunk. The items that read one chunk are a FAMILY; a family goes to one XCD,
    // its items one after the other, so that the XCD's 32 CUs work through the same positions at the same time
    // and HBM delivers them once (the kernel fetched 16 GB per launch at c4's 20971 draws — every group
    // streaming its own 4 MiB chunks through an L2 that hit 9 % of the time — and ran at the HBM rate with the
    // LDS half idle). Every item pays for its group's histogram, so fewer, longer items win as long as the
    // 512 workgroup slots stay filled: / 4096 and 2^21 until round 4; / 2048 is 8 - 18 % faster at every c4
    // load and 2^23 another 7 % at 30000 draws (profiles/r04_h_sparse_probe.txt).
    const uint64_t kProbeChunk =
        std::min<uint64_t>(1u << 23, std::max<uint64_t>(1u << 15, far_work / 2048)) & ~7ull;
    Families<ProbeItem> thin;
    Families<ProbeFatItem> fat;   // the same chunk grid, the same families and queues
    std::vector<uint32_t> chunk_first;
    for (const ProbeStream& st : streams) {
        chunk_first.clear();
        for (uint32_t t = 1; t < st.n_atoms();) {
            chunk_first.push_back(t);
            const uint64_t from = st.atom_start(t);
            ++t;
            while (t < st.n_atoms() && st.atom_start(t) - from < kProbeChunk) ++t;
        }
        chunk_first.push_back(st.n_atoms());
        plan_stream_items(st, chunk_first, 1u, &thin, make_thin_item);
        plan_stream_items(st, chunk_first, kFatGroups, &fat, make_fat_item);
    }
    thin.deal(&work->items, &work->item_col);
    fat.deal(&work->fat_items, &work->fat_col);
    return STORM_HIP_OK;
}

// lookups of an item: a streamed far position against every group of the item + the own rows' elements (against
// their own group and, in a bundle, the groups in front of it)
static uint64_t item_lookups(const ProbeItem& it) { return (uint64_t)(it.b_end - it.b_begin) + (it.n_end - it.n_begin); }
static uint64_t item_lookups(const ProbeFatItem& it) {
    uint64_t lookups = 0;
    uint32_t groups = 0;
    for (uint32_t g = 0; g < kFatGroups; ++g) {
        const uint32_t len = it.at[g + 1] - it.at[g];
        groups += len != 0;
        if (it.first) lookups += (uint64_t)len * (g + 1u);
    }
    return lookups + (uint64_t)(it.b_end - it.b_begin) * groups;
}
template <class Item>
static void plan_launch_of(const std::vector<Item>& all, const std::vector<uint32_t>& col, const ProbeLaunchRequest& rq,
                           std::vector<Item>* mine, ProbeLaunchPlan* plan) {
    for (size_t k = 0; k < all.size(); ++k)
        if (rq.use_probe[col[k]]) mine->push_back(all[k]);
    // shard r of G takes items r, r + G, ...: the grid covers ceil((n - r) / G) of them
    const size_t n_mine = mine->size();
    plan->n_probe_launch = n_mine > rq.shard_rank ? (uint32_t)((n_mine - rq.shard_rank + rq.shard_count - 1) / rq.shard_count) : 0u;
    for (size_t k = rq.shard_rank; k < n_mine; k += rq.shard_count) plan->probe_lookups_launch += item_lookups((*mine)[k]);
}

void plan_probe_launch(const ProbeWork& work, const ProbeLaunchRequest& rq, ProbeLaunchPlan* plan) {
    *plan = ProbeLaunchPlan();
    for (uint8_t u : rq.use_probe) plan->n_probe_cols_launch += u;
    if (rq.bundle == 1) plan_launch_of(work.items, work.item_col, rq, &plan->mine, plan);
    else plan_launch_of(work.fat_items, work.fat_col, rq, &plan->fat, plan);
}

void plan_sparse_segments(const std::vector<RowRange>& cols, uint32_t seg_len, uint32_t shard_rank, uint32_t shard_count,
                          std::vector<Seg>* out, uint64_t* seg_row_sum) {
    std::vector<Seg>& mine = *out;
    mine.clear();
    // upper triangle of every block column; shard = every shard_count-th segment
    std::vector<Seg> full, diag;
    for (const RowRange& col : cols) {
        const uint64_t lo = col.r0, hi = col.r1;
        for (uint64_t a0 = lo; a0 < hi; a0 += kABlockRows) {
            const uint32_t a_end = (uint32_t)std::min<uint64_t>(a0 + kABlockRows, hi);
            if (a_end - a0 > 1) diag.push_back({(uint32_t)a0, a_end, (uint32_t)a0, a_end});
            for (uint64_t j = a0 + kABlockRows; j < hi; j += seg_len)
                full.push_back({(uint32_t)a0, a_end, (uint32_t)j, (uint32_t)std::min<uint64_t>(j + seg_len, hi)});
        }
    }
    for (size_t i = shard_rank; i < full.size(); i += shard_count) mine.push_back(full[i]);
    for (size_t i = shard_rank; i < diag.size(); i += shard_count) mine.push_back(diag[i]);
    *seg_row_sum = 0;
    for (const Seg& g : mine) *seg_row_sum += g.j_hi - g.j_lo;
}

// ---- the block stage's list space ----
StageListPlace stage_place_list(uint64_t lbase, uint32_t lfill, uint32_t n) {
    const uint64_t bytes = (uint64_t)n * 2u, at = lbase + lfill;
    // the buffer goes to its chunk with ONE copy: with this list behind its bytes it must end inside the chunk it starts
    // in. (A buffer that ends exactly ON the chunk's end leaves too: at % kStageListChunk is 0 there, and a list appended
    // to it would be copied past the end of the chunk it does not belong to.)
    const bool over_chunk = lbase % kStageListChunk + lfill + bytes > kStageListChunk;
    StageListPlace p;
    p.send = (over_chunk || lfill + bytes > kStageListBuf) ? 1u : 0u;
    p.lbase = p.send ? at : lbase;
    if (over_chunk) p.lbase = (at + kStageListChunk - 1u) / kStageListChunk * kStageListChunk;
    p.token = p.send ? p.lbase : at;
    return p;
}

void stage_note_list(std::vector<uint64_t>* written, uint64_t token, uint32_t n) {
    const uint64_t chunk = token / kStageListChunk;
    if (written->size() <= chunk) written->resize(chunk + 1u, 0);
    (*written)[chunk] = token % kStageListChunk + (uint64_t)n * 2u;
}

bool stage_list_readable(const std::vector<uint64_t>& written, uint64_t token, uint64_t n) {
    if (token & 1u) return false;
    const uint64_t chunk = token / kStageListChunk, off = token % kStageListChunk;
    if (chunk >= written.size()) return false;                  // beyond the stage
    if (n > kStageListChunk) return false;                      // (2 n below cannot wrap)
    return off + n * 2u <= written[chunk];                      // not in the gap, not across the chunk's end
}

uint64_t dosage_topk_plane_words(uint64_t n_b, bool complete) {
    const uint64_t ld = (n_b + 3u) / 4u * 4u;
    if (!complete) return ld;
    const uint64_t rows128 = (n_b + kThTile - 1) / kThTile * kThTile;
    return ld + 2 * ld + (2 * rows128 + ld);   // P, G_p M_b and H_p M_b, M_p x [G_b ; H_b ; M_b]
}

uint64_t dosage_topk_panel_rows(uint64_t panel_rows, uint64_t n_rows, uint64_t plane_words_per_row) {
    if (panel_rows == 0) {
        const uint64_t row_bytes = std::max<uint64_t>(plane_words_per_row, 1u) * sizeof(uint32_t);
        panel_rows = std::max<uint64_t>(256u, kTopkPanelBytes / row_bytes / 256u * 256u);
    }
    return std::min<uint64_t>(panel_rows, (n_rows + 255u) / 256u * 256u);
}

}  // namespace storm

// a K2h list as the 8-word records of storm_hip_matrix_plan / storm_hip_lag_plan (out == NULL: the count alone)
static int export_part_items(const char* who, const storm::Tile128Plan& plan, uint32_t* out, uint64_t capacity_items,
                             uint64_t* n_items) {
    using namespace storm;
    *n_items = plan.items.size();
    if (out) {
        if (capacity_items < plan.items.size()) {
            set_error("%s: capacity %llu < %zu items", who, (unsigned long long)capacity_items, plan.items.size());
            return STORM_HIP_EINVAL;
        }
        for (size_t k = 0; k < plan.items.size(); ++k) {
            const PartItem& it = plan.items[k];
            uint32_t* o = out + 8 * k;
            o[0] = it.I, o[1] = it.J, o[2] = it.stage0 / 4u, o[3] = it.n_stages / 4u, o[4] = it.tile;
            o[5] = (uint32_t)(it.part & (uint16_t)~kThNarrow), o[6] = it.n_parts, o[7] = (it.part & kThNarrow) ? 1u : 0u;
        }
    }
    return STORM_HIP_OK;
}

// Host-only view of the default path's work decomposition (no device is touched): what a shard
// of a multi-GPU run multiplies, so that the partition of the pair space can be checked — and
// rehearsed with CPU partials — without a GPU (tests/test_dist_cpu.py).
extern "C" int storm_hip_matrix_plan(uint64_t n_rows_a, uint64_t n_rows_b, uint32_t n_words, uint64_t band_row0,
                                     uint64_t band_rows, uint32_t n_cus, int slots_per_cu, int min_chunks, int diag_cost_pct,
                                     uint32_t* out, uint64_t capacity_items, uint64_t* n_items) {
    using namespace storm;
    if (!n_items || n_rows_a == 0 || n_words == 0 || n_cus == 0 || slots_per_cu < 0 || slots_per_cu > 2 || min_chunks < 1 ||
        diag_cost_pct < 10 || diag_cost_pct > 100) {
        set_error("matrix_plan: bad arguments");
        return STORM_HIP_EINVAL;
    }
    try {
        const uint32_t total_stages = (n_words + 7u) / 8u * 4u;
        Tile128Plan plan;
        if (n_rows_b == 0) {   // triangle (a band of it)
            const uint64_t end = std::min(n_rows_a, band_row0 + (band_rows ? band_rows : n_rows_a));
            if (band_row0 < end)
                plan_tile128({(uint32_t)(band_row0 / kThTile), (uint32_t)((end + kThTile - 1) / kThTile), 0u,
                              (uint32_t)((n_rows_a + kThTile - 1) / kThTile), 1u, total_stages, n_cus, slots_per_cu, min_chunks,
                              diag_cost_pct, 1u, 0u, kThWeightBits}, &plan);
        } else {   // rectangle: B's tiles count on behind A's rows padded to 256
            const uint64_t rows_a = (n_rows_a + kTile - 1) / kTile * kTile;
            plan_tile128({0u, (uint32_t)((n_rows_a + kThTile - 1) / kThTile), (uint32_t)(rows_a / kThTile),
                          (uint32_t)((rows_a + n_rows_b + kThTile - 1) / kThTile), 0u, total_stages, n_cus, slots_per_cu,
                          min_chunks, diag_cost_pct, 1u, 0u, kThWeightBits}, &plan);
        }
        return export_part_items("matrix_plan", plan, out, capacity_items, n_items);
    } catch (const std::exception& e) {
        set_error("matrix_plan: %s", e.what());
        return STORM_HIP_ENOMEM;
    }
}

// The K2h list of the dosage form (launch_pairw_dosage_matrix): the triangle of one matrix of rows of 2-bit values, planned
// with a chunk's weight of 9 x 256. Arguments and records as storm_hip_matrix_plan; the rectangle's list is
// storm_hip_dosage_square_plan's.
extern "C" int storm_hip_dosage_plan(uint64_t n_rows_a, uint64_t n_rows_b, uint32_t n_words, uint64_t band_row0,
                                     uint64_t band_rows, uint32_t n_cus, int slots_per_cu, int min_chunks, int diag_cost_pct,
                                     uint32_t* out, uint64_t capacity_items, uint64_t* n_items) {
    using namespace storm;
    if (!n_items || n_rows_a == 0 || n_rows_b != 0 || n_words == 0 || n_cus == 0 || slots_per_cu < 0 || slots_per_cu > 2 ||
        min_chunks < 1 || diag_cost_pct < 10 || diag_cost_pct > 100 || (n_rows_a + kThTile - 1) / kThTile > 65535u) {
        set_error("dosage_plan: bad arguments (the dosage form is the triangle of one matrix: n_rows_b must be 0)");
        return STORM_HIP_EINVAL;
    }
    try {
        Tile128Plan plan;
        const uint64_t end = std::min(n_rows_a, band_row0 + std::min(band_rows ? band_rows : n_rows_a, n_rows_a));
        if (band_row0 < end)
            plan_tile128({(uint32_t)(band_row0 / kThTile), (uint32_t)((end + kThTile - 1) / kThTile), 0u,
                          (uint32_t)((n_rows_a + kThTile - 1) / kThTile), 1u, (n_words + 7u) / 8u * 4u, n_cus, slots_per_cu,
                          min_chunks, diag_cost_pct, 1u, 0u, kThWeightDosage}, &plan);
        return export_part_items("dosage_plan", plan, out, capacity_items, n_items);
    } catch (const std::exception& e) {
        set_error("dosage_plan: %s", e.what());
        return STORM_HIP_ENOMEM;
    }
}

// The K2h list of the dosage form's rectangle (launch_square_dosage_matrix): every 128 x 128 tile of n_rows_a x n_rows_b,
// B's tiles counting on behind A's rows padded to 256 as in storm_hip_matrix_plan's rectangle; a chunk weighs 9 x 256.
extern "C" int storm_hip_dosage_square_plan(uint64_t n_rows_a, uint64_t n_rows_b, uint32_t n_words, uint32_t n_cus,
                                            int slots_per_cu, int min_chunks, int diag_cost_pct, uint32_t* out,
                                            uint64_t capacity_items, uint64_t* n_items) {
    using namespace storm;
    const uint64_t rows_a = (n_rows_a + kTile - 1) / kTile * kTile;
    if (!n_items || n_rows_a == 0 || n_rows_b == 0 || n_words == 0 || n_cus == 0 || slots_per_cu < 0 || slots_per_cu > 2 ||
        min_chunks < 1 || diag_cost_pct < 10 || diag_cost_pct > 100 || n_rows_a > (1ull << 32) || n_rows_b > (1ull << 32) ||
        (rows_a + n_rows_b + kThTile - 1) / kThTile > 65535u) {
        set_error("dosage_square_plan: bad arguments");
        return STORM_HIP_EINVAL;
    }
    try {
        Tile128Plan plan;
        plan_tile128({0u, (uint32_t)((n_rows_a + kThTile - 1) / kThTile), (uint32_t)(rows_a / kThTile),
                      (uint32_t)((rows_a + n_rows_b + kThTile - 1) / kThTile), 0u, (n_words + 7u) / 8u * 4u, n_cus, slots_per_cu,
                      min_chunks, diag_cost_pct, 1u, 0u, kThWeightDosage}, &plan);
        return export_part_items("dosage_square_plan", plan, out, capacity_items, n_items);
    } catch (const std::exception& e) {
        set_error("dosage_square_plan: %s", e.what());
        return STORM_HIP_ENOMEM;
    }
}

// The K2h list of the lag layout (launch_pairw_lag_matrix): the triangle's tiles that hold a pair within max_lag rows.
extern "C" int storm_hip_lag_plan(uint64_t n_rows, uint32_t n_words, uint64_t max_lag, uint64_t band_row0, uint64_t band_rows,
                                  uint32_t n_cus, int slots_per_cu, int min_chunks, int diag_cost_pct, uint32_t* out,
                                  uint64_t capacity_items, uint64_t* n_items) {
    using namespace storm;
    if (!n_items || n_rows == 0 || n_words == 0 || max_lag == 0 || n_cus == 0 || slots_per_cu < 0 || slots_per_cu > 2 ||
        min_chunks < 1 || diag_cost_pct < 10 || diag_cost_pct > 100 || (n_rows + kThTile - 1) / kThTile > 65535u) {
        set_error("lag_plan: bad arguments");
        return STORM_HIP_EINVAL;
    }
    try {
        Tile128Plan plan;
        const uint64_t end = std::min(n_rows, band_row0 + std::min(band_rows ? band_rows : n_rows, n_rows));
        const uint32_t lag = (uint32_t)std::min<uint64_t>(max_lag, n_rows - 1);
        if (band_row0 < end && lag)
            plan_tile128({(uint32_t)(band_row0 / kThTile), (uint32_t)((end + kThTile - 1) / kThTile), 0u,
                          (uint32_t)((n_rows + kThTile - 1) / kThTile), 1u, (n_words + 7u) / 8u * 4u, n_cus, slots_per_cu,
                          min_chunks, diag_cost_pct, 1u, lag, kThWeightBits}, &plan);
        return export_part_items("lag_plan", plan, out, capacity_items, n_items);
    } catch (const std::exception& e) {
        set_error("lag_plan: %s", e.what());
        return STORM_HIP_ENOMEM;
    }
}

// The K2h list of the dosage form in the lag layout (launch_pairw_lag_dosage_matrix): storm_hip_lag_plan's tiles, planned
// with a chunk's weight of 9 x 256 like storm_hip_dosage_plan's.
extern "C" int storm_hip_lag_dosage_plan(uint64_t n_rows, uint32_t n_words, uint64_t max_lag, uint64_t band_row0,
                                         uint64_t band_rows, uint32_t n_cus, int slots_per_cu, int min_chunks, int diag_cost_pct,
                                         uint32_t* out, uint64_t capacity_items, uint64_t* n_items) {
    using namespace storm;
    if (!n_items || n_rows == 0 || n_words == 0 || max_lag == 0 || n_cus == 0 || slots_per_cu < 0 || slots_per_cu > 2 ||
        min_chunks < 1 || diag_cost_pct < 10 || diag_cost_pct > 100 || (n_rows + kThTile - 1) / kThTile > 65535u) {
        set_error("lag_dosage_plan: bad arguments");
        return STORM_HIP_EINVAL;
    }
    try {
        Tile128Plan plan;
        const uint64_t end = std::min(n_rows, band_row0 + std::min(band_rows ? band_rows : n_rows, n_rows));
        const uint32_t lag = (uint32_t)std::min<uint64_t>(max_lag, n_rows - 1);
        if (band_row0 < end && lag)
            plan_tile128({(uint32_t)(band_row0 / kThTile), (uint32_t)((end + kThTile - 1) / kThTile), 0u,
                          (uint32_t)((n_rows + kThTile - 1) / kThTile), 1u, (n_words + 7u) / 8u * 4u, n_cus, slots_per_cu,
                          min_chunks, diag_cost_pct, 1u, lag, kThWeightDosage}, &plan);
        return export_part_items("lag_dosage_plan", plan, out, capacity_items, n_items);
    } catch (const std::exception& e) {
        set_error("lag_dosage_plan: %s", e.what());
        return STORM_HIP_ENOMEM;
    }
}

extern "C" int storm_hip_strip_plan3(uint64_t n_rows, uint32_t n_words, uint32_t shard_rank,
                                     uint32_t shard_count, int form, int pair_space, int max_run, int tail_run,
                                     int tail_slices, int lpt_rounds, uint32_t n_cus, uint32_t* out,
                                     uint64_t capacity_items, uint64_t* n_items, int* run_chosen) {
    using namespace storm;
    if (!n_items || shard_count == 0 || shard_rank >= shard_count || n_words == 0 || form < 0 || form > 2 ||
        max_run < 0 || max_run > 4096 || tail_run < 0 || tail_run > 4096 || tail_slices < 0 || tail_slices > 255 ||
        lpt_rounds < 0 || lpt_rounds > 63 || n_cus == 0) {
        set_error("strip_plan: bad arguments");
        return STORM_HIP_EINVAL;
    }
    try {
        // slices that hold data: form 0 (FP4 shadow, launch_pairw_mfma_ranges): 256 consecutive bits each;
        // form 1 (K2b, launch_pairw_bits_ranges): slice ks = class pair ks & 1 of the 512-bit chunk ks / 2;
        // form 2 (K2b with 128 A rows per wave, strip16_rows_kernel): 128 consecutive bits each, A tiles of 512 rows
        const StripForm& f = *strip_form_of_plan(form);
        std::vector<RowRange> ranges;
        if (n_rows > 1) ranges.push_back({0, n_rows});
        std::vector<StripItem> items;
        uint32_t qb[8], qc[8];
        StripOptions o;
        o.max_run = max_run;
        // tail_run 0: neither tail option is set (a fresh context) — form 2 chooses both for a whole pass, elsewhere the defaults
        o.tail_auto = tail_run == 0;
        o.rows_form = f.rows_form();
        o.tail_run = tail_run == 0 ? StripOptions().tail_run : tail_run;
        o.tail_slices = tail_run == 0 ? StripOptions().tail_slices : tail_slices;
        o.lpt_rounds = lpt_rounds;
        o.shard_pairs = pair_space != 0;
        o.n_cus = (int)n_cus;
        o.xcd_group = f.xcd_group;
        // exactly what ensure_strip_items launches for these options (one function plans both)
        StripChoice used;
        plan_strips(strip_request(o, ranges, f.kslices(n_words), shard_rank, shard_count, f.a_tile), ranges, items, qb, qc, &used);
        // (tail_run 0: the tail in use rides above the run length, which is at most 4096)
        if (run_chosen) *run_chosen = tail_run == 0 ? used.max_run | used.tail_run << 16 | used.tail_slices << 24 : used.max_run;
        *n_items = items.size();
        if (out)
            for (uint64_t i = 0; i < std::min<uint64_t>(capacity_items, items.size()); ++i) {
                out[i * 5 + 0] = items[i].a_row0;
                out[i * 5 + 1] = items[i].diag;
                out[i * 5 + 2] = items[i].j0;
                out[i * 5 + 3] = items[i].j1;
                out[i * 5 + 4] = items[i].ks;
            }
    } catch (const std::exception& e) {
        set_error("strip_plan: %s", e.what());
        return STORM_HIP_ENOMEM;
    }
    return STORM_HIP_OK;
}

// The context's default options on a 256-CU device (what a fresh context launches on an MI355X).
extern "C" int storm_hip_strip_plan2(uint64_t n_rows, uint32_t n_words, uint32_t shard_rank,
                                     uint32_t shard_count, int form, int pair_space, uint32_t* out,
                                     uint64_t capacity_items, uint64_t* n_items) {
    const storm::StripOptions d;
    return storm_hip_strip_plan3(n_rows, n_words, shard_rank, shard_count, form, pair_space, d.max_run, 0 /* not set */,
                                 d.tail_slices, d.lpt_rounds, (uint32_t)d.n_cus, out, capacity_items, n_items, nullptr);
}

extern "C" int storm_hip_strip_plan(uint64_t n_rows, uint32_t n_words, uint32_t shard_rank,
                                    uint32_t shard_count, uint32_t* out, uint64_t capacity_items,
                                    uint64_t* n_items) {
    return storm_hip_strip_plan2(n_rows, n_words, shard_rank, shard_count, 0, 0, out, capacity_items, n_items);
}

extern "C" int storm_hip_stream_plan(uint64_t n_rows, uint32_t n_words, uint32_t shard_rank, uint32_t shard_count,
                                     uint32_t n_cus, uint32_t* out, uint64_t capacity_segments,
                                     uint64_t* n_segments, uint32_t* n_workgroups) {
    using namespace storm;
    if (!n_segments || shard_count == 0 || shard_rank >= shard_count || n_words == 0 || n_cus == 0) {
        set_error("stream_plan: bad arguments");
        return STORM_HIP_EINVAL;
    }
    try {
        std::vector<RowRange> ranges;
        if (n_rows > 1) ranges.push_back({0, n_rows});
        BitstreamPlan plan;
        const uint64_t stride_words = ((uint64_t)n_words + kChunkWords - 1) / kChunkWords * kChunkWords;
        build_bitstream(bitstream_request(BitstreamShaping{}, ranges, (n_words + 7u) / 8u, shard_rank, shard_count, n_cus,
                                          stride_words * 8),
                        ranges, plan);
        *n_segments = plan.segs.size();
        if (n_workgroups) *n_workgroups = plan.groups;
        if (out) {
            uint32_t wg = 0;
            for (uint64_t i = 0; i < std::min<uint64_t>(capacity_segments, plan.segs.size()); ++i) {
                while (wg + 1 < plan.first.size() && plan.first[wg + 1] <= i) ++wg;
                const BitSeg& sg = plan.segs[i];
                uint32_t* o = out + i * 8;
                o[0] = wg;
                o[1] = sg.a_blk;
                o[2] = sg.ks;
                o[3] = sg.b_first;
                o[4] = sg.n_b;
                o[5] = sg.range_nb;
                o[6] = sg.flags & kBsDiag;
                o[7] = 4u + sg.n_b;
            }
        }
    } catch (const std::exception& e) {
        set_error("stream_plan: %s", e.what());
        return STORM_HIP_ENOMEM;
    }
    return STORM_HIP_OK;
}
