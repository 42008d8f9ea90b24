// The sparse arena's host-only planners (storm_hip_plan.cpp, nothing else of the library) on one case read from a file;
// every output array as JSON on stdout. tests/test_arena_plan.py builds this with the host compiler — once as it is,
// once under AddressSanitizer + UBSan — and pins the output (tests/golden/arena_plan_digests.json).
//
// Case file (text, whitespace separated):
//     n_rows n_blocks
//     row_block_offset[0 .. n_rows]
//     per block:  id kind n ptr  v[0 .. n)      kind 0 = list of n positions (the values follow), else no values;
//                                                ptr 0 = the block has data, 1 = at an odd address, 2 = NULL
//     n_overrides, then per override:  probe_block octant value     (replaces a computed run end)
// With the argument --single-column instead of a case file: K1's segment tables of a dense matrix (one column from row 0).
#include <cstdarg>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>

#include "storm_hip.h"
#include "storm_hip_plan.h"

using namespace storm;

static std::string g_error;
namespace storm {
void set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_error = buf;
}
}  // namespace storm

template <class T>
static void put(const char* name, const std::vector<T>& v, const char* tail = ",") {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%lld", i ? "," : "", (long long)v[i]);
    printf("]%s\n", tail);
}
static void put_rows(const char* name, const std::vector<std::vector<uint32_t>>& rows, const char* tail = ",") {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < rows.size(); ++i) {
        printf("%s[", i ? "," : "");
        for (size_t k = 0; k < rows[i].size(); ++k) printf("%s%u", k ? "," : "", rows[i][k]);
        printf("]");
    }
    printf("]%s\n", tail);
}
static std::vector<uint32_t> fields(const ProbeItem& it) {
    return {it.a_begin, it.a_end, it.n_begin, it.n_end, it.b_begin, it.b_end, it.a0};
}
static std::vector<uint32_t> fields(const ProbeFatItem& it) {
    return {it.at[0], it.at[1], it.at[2], it.at[3], it.at[4], it.b_begin, it.b_end, it.first};
}
// every item of the arena as its device record's fields + its column
template <class Item>
static std::vector<std::vector<uint32_t>> with_col(const std::vector<Item>& items, const std::vector<uint32_t>& col) {
    std::vector<std::vector<uint32_t>> rows;
    for (size_t k = 0; k < items.size(); ++k) {
        rows.push_back(fields(items[k]));
        rows.back().push_back(col.at(k));
    }
    return rows;
}

// K1's segment table of a dense matrix: plan_sparse_segments over the single column from row 0 (storm_hip.hip: ensure_segments)
static int single_column_segments() {
    printf("{\n");
    bool first_case = true;
    for (uint64_t n : {1ull, 2ull, 128ull, 129ull, 600ull})
        for (uint32_t seg_len : {256u, 100u})
            for (uint32_t world : {1u, 3u})
                for (uint32_t rank = 0; rank < world; ++rank) {
                    std::vector<Seg> mine;
                    uint64_t row_sum = 0;
                    plan_sparse_segments({{0, n}}, seg_len, rank, world, &mine, &row_sum);
                    std::vector<std::vector<uint32_t>> recs;
                    for (const Seg& g : mine) recs.push_back({g.a_row0, g.a_end, g.j_lo, g.j_hi});
                    printf("%s\"n%llu/len%u/w%u/r%u\": {\n", first_case ? "" : ",", (unsigned long long)n, seg_len, world, rank);
                    first_case = false;
                    put_rows("segs", recs);
                    put("row_sum", std::vector<uint64_t>{row_sum}, "");
                    printf("}\n");
                }
    printf("}\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    if (std::string(argv[1]) == "--single-column") return single_column_segments();
    std::ifstream f(argv[1]);
    uint64_t n_rows = 0, n_blocks = 0;
    if (!(f >> n_rows >> n_blocks)) return 2;
    std::vector<uint64_t> row_off(n_rows + 1);
    for (uint64_t& v : row_off) f >> v;
    std::vector<uint32_t> id(n_blocks), len(n_blocks);
    std::vector<uint8_t> kind(n_blocks);
    std::vector<std::vector<uint16_t>> lists(n_blocks);
    std::vector<const void*> ptr(n_blocks, nullptr);
    static const uint64_t bitmap_words[kBlockWords] = {0};   // (the planners never read a block's data)
    for (uint64_t b = 0; b < n_blocks; ++b) {
        uint32_t k = 0, how = 0;
        f >> id[b] >> k >> len[b] >> how;
        kind[b] = (uint8_t)k;
        if (k == 0) {
            lists[b].resize(len[b] <= 65536u ? len[b] : 0u);
            for (uint16_t& v : lists[b]) f >> v;
        }
        const uint8_t* data = k == 0 ? reinterpret_cast<const uint8_t*>(lists[b].data()) : reinterpret_cast<const uint8_t*>(bitmap_words);
        if (k == 0 && lists[b].empty()) data = reinterpret_cast<const uint8_t*>(bitmap_words);   // (some address: never read)
        ptr[b] = how == 2 ? nullptr : how == 1 ? data + 1 : data;
    }
    size_t n_overrides = 0;
    f >> n_overrides;
    std::vector<uint32_t> overrides(3 * n_overrides);
    for (uint32_t& v : overrides) f >> v;
    if (!f) return 2;

    ArenaBlocks in{n_rows, n_blocks, row_off.data(), id.data(), kind.data(), len.data(), ptr.data()};
    ArenaColumns cols;
    ArenaRows rows;
    ArenaLaps laps;
    ProbeWork work;
    ProbeLayout layout;
    std::vector<uint32_t> run_end;
    int rc = plan_arena_columns(in, &cols, &rows, laps);
    if (rc == STORM_HIP_OK) {
        // probe_run_end_kernel on the host: the first index of the list whose value is >= (o + 1) * 8192
        for (uint64_t b : rows.probe_blocks)
            for (uint32_t o = 0; o < kProbeOctants; ++o) {
                const uint32_t lim = (o + 1u) << kProbeOctBits;
                uint32_t lo = 0, hi = len[b];
                while (lo < hi) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if ((uint32_t)lists[b][mid] < lim) lo = mid + 1u;
                    else hi = mid;
                }
                run_end.push_back(lo);
            }
        for (size_t k = 0; k < n_overrides; ++k) run_end.at(overrides[3 * k] * kProbeOctants + overrides[3 * k + 1]) = overrides[3 * k + 2];
        rc = plan_arena_probe(in, cols, rows, run_end, &work, &layout, laps);
    }
    printf("{\"status\": {\"rc\": %d, \"error\": \"%s\"}", rc, rc ? g_error.c_str() : "");
    if (rc != STORM_HIP_OK) {
        printf("}\n");
        return 0;
    }
    printf(",\n\"columns\": {\n");
    std::vector<uint64_t> r0, r1;
    for (const RowRange& c : cols.cols) r0.push_back(c.r0), r1.push_back(c.r1);
    put("cols_r0", r0);
    put("cols_r1", r1);
    put("col_list0", cols.col_list0);
    put("col_probe", cols.col_probe);
    put("col_avg_len", cols.col_avg_len);
    put("census", std::vector<uint64_t>(cols.census, cols.census + 4));
    put("pool_rows", std::vector<uint64_t>{cols.pool_rows_ready, cols.n_pool_rows});
    put("list_row", rows.list_row);
    put("list_blk", rows.list_blk);
    put("list_len", rows.list_len);
    put("dense_row", rows.dense_row);
    put("dense_blk", rows.dense_blk);
    put("probe_blocks", rows.probe_blocks, "");
    printf("},\n\"probe\": {\n");
    std::vector<std::vector<uint32_t>> regions;
    for (const ProbeRegion& r : work.probe_regions) regions.push_back({r.e_begin, r.e_end, r.pool_row0, r.octant});
    put_rows("probe_regions", regions);
    put("run_end", run_end);
    put("run_dst", layout.run_dst);
    put("block_local", layout.block_local);
    put("atoms", layout.atoms);
    put("n_probe_elems", std::vector<uint64_t>{layout.n_probe_elems});
    put_rows("items", with_col(work.items, work.item_col));
    put_rows("fat_items", with_col(work.fat_items, work.fat_col), "");
    printf("},\n\"launch\": {\n");
    bool first_case = true;
    for (int bundle : {1, (int)kFatGroups})
        for (uint32_t world : {1u, 2u, 3u})
            for (uint32_t rank = 0; rank < world; ++rank)
                for (int masked = 0; masked < 2; ++masked) {
                    ProbeLaunchRequest rq{rank, world, bundle, cols.col_probe};
                    if (masked) {   // every other probe column is not in use
                        uint32_t seen = 0;
                        for (uint8_t& u : rq.use_probe)
                            if (u && (seen++ & 1u)) u = 0;
                    }
                    ProbeLaunchPlan plan;
                    plan_probe_launch(work, rq, &plan);
                    std::vector<std::vector<uint32_t>> recs;
                    for (const ProbeItem& it : plan.mine) recs.push_back(fields(it));
                    for (const ProbeFatItem& it : plan.fat) recs.push_back(fields(it));
                    printf("%s\"b%d/w%u/r%u/%s\": {\n", first_case ? "" : ",", bundle, world, rank, masked ? "alt" : "all");
                    first_case = false;
                    put_rows("records", recs);
                    put("counts", std::vector<uint64_t>{plan.n_probe_launch, plan.n_probe_cols_launch, plan.probe_lookups_launch}, "");
                    printf("}\n");
                }
    printf("},\n\"segments\": {\n");
    first_case = true;
    for (uint32_t seg_len : {1u, 256u})   // 256: the context's default of option seg_rows
        for (uint32_t world : {1u, 3u})
            for (uint32_t rank = 0; rank < world; ++rank) {
                std::vector<Seg> mine;
                uint64_t row_sum = 0;
                plan_sparse_segments(cols.cols, seg_len, rank, world, &mine, &row_sum);
                std::vector<std::vector<uint32_t>> recs;
                for (const Seg& g : mine) recs.push_back({g.a_row0, g.a_end, g.j_lo, g.j_hi});
                printf("%s\"len%u/w%u/r%u\": {\n", first_case ? "" : ",", seg_len, world, rank);
                first_case = false;
                put_rows("segs", recs);
                put("row_sum", std::vector<uint64_t>{row_sum}, "");
                printf("}\n");
            }
    printf("}}\n");
    return 0;
}
