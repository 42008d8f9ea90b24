// The block stage's list-space rules (storm_hip_plan.cpp: stage_place_list, stage_note_list, stage_list_readable; nothing
// else of the library) on one case read from a file; the answers as JSON on stdout. tests/test_stage_plan.py builds this
// with the host compiler — once as it is, once under AddressSanitizer + UBSan — and checks the answers against the
// rules as DESIGN.md §2 and storm_hip.h state them.
//
// Case file (text, whitespace separated):
//     n_lists    n[0 .. n_lists)              the lengths handed to storm_hip_stage_add_list, in order
//     n_queries  per query:  token n          is (token, n) readable once all the lists above are staged?
//
// The lists are placed the way storm_hip_stage_add_list places them: a send where stage_place_list asks for one (what
// stage_send_lists does to lbase and lfill), then the list behind the buffer's bytes.
#include <cstdarg>
#include <cstdio>
#include <fstream>
#include <vector>

#include "storm_hip_plan.h"

using namespace storm;

namespace storm {
void set_error(const char*, ...) {}
}  // namespace storm

static void put(const char* name, const std::vector<uint64_t>& v, const char* tail = ",") {
    printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); ++i) printf("%s%llu", i ? "," : "", (unsigned long long)v[i]);
    printf("]%s\n", tail);
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    size_t n_lists = 0, n_queries = 0;
    if (!(f >> n_lists)) return 2;
    std::vector<uint32_t> len(n_lists);
    for (uint32_t& v : len) f >> v;
    f >> n_queries;
    std::vector<uint64_t> query(2 * n_queries);
    for (uint64_t& v : query) f >> v;
    if (!f) return 2;

    uint64_t lbase = 0;
    uint32_t lfill = 0;
    std::vector<uint64_t> written, tokens, sent_base, sent_bytes, list_buffer;
    for (uint32_t n : len) {
        const StageListPlace at = stage_place_list(lbase, lfill, n);
        if (at.send) {   // (the buffer [lbase, lbase + lfill) leaves for its chunk)
            sent_base.push_back(lbase);
            sent_bytes.push_back(lfill);
        }
        lbase = at.lbase;
        lfill = (uint32_t)(at.token - at.lbase) + 2u * n;
        stage_note_list(&written, at.token, n);
        tokens.push_back(at.token);
        list_buffer.push_back(sent_base.size());   // the buffer the list lies in: the next one to leave
    }
    sent_base.push_back(lbase);   // what a build sends before it reads
    sent_bytes.push_back(lfill);

    std::vector<uint64_t> readable;
    for (size_t q = 0; q < n_queries; ++q) readable.push_back(stage_list_readable(written, query[2 * q], query[2 * q + 1]) ? 1 : 0);
    printf("{\n");
    put("tokens", tokens);
    put("list_buffer", list_buffer);
    put("buffer_base", sent_base);
    put("buffer_bytes", sent_bytes);
    put("written", written);
    put("limits", std::vector<uint64_t>{kStageListBuf, kStageListChunk, kStageMaxList});
    put("readable", readable, "");
    printf("}\n");
    return 0;
}
