// The panel-size rule of the dosage top-k calls (storm_hip_plan.cpp: dosage_topk_plane_words, dosage_topk_panel_rows;
// nothing else of the library) on cases read from a file; the answers as JSON on stdout. tests/test_dosage_topk_plan.py
// builds this with the host compiler and checks the answers against the rule as storm_hip.h states it.
//
// Case file (text, whitespace separated):  n_cases, then per case  panel_rows n_a n_b complete
#include <cstdio>
#include <fstream>

#include "storm_hip_plan.h"

using namespace storm;

namespace storm {
void set_error(const char*, ...) {}
}  // namespace storm

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream f(argv[1]);
    size_t n_cases = 0;
    if (!(f >> n_cases)) return 2;
    printf("{\"panel_bytes\": %llu, \"cases\": [", (unsigned long long)kTopkPanelBytes);
    for (size_t c = 0; c < n_cases; ++c) {
        uint64_t panel_rows = 0, n_a = 0, n_b = 0, complete = 0;
        if (!(f >> panel_rows >> n_a >> n_b >> complete)) return 2;
        const uint64_t words = dosage_topk_plane_words(n_b, complete != 0);
        printf("%s[%llu, %llu]", c ? ", " : "", (unsigned long long)words,
               (unsigned long long)dosage_topk_panel_rows(panel_rows, n_a, words));
    }
    printf("]}\n");
    return 0;
}
