// The scheduling model of strip16_rows_kernel's work lists (storm_hip_plan.h: strip_rows_makespan, strip_rows_item_cost;
// nothing else of the library), asked on stdin, one query a line:
//   s <n_cus> <slots_per_cu> <start_latency> <item> ...   the makespan of the list; an item is its run length in stages
//                                                        (no diagonal), or d<run> for a tile's first item (diagonal first)
//   c <n_rows> <a_row0> <diag> <j0> <j1>                  what one item costs in stages, where the rows end at n_rows
// Answers go to stdout with seven decimals (a cost is a multiple of 1 / 128). tests/test_strip_rows_tail_plan.py builds this
// with the host compiler — once as it is, once under AddressSanitizer + UBSan — and compares with schedules worked out by
// hand.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "storm_hip_plan.h"

using namespace storm;

namespace storm {
void set_error(const char*, ...) {}
}  // namespace storm

int main() {
    char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) {
        char* tok = strtok(line, " \n");
        if (!tok) continue;
        if (!strcmp(tok, "c")) {
            uint32_t v[5] = {0, 0, 0, 0, 0};
            for (int i = 0; i < 5 && (tok = strtok(nullptr, " \n")); ++i) v[i] = (uint32_t)strtoul(tok, nullptr, 10);
            printf("%.7f\n", strip_rows_item_cost(StripItem{v[1], v[2], v[3], v[4], 0u}, v[0]));
            continue;
        }
        if (strcmp(tok, "s")) return 2;
        uint32_t n_cus = 0, slots = 0;
        double latency = 0;
        if ((tok = strtok(nullptr, " \n"))) n_cus = (uint32_t)strtoul(tok, nullptr, 10);
        if ((tok = strtok(nullptr, " \n"))) slots = (uint32_t)strtoul(tok, nullptr, 10);
        if ((tok = strtok(nullptr, " \n"))) latency = strtod(tok, nullptr);
        std::vector<StripItem> list;
        while ((tok = strtok(nullptr, " \n"))) {
            const uint32_t diag = tok[0] == 'd';
            const uint32_t run = (uint32_t)strtoul(tok + diag, nullptr, 10);
            list.push_back(StripItem{0u, diag, 8u, 8u + run, 0u});   // tile 0: its own 8 blocks, then the run behind them
        }
        printf("%.7f\n", strip_rows_makespan(list.data(), list.size(), kStripRowsNoTrim, n_cus, slots, latency));
    }
    return 0;
}
