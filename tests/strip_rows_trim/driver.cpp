// What strip16_rows_kernel skips behind the matrix's last row (storm_hip_plan.h: strip_rows_real_frags,
// strip_rows_real_blocks, strip_rows_top_trimmed, strip_rows_item_mfmas; nothing else of the library). Reads queries
// from stdin, one per line, and answers each with one line of numbers on stdout:
//   f <n_rows> <blk>                        -> fragments of B block blk that hold a row below n_rows
//   b <n_rows> <a_row0>                     -> blocks of the A tile at a_row0 that hold a row below n_rows
//   m <n_rows> <a_row0> <diag> <j0> <j1>    -> MFMAs of the item: nothing trimmed, the top block alone, the kernel's rule;
//                                              then 1 if the item's top block is multiplied last and in part
// tests/test_strip_rows_trim.py builds this with the host compiler — once as it is, once under AddressSanitizer + UBSan.
#include <cstdio>

#include "storm_hip_plan.h"

using namespace storm;

namespace storm {
void set_error(const char*, ...) {}
}  // namespace storm

// the functions are constexpr: the headline shape's figures are known when this is compiled
static_assert(strip_rows_real_frags(156, 10000) == 1 && strip_rows_real_frags(155, 10000) == 4 && strip_rows_real_frags(157, 10000) == 0,
              "10000 rows: block 156 holds 16 of them");
static_assert(strip_rows_real_blocks(9728, 10000) == 5 && strip_rows_real_blocks(9216, 10000) == 8 && strip_rows_real_blocks(10240, 10000) == 0,
              "10000 rows: the last tile holds 272 of them in 5 blocks");
static_assert(strip_rows_real_frags(0, kStripRowsNoTrim) == 4 && strip_rows_real_blocks(0, kStripRowsNoTrim) == 8, "nothing trimmed");
static_assert(strip_rows_item_mfmas(9728, 1, 0, 0, kStripRowsNoTrim) == 528 && strip_rows_item_mfmas(9728, 1, 0, 0, 10000) == 210,
              "the last tile's diagonal phase at 10000 rows");
static_assert(strip_rows_item_mfmas(0, 0, 150, 157, kStripRowsNoTrim) == 7 * 128 && strip_rows_item_mfmas(0, 0, 150, 157, 10000) == 6 * 128 + 32,
              "a run that ends in block 156 at 10000 rows");

int main() {
    char kind;
    unsigned n_rows, a, diag, j0, j1;
    while (scanf(" %c %u %u", &kind, &n_rows, &a) == 3) {
        if (kind == 'f') {
            printf("%u\n", strip_rows_real_frags(a, n_rows));
        } else if (kind == 'b') {
            printf("%u\n", strip_rows_real_blocks(a, n_rows));
        } else if (kind == 'm' && scanf("%u %u %u", &diag, &j0, &j1) == 3) {
            // the top block alone: the run by the rule, the diagonal phase whole
            const unsigned top_only = strip_rows_item_mfmas(a, 0, j0, j1, n_rows) + (diag ? strip_rows_item_mfmas(a, 1, 0, 0, kStripRowsNoTrim) : 0u);
            printf("%u %u %u %u\n", strip_rows_item_mfmas(a, diag, j0, j1, kStripRowsNoTrim), top_only,
                   strip_rows_item_mfmas(a, diag, j0, j1, n_rows), strip_rows_top_trimmed(j0, j1, n_rows) ? 1u : 0u);
        } else {
            return 2;
        }
    }
    return 0;
}
