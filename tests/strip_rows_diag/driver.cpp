// The schedule of strip16_rows_kernel's diagonal phase (storm_hip_plan.h: strip_rows_block, strip_rows_role,
// strip_rows_diag_begin / _end, strip_rows_role_mfmas; nothing else of the library) as JSON on stdout: per wave its two
// blocks, the block steps it walks and the role of each half at EVERY block d of the tile, walked or not.
// tests/test_strip_rows_diag_schedule.py builds this with the host compiler — once as it is, once under
// AddressSanitizer + UBSan — and checks that the four waves together multiply every pair of blocks exactly once.
#include <cstdio>

#include "storm_hip_plan.h"

using namespace storm;

namespace storm {
void set_error(const char*, ...) {}
}  // namespace storm

// the functions are constexpr: what the kernel's loop bounds are built from is known when it is compiled
static_assert(strip_rows_role(0, 0, 0) == kStripRowsOwn && strip_rows_role(0, 1, 7) == kStripRowsOwn, "wave 0 keeps blocks 0 and 7");
static_assert(strip_rows_diag_begin(3) == 3 && strip_rows_diag_end(3) == kStripRowsBlocks, "wave 3 walks blocks 3 .. 7");

int main() {
    printf("{\"blocks\": %u, \"waves\": %u, \"skip\": %u, \"own\": %u, \"whole\": %u,\n", kStripRowsBlocks, kStripRowsWaves,
           (unsigned)kStripRowsSkip, (unsigned)kStripRowsOwn, (unsigned)kStripRowsWhole);
    printf(" \"mfmas\": [%u, %u, %u],\n", strip_rows_role_mfmas(kStripRowsSkip), strip_rows_role_mfmas(kStripRowsOwn),
           strip_rows_role_mfmas(kStripRowsWhole));
    printf(" \"wave\": [\n");
    for (uint32_t w = 0; w < kStripRowsWaves; ++w) {
        printf("  {\"block\": [%u, %u], \"begin\": %u, \"end\": %u, \"role\": [", strip_rows_block(w, 0), strip_rows_block(w, 1),
               strip_rows_diag_begin(w), strip_rows_diag_end(w));
        for (uint32_t half = 0; half < 2; ++half) {
            printf("%s[", half ? ", " : "");
            for (uint32_t d = 0; d < kStripRowsBlocks; ++d) printf("%s%u", d ? "," : "", (unsigned)strip_rows_role(w, half, d));
            printf("]");
        }
        printf("]}%s\n", w + 1 < kStripRowsWaves ? "," : "");
    }
    printf(" ]}\n");
    return 0;
}
