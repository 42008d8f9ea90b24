// choose_pass and the StripForm table (storm_hip_plan.*, nothing else of the library), asked on stdin, one query a line:
//   s <d|p> <n_rows> <n_rows_pad> <n_words> <stride_words> <rows_dst> <pool_rows_ready> <widest>
//         remembers a shape: d for the dense callers, p for the sparse pool (no answer)
//   q <caller> <variant> <k2_strip_operands> <k2_strip_rows> <k2_ring> <k2_shape> <k2_persistent> <k2_debug> <tools> <shard_count>
//         caller 0 dense, 1 dense-upload, 2 sparse pool: one line per remembered shape of the caller's kind, in order:
//         <kernel> <form> <variant_used> <operands_used> <strip_mode> <in_panels>   (the enums as numbers, form -1: none)
//   f <form> <w> ...
//         the record of StripKernel <form>: a_tile waves threads slice_words xcd_group wave_sum_max operands_report rows_report
//         plan_form, then kslices(w) for every w
//   p <form>
//         the StripKernel of storm_hip_strip_plan3's form, -1: none
// tests/test_pass_form.py builds this with the host compiler — once as it is, once under AddressSanitizer + UBSan — and
// compares with tests/_pass_forms.py.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "storm_hip.h"
#include "storm_hip_plan.h"

using namespace storm;

namespace storm {
void set_error(const char*, ...) {}
}  // namespace storm

int main() {
    static const StripForm* const kForms[4] = {&kStripFp4, &kStripBits, &kStripBitsWide, &kStripRows};
    std::vector<PassShape> shapes[2];
    char line[1 << 12];
    while (fgets(line, sizeof line, stdin)) {
        char* tok = strtok(line, " \n");
        if (!tok) continue;
        const char what = tok[0];
        std::vector<long long> v;
        char kind = 0;
        if (what == 's' && (tok = strtok(nullptr, " \n"))) kind = tok[0];
        while ((tok = strtok(nullptr, " \n"))) v.push_back(strtoll(tok, nullptr, 10));
        if (what == 's' && v.size() == 7 && (kind == 'd' || kind == 'p')) {
            PassShape s;
            s.n_rows = (uint64_t)v[0];
            s.n_rows_pad = (uint64_t)v[1];
            s.n_words = (uint32_t)v[2];
            s.stride_words = (uint64_t)v[3];
            s.rows_dst = (uint64_t)v[4];
            s.pool_rows_ready = (uint64_t)v[5];
            s.widest = (uint64_t)v[6];
            shapes[kind == 'p'].push_back(s);
        } else if (what == 'q' && v.size() == 10 && v[0] >= 0 && v[0] <= 2) {
            const PassOptions o = {(int32_t)v[1], (int32_t)v[2], (int32_t)v[3], (int32_t)v[4], (int32_t)v[5], (int32_t)v[6], (int32_t)v[7], v[8] != 0};
            for (PassShape s : shapes[v[0] == 2]) {
                s.shard_count = (uint32_t)v[9];
                const PassChoice c = choose_pass((PassCaller)v[0], o, s);
                printf("%d %d %d %d %d %d\n", (int)c.kernel, c.form ? (int)c.form->kernel : -1, c.variant_used, c.operands_used,
                       c.strip_mode, (int)c.in_panels);
            }
        } else if (what == 'f' && !v.empty() && v[0] >= 0 && v[0] < 4) {
            const StripForm& f = *kForms[v[0]];
            if ((long long)f.kernel != v[0]) return 3;
            printf("%u %u %u %u %d %llu %d %d %d", f.a_tile, f.waves, f.threads(), f.slice_words(), f.xcd_group,
                   (unsigned long long)f.wave_sum_max, f.operands_report, f.rows_report, f.plan_form);
            for (size_t i = 1; i < v.size(); ++i) printf(" %u", f.kslices((uint32_t)v[i]));
            printf("\n");
        } else if (what == 'p' && v.size() == 1) {
            const StripForm* f = strip_form_of_plan((int)v[0]);
            printf("%d\n", f ? (int)f->kernel : -1);
        } else
            return 2;
    }
    return 0;
}
