/* storm_prune_order.c — the order planner of LD pruning and clumping (storm_prune_order.h). Host only. */
#include "storm_prune_order.h"

#include <stdlib.h>
#include <string.h>

int storm_prune_order_plan(const float* priority, uint64_t n, uint32_t* order, uint32_t* rank, uint64_t* bad) {
    if (n > 0xFFFFFFFFull) return STORM_PRUNE_ORDER_TOO_MANY;
    /* every refusal before the first write */
    if (priority)
        for (uint64_t i = 0; i < n; ++i)
            if (priority[i] != priority[i]) {
                if (bad) *bad = i;
                return STORM_PRUNE_ORDER_NAN;
            }
    uint32_t* tmp = NULL;
    if (priority && n > 1) {
        tmp = (uint32_t*)malloc((size_t)n * sizeof(uint32_t));
        if (!tmp) return STORM_PRUNE_ORDER_NOMEM;
    }
    for (uint64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
    if (tmp) {
        /* runs of `width` rows, merged pairwise; the left run wins a tie: rows of equal priority stay in row order */
        uint32_t *src = order, *dst = tmp;
        for (uint64_t width = 1; width < n; width *= 2) {
            for (uint64_t lo = 0; lo < n; lo += 2 * width) {
                const uint64_t mid = lo + width < n ? lo + width : n, hi = lo + 2 * width < n ? lo + 2 * width : n;
                uint64_t a = lo, b = mid, k = lo;
                while (a < mid && b < hi) dst[k++] = priority[src[b]] > priority[src[a]] ? src[b++] : src[a++];
                while (a < mid) dst[k++] = src[a++];
                while (b < hi) dst[k++] = src[b++];
            }
            uint32_t* const t = src;
            src = dst, dst = t;
        }
        if (src != order) memcpy(order, src, (size_t)n * sizeof(uint32_t));
        free(tmp);
    }
    if (rank)
        for (uint64_t k = 0; k < n; ++k) rank[order[k]] = (uint32_t)k;
    return STORM_PRUNE_ORDER_OK;
}
