/* stub_dosage.h — TEST ONLY. What the stubs of the device library share: the "device" matrix in host memory (device_stub.c
 * fills it), a dosage value of it, and a pair's r^2 computed sample by sample on the CPU. Never linked into the product. */
#pragma once
#include <math.h>
#include <stdint.h>

#include "storm_hip.h"

struct storm_hip_matrix_s { uint64_t n_rows; uint32_t n_words; uint64_t* rows; };

static inline unsigned value_at(const storm_hip_matrix_t* m, uint64_t row, uint64_t s) {
    return (unsigned)(m->rows[row * m->n_words + s / 32] >> (2 * (s % 32))) & 3u;
}

/* the pair's r^2 as the corr call's float and the samples behind it; `missing` reads 3 as "no call" */
static inline float pair_r2(const storm_hip_matrix_t* m, uint64_t i, uint64_t j, int missing, uint64_t n_samples, uint64_t* n_obs) {
    double N = 0, P = 0, sx = 0, sy = 0, qx = 0, qy = 0;
    for (uint64_t s = 0; s < n_samples; ++s) {
        const unsigned x = value_at(m, i, s), y = value_at(m, j, s);
        if (missing && (x == 3u || y == 3u)) continue;
        N += 1, P += x * y, sx += x, sy += y, qx += x * x, qy += y * y;
    }
    *n_obs = (uint64_t)N;
    const double num = N * P - sx * sy, dx = N * qx - sx * sx, dy = N * qy - sy * sy;
    return dx == 0 || dy == 0 ? NAN : (float)(num * num / (dx * dy));
}
