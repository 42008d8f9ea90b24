/* dosage_lag_sparse_driver.c — TEST ONLY. The host entry points of the dosage container's sparse LD report
 * (stormbitmaps_amd/csrc/storm_dosage_lag_sparse.c with the planner storm_ldscore_window.c, on storm_dosage.c and
 * storm_host.c's locked paths) as a stand-alone program for AddressSanitizer / UBSan, on device_stub.c, dosage_band_stub.c and
 * dosage_lag_sparse_stub.c: row_start of exactly n + 1 and col / val of exactly `total` elements (a write behind them is a
 * heap overflow), a capacity of total - 1 (-4 from the host forms, the first total - 1 pairs from the _device forms), the
 * count-only call, windows that need exactly max_lag rows and one row more than max_lag, every refusal with nothing written.
 * Never linked into the product. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "storm.h"
#include "storm_hip.h"

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static unsigned next_bits(void) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_rng >> 40);
}

static const char* const names[4] = {"STORM_dosage_lag_corr_sparse:", "STORM_dosage_lag_corr_sparse_device:",
                                     "STORM_dosage_lag_corr_sparse_complete:", "STORM_dosage_lag_corr_sparse_complete_device:"};

/* call k: 0 host, 1 _device, 2 _complete, 3 _complete_device (the _device forms take no n_pairs) */
static int sparse(int k, STORM_dosage_t* h, float min_r2, uint64_t max_lag, const double* pos, double max_dist, uint64_t* row_start,
                  uint64_t out_rows, uint32_t* col, float* val, uint64_t capacity, uint64_t* n_pairs) {
    switch (k) {
        case 0: return STORM_dosage_lag_corr_sparse(h, min_r2, max_lag, pos, max_dist, row_start, out_rows, col, val, capacity, n_pairs);
        case 1: return STORM_dosage_lag_corr_sparse_device(h, min_r2, max_lag, pos, max_dist, row_start, out_rows, col, val, capacity);
        case 2:
            return STORM_dosage_lag_corr_sparse_complete(h, min_r2, max_lag, pos, max_dist, row_start, out_rows, col, val, capacity,
                                                         n_pairs);
        default:
            return STORM_dosage_lag_corr_sparse_complete_device(h, min_r2, max_lag, pos, max_dist, row_start, out_rows, col, val,
                                                                capacity);
    }
}

/* the pair's r^2 from the values themselves, in integers up to the one division; 0: not a number */
static int pair_r2(const uint8_t* v, uint64_t S, uint64_t i, uint64_t j, int missing, float* rho) {
    uint64_t N = 0, P = 0, sx = 0, sy = 0, qx = 0, qy = 0;
    for (uint64_t s = 0; s < S; ++s) {
        const unsigned x = v[i * S + s], y = v[j * S + s];
        if (missing && (x == 3u || y == 3u)) continue;
        N += 1, P += x * y, sx += x, sy += y, qx += x * x, qy += y * y;
    }
    const uint64_t dx = N * qx - sx * sx, dy = N * qy - sy * sy;
    if (dx == 0 || dy == 0) return 0;
    const double num = (double)(N * P) - (double)(sx * sy);
    *rho = (float)(num * num / ((double)dx * (double)dy));
    return 1;
}

/* the list once more, pair by pair: the wanted offsets into want_rows (n + 1), the entries compared where given */
static uint64_t check_list(const uint8_t* v, uint64_t S, uint64_t n, uint64_t L, const double* pos, double max_dist, int missing,
                           float min_r2, const uint64_t* row_start, const uint32_t* col, const float* val, uint64_t written) {
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) {
        CHECK(row_start[i] == total);
        for (uint64_t j = i + 1; j < n; ++j) {
            float rho = 0;
            if (pos ? pos[j] - pos[i] > max_dist : j - i > L) continue;
            if (!pair_r2(v, S, i, j, missing, &rho) || !(rho > min_r2)) continue;
            if (col && total < written) CHECK(col[total] == j && val[total] == rho);
            ++total;
        }
    }
    CHECK(row_start[n] == total);
    return total;
}

static void one_shape(uint64_t S, uint64_t n) {
    STORM_dosage_t* h = STORM_dosage_new(S);
    CHECK(h);
    uint8_t* v = (uint8_t*)malloc((size_t)(n ? n : 1) * S);
    CHECK(v);
    for (uint64_t r = 0; r < n; ++r) {
        /* row 0: all missing; a row is mostly its predecessor, so that pairs exceed the thresholds */
        for (uint64_t s = 0; s < S; ++s)
            v[r * S + s] = (uint8_t)(r == 0 ? 3u : (r > 1 && next_bits() % 4u) ? v[(r - 1) * S + s] : next_bits() & 3u);
        CHECK(STORM_dosage_add(h, v + r * S, S) == 0);
    }
    uint64_t* rows = (uint64_t*)malloc((n + 1) * sizeof(uint64_t));   /* exactly n + 1 */
    double* pos = (double*)malloc((n ? n : 1) * sizeof(double));
    CHECK(rows && pos);
    for (uint64_t i = 0; i < n; ++i) pos[i] = (double)(i - (i % 5 == 1 ? 1 : 0)) + (i >= n / 2 ? 10.0 : 0.0);
    const double max_dist = 3.0;
    uint64_t need = 777;
    CHECK(STORM_ldscore_window_lag(pos, n, max_dist, &need) == 0);

    const float thresholds[4] = {-1.0f, 0.05f, 0.3f, 1.0f};
    for (int k = 0; k < 4; ++k)
        for (int t = 0; t < 4; ++t)
            for (int w = 0; w < 4; ++w) {   /* w 0: a count window (pos NULL, max_dist ignored: NaN); 1 .. 3: positions */
                const int missing = k >= 2, device = k & 1;
                const float min_r2 = thresholds[t];
                const uint64_t lags[4] = {4, 0, need, need + 1000};
                const double* const p = w ? pos : NULL;
                const double dist = w ? max_dist : NAN;
                if (w == 2 && need == 0) continue;
                /* the count-only call */
                uint64_t total = 12345;
                memset(rows, 0x77, (n + 1) * sizeof(uint64_t));
                CHECK(sparse(k, h, min_r2, lags[w], p, dist, rows, n + 1, NULL, NULL, 0, &total) == 0);
                const uint64_t want = check_list(v, S, n, 4, p, max_dist, missing, min_r2, rows, NULL, NULL, 0);
                CHECK(device ? total == 12345 : total == want);
                if (min_r2 == 1.0f) CHECK(want == 0);   /* nothing exceeds 1 */
                /* outputs of exactly `want` elements */
                uint32_t* col = (uint32_t*)malloc(want ? want * sizeof(uint32_t) : 1);
                float* val = (float*)malloc(want ? want * sizeof(float) : 1);
                CHECK(col && val);
                memset(rows, 0x77, (n + 1) * sizeof(uint64_t));
                total = 12345;
                CHECK(sparse(k, h, min_r2, lags[w], p, dist, rows, n + 1, col, val, want, &total) == 0);
                CHECK(check_list(v, S, n, 4, p, max_dist, missing, min_r2, rows, col, val, want) == want);
                CHECK(device ? total == 12345 : total == want);
                free(col), free(val);
                /* one element fewer: -4 from a host form with the offsets and the total valid; a _device form writes the first
                 * want - 1 pairs and nothing behind them */
                if (want) {
                    char both[96];
                    col = (uint32_t*)malloc(want > 1 ? (want - 1) * sizeof(uint32_t) : 1);
                    val = (float*)malloc(want > 1 ? (want - 1) * sizeof(float) : 1);
                    CHECK(col && val);
                    memset(rows, 0x77, (n + 1) * sizeof(uint64_t));
                    total = 12345;
                    const int rc = sparse(k, h, min_r2, lags[w], p, dist, rows, n + 1, col, val, want - 1, &total);
                    if (device) {
                        CHECK(rc == 0);
                        CHECK(check_list(v, S, n, 4, p, max_dist, missing, min_r2, rows, col, val, want - 1) == want);
                    } else {
                        CHECK(rc == -4 && total == want);
                        CHECK(check_list(v, S, n, 4, p, max_dist, missing, min_r2, rows, NULL, NULL, 0) == want);
                        snprintf(both, sizeof(both), "%llu pairs are listed, capacity is %llu", (unsigned long long)want,
                                 (unsigned long long)(want - 1));
                        CHECK(strstr(STORM_hip_error(), both) && strstr(STORM_hip_error(), names[k]));
                    }
                    free(col), free(val);
                }
                /* one row too few for the windows: refused, both numbers named, nothing written */
                if (w && need >= 2) {
                    char both[64];
                    memset(rows, 0x77, (n + 1) * sizeof(uint64_t));
                    total = 12345;
                    CHECK(sparse(k, h, min_r2, need - 1, pos, max_dist, rows, n + 1, NULL, NULL, 0, &total) == -3);
                    snprintf(both, sizeof(both), "%llu rows, max_lag is %llu", (unsigned long long)need, (unsigned long long)(need - 1));
                    CHECK(strstr(STORM_hip_error(), both) && strstr(STORM_hip_error(), names[k]));
                    for (uint64_t i = 0; i <= n; ++i) CHECK(rows[i] == 0x7777777777777777ull);
                    CHECK(total == 12345);
                }
            }

    /* refusals at this geometry, in their order: nothing is written */
    uint32_t col[4] = {9, 9, 9, 9};
    float val[4] = {9, 9, 9, 9};
    uint64_t total = 12345;
    memset(rows, 0x77, (n + 1) * sizeof(uint64_t));
    for (int k = 0; k < 4; ++k) {
        const int device = k & 1;
        CHECK(sparse(k, NULL, 0.2f, 4, NULL, 0, rows, n + 1, col, val, 4, &total) == -1);
        CHECK(sparse(k, h, 0.2f, 4, NULL, 0, NULL, n + 1, col, val, 4, &total) == -2);
        if (!device) CHECK(sparse(k, h, 0.2f, 4, NULL, 0, rows, n + 1, col, val, 4, NULL) == -2);
        CHECK(sparse(k, h, 0.2f, 4, NULL, 0, rows, n + 1, NULL, val, 4, &total) == -2);
        CHECK(sparse(k, h, 0.2f, 4, NULL, 0, rows, n + 1, col, NULL, 4, &total) == -2);
        CHECK(sparse(k, h, 0.2f, 4, NULL, 0, rows, n + 1, NULL, NULL, 4, &total) == -2);
        if (n) CHECK(sparse(k, h, 0.2f, 4, NULL, 0, rows, n, col, val, 4, &total) == -4);
        if (n) CHECK(sparse(k, h, NAN, 4, pos, -1.0, rows, n, col, val, 4, &total) == -4);   /* the size before the rest */
        CHECK(sparse(k, h, 0.2f, 0, NULL, 0, rows, n + 1, col, val, 4, &total) == -3 && strstr(STORM_hip_error(), "max_lag"));
        CHECK(sparse(k, h, 0.2f, 0, NULL, 0, rows, 0, col, val, 4, &total) == -3 && strstr(STORM_hip_error(), "max_lag"));
        CHECK(sparse(k, h, NAN, 4, pos, -1.0, rows, n + 1, col, val, 4, &total) == -3 && strstr(STORM_hip_error(), "min_r2"));
        CHECK(sparse(k, h, 0.2f, 4, pos, -1.0, rows, n + 1, col, val, 4, &total) == -3 && strstr(STORM_hip_error(), "max_dist"));
        CHECK(sparse(k, h, 0.2f, 0, pos, NAN, rows, n + 1, col, val, 4, &total) == -3 && strstr(STORM_hip_error(), "max_dist"));
        if (n >= 3) {
            const double was = pos[n - 2];
            pos[n - 2] = INFINITY;
            CHECK(sparse(k, h, 0.2f, 0, pos, 3.0, rows, n + 1, col, val, 4, &total) == -3);
            CHECK(strstr(STORM_hip_error(), "is not finite") && strstr(STORM_hip_error(), "pos["));
            pos[n - 2] = pos[n - 3] - 1.0;
            CHECK(sparse(k, h, 0.2f, 0, pos, 3.0, rows, n + 1, col, val, 4, &total) == -3);
            CHECK(strstr(STORM_hip_error(), "must not decrease"));
            pos[n - 2] = was;
        }
    }
    /* several device slots in view: -5 from every call, which names itself, ahead of the other checks; one slot again after */
    {
        const int three[3] = {0, 0, 0}, one[1] = {0};
        CHECK(STORM_hip_set_devices(3, three) == 0);
        for (int k = 0; k < 4; ++k) {
            CHECK(sparse(k, h, 0.2f, 4, pos, max_dist, rows, n + 1, col, val, 4, &total) == -5 && strstr(STORM_hip_error(), names[k]));
            CHECK(sparse(k, h, NAN, 0, NULL, 0, rows, 0, NULL, NULL, 0, &total) == -5 && strstr(STORM_hip_error(), "ONE device"));
        }
        CHECK(STORM_hip_set_devices(1, one) == 0);
    }
    for (uint64_t i = 0; i <= n; ++i) CHECK(rows[i] == 0x7777777777777777ull);
    for (int i = 0; i < 4; ++i) CHECK(col[i] == 9 && val[i] == 9);
    CHECK(total == 12345);
    STORM_dosage_free(h);
    free(v), free(rows), free(pos);
}

int main(void) {
    const uint64_t samples[] = {1, 2, 33, 65};
    const uint64_t rows[] = {0, 1, 2, 3, 12, 41};
    for (size_t s = 0; s < sizeof(samples) / sizeof(samples[0]); ++s)
        for (size_t r = 0; r < sizeof(rows) / sizeof(rows[0]); ++r) one_shape(samples[s], rows[r]);
    STORM_hip_shutdown();
    printf("dosage lag sparse sanitize: ok\n");
    return 0;
}
