/* dosage_prune_driver.c — TEST ONLY. The host entry points of the dosage container's prune / clump calls
 * (stormbitmaps_amd/csrc/storm_dosage_prune.c with the planners storm_ldscore_window.c and storm_prune_order.c, on
 * storm_dosage.c and storm_host.c's locked paths) as a stand-alone program for AddressSanitizer / UBSan, on device_stub.c,
 * dosage_complete_stub.c and dosage_band_stub.c: outputs of exactly n elements (a write behind them
 * is a heap overflow), owner NULL and given, priorities NULL, random, tied and infinite, windows that need exactly max_lag
 * rows and one row more than max_lag, every refusal with nothing written. Never linked into the product. */
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

typedef int (*prune_call)(STORM_dosage_t*, float, uint64_t, const double*, double, const float*, uint8_t*, uint32_t*, uint64_t);
static const prune_call calls[4] = {STORM_dosage_lag_prune, STORM_dosage_lag_prune_device, STORM_dosage_lag_prune_complete,
                                    STORM_dosage_lag_prune_complete_device};
static const char* const names[4] = {"STORM_dosage_lag_prune:", "STORM_dosage_lag_prune_device:", "STORM_dosage_lag_prune_complete:",
                                     "STORM_dosage_lag_prune_complete_device:"};

/* is the pair an edge: from the values themselves, in integers up to the one division */
static int pair_edge(const uint8_t* v, uint64_t S, uint64_t i, uint64_t j, int missing, float min_r2) {
    uint64_t N = 0, P = 0, sx = 0, sy = 0, qx = 0, qy = 0;
    for (uint64_t s = 0; s < S; ++s) {
        const unsigned x = v[i * S + s], y = v[j * S + s];
        if (missing && (x == 3u || y == 3u)) continue;
        N += 1, P += x * y, sx += x, sy += y, qx += x * x, qy += y * y;
    }
    const uint64_t dx = N * qx - sx * sx, dy = N * qy - sy * sy;
    if (dx == 0 || dy == 0) return 0;
    const double num = (double)(N * P) - (double)(sx * sy);
    return (float)(num * num / ((double)dx * (double)dy)) > min_r2;
}

/* pos NULL: rows within L of each other; else within max_dist (the call was not refused: no window exceeds the lag) */
static int adjacent(const uint8_t* v, uint64_t S, uint64_t i, uint64_t j, uint64_t L, const double* pos, double max_dist, int missing,
                    float min_r2) {
    if (i == j) return 0;
    if (pos ? fabs(pos[j] - pos[i]) > max_dist : (j > i ? j - i : i - j) > L) return 0;
    return pair_edge(v, S, i < j ? i : j, i < j ? j : i, missing, min_r2);
}

/* the greedy once more, the slow way: the next row is the best unvisited one (priority, then index) */
static void check_outputs(const uint8_t* v, uint64_t S, uint64_t n, uint64_t L, const double* pos, double max_dist, int missing,
                          float min_r2, const float* priority, const uint8_t* keep, const uint32_t* owner) {
    uint8_t* visited = (uint8_t*)calloc(n ? n : 1, 1);
    uint8_t* want = (uint8_t*)calloc(n ? n : 1, 1);
    uint32_t* own = (uint32_t*)malloc((n ? n : 1) * sizeof(uint32_t));
    CHECK(visited && want && own);
    for (uint64_t k = 0; k < n; ++k) {
        uint64_t best = n;
        for (uint64_t i = 0; i < n; ++i)
            if (!visited[i] && (best == n || (priority && priority[i] > priority[best]))) best = i;
        visited[best] = 1;
        want[best] = 1;   /* ... unless a row kept before it is adjacent */
        for (uint64_t j = 0; j < n; ++j)
            if (want[j] && j != best && adjacent(v, S, best, j, L, pos, max_dist, missing, min_r2)) want[best] = 0;
    }
    /* owners: walk the order again, the first kept neighbour claims */
    memset(visited, 0, n ? n : 1);
    for (uint64_t i = 0; i < n; ++i) own[i] = want[i] ? (uint32_t)i : 0xFFFFFFFFu;
    for (uint64_t k = 0; k < n; ++k) {
        uint64_t best = n;
        for (uint64_t i = 0; i < n; ++i)
            if (!visited[i] && (best == n || (priority && priority[i] > priority[best]))) best = i;
        visited[best] = 1;
        if (!want[best]) continue;
        for (uint64_t j = 0; j < n; ++j)
            if (!want[j] && own[j] == 0xFFFFFFFFu && adjacent(v, S, best, j, L, pos, max_dist, missing, min_r2)) own[j] = (uint32_t)best;
    }
    for (uint64_t i = 0; i < n; ++i) {
        CHECK(keep[i] == want[i]);
        CHECK(own[i] != 0xFFFFFFFFu);   /* a removed row has a kept neighbour */
        if (owner) CHECK(owner[i] == own[i]);
    }
    free(visited), free(want), free(own);
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
    /* outputs of exactly n elements */
    uint8_t* keep = (uint8_t*)malloc(n ? n : 1);
    uint32_t* owner = (uint32_t*)malloc((n ? n : 1) * sizeof(uint32_t));
    float* prio = (float*)malloc((n ? n : 1) * sizeof(float));
    double* pos = (double*)malloc((n ? n : 1) * sizeof(double));
    CHECK(keep && owner && prio && pos);
    /* positions with a tie and a gap; need = the lag the windows need under max_dist 3 */
    for (uint64_t i = 0; i < n; ++i) pos[i] = (double)(i - (i % 5 == 1 ? 1 : 0)) + (i >= n / 2 ? 10.0 : 0.0);
    const double max_dist = 3.0;
    uint64_t need = 777;
    CHECK(STORM_ldscore_window_lag(pos, n, max_dist, &need) == 0);

#define FILL()                                                         \
    do {                                                               \
        for (uint64_t k_ = 0; k_ < n; ++k_) keep[k_] = 0x77u, owner[k_] = 0xDEADBEEFu; \
    } while (0)
#define UNTOUCHED()                                                                          \
    do {                                                                                     \
        for (uint64_t k_ = 0; k_ < n; ++k_) CHECK(keep[k_] == 0x77u && owner[k_] == 0xDEADBEEFu); \
    } while (0)

    const float thresholds[3] = {0.05f, 0.3f, 1.0f};
    for (int k = 0; k < 4; ++k)
        for (int t = 0; t < 3; ++t)
            for (int pk = 0; pk < 4; ++pk)
                for (int with_owner = 0; with_owner < 2; ++with_owner) {
                    const int missing = k >= 2;
                    const float min_r2 = thresholds[t];
                    uint32_t* const o = with_owner ? owner : NULL;
                    /* priorities: NULL, random, two values (ties), infinities */
                    for (uint64_t i = 0; i < n; ++i)
                        prio[i] = pk == 1 ? (float)(next_bits() % 1000u) : pk == 2 ? (float)(next_bits() & 1u)
                                  : (i % 3 == 0 ? INFINITY : i % 3 == 1 ? -INFINITY : 0.5f);
                    const float* const p = pk ? prio : NULL;
                    /* a count window: pos NULL, max_dist ignored (NaN) */
                    FILL();
                    CHECK(calls[k](h, min_r2, 4, NULL, NAN, p, keep, o, n) == 0);
                    check_outputs(v, S, n, 4, NULL, 0, missing, min_r2, p, keep, o);
                    if (!with_owner)
                        for (uint64_t i = 0; i < n; ++i) CHECK(owner[i] == 0xDEADBEEFu);
                    if (n == 1) CHECK(keep[0] == 1 && (!o || o[0] == 0));
                    if (min_r2 == 1.0f)
                        for (uint64_t i = 0; i < n; ++i) CHECK(keep[i] == 1);   /* nothing exceeds 1: every row is kept */
                    if (n) CHECK(keep[0] == 1);                               /* the all-missing row has no edge */
                    /* positions: max_lag 0 (what the windows need), exactly what they need, far more */
                    const uint64_t lags[3] = {0, need, need + 1000};
                    for (int l = 0; l < 3; ++l) {
                        if (l == 1 && need == 0) continue;
                        FILL();
                        CHECK(calls[k](h, min_r2, lags[l], pos, max_dist, p, keep, o, n) == 0);
                        check_outputs(v, S, n, 0, pos, max_dist, missing, min_r2, p, keep, o);
                    }
                    /* ... and one row too few: refused, both numbers named, nothing written */
                    if (need >= 2) {
                        char both[64];
                        FILL();
                        CHECK(calls[k](h, min_r2, need - 1, pos, max_dist, p, keep, o, n) == -3);
                        snprintf(both, sizeof(both), "%llu rows, max_lag is %llu", (unsigned long long)need, (unsigned long long)(need - 1));
                        CHECK(strstr(STORM_hip_error(), both) && strstr(STORM_hip_error(), names[k]));
                        UNTOUCHED();
                    }
                }

    /* refusals at this geometry, in their order: nothing is written */
    FILL();
    for (int k = 0; k < 4; ++k) {
        CHECK(calls[k](NULL, 0.2f, 4, NULL, 0, NULL, keep, owner, n) == -1);
        CHECK(calls[k](h, 0.2f, 4, NULL, 0, NULL, NULL, owner, n) == -2);
        if (n) CHECK(calls[k](h, 0.2f, 4, NULL, 0, NULL, keep, owner, n - 1) == -4);
        if (n) CHECK(calls[k](h, NAN, 4, pos, -1.0, NULL, keep, owner, n - 1) == -4);   /* the size before the rest */
        CHECK(calls[k](h, 0.2f, 0, NULL, 0, NULL, keep, owner, n) == -3 && strstr(STORM_hip_error(), "max_lag"));
        CHECK(calls[k](h, 0.2f, 0, NULL, 0, NULL, keep, owner, 0) == -3 && strstr(STORM_hip_error(), "max_lag"));
        CHECK(calls[k](h, NAN, 4, pos, -1.0, NULL, keep, owner, n) == -3 && strstr(STORM_hip_error(), "min_r2"));
        CHECK(calls[k](h, 0.2f, 4, pos, -1.0, NULL, keep, owner, n) == -3 && strstr(STORM_hip_error(), "max_dist"));
        CHECK(calls[k](h, 0.2f, 0, pos, NAN, NULL, keep, owner, n) == -3 && strstr(STORM_hip_error(), "max_dist"));
        if (n >= 3) {
            const double was = pos[n - 2];
            pos[n - 2] = INFINITY;
            CHECK(calls[k](h, 0.2f, 0, pos, 3.0, NULL, keep, owner, n) == -3);
            CHECK(strstr(STORM_hip_error(), "is not finite") && strstr(STORM_hip_error(), "pos["));
            pos[n - 2] = pos[n - 3] - 1.0;
            CHECK(calls[k](h, 0.2f, 0, pos, 3.0, NULL, keep, owner, n) == -3);
            CHECK(strstr(STORM_hip_error(), "must not decrease"));
            pos[n - 2] = was;
        }
        if (n) {   /* the first NaN priority is named */
            char where[64];
            for (uint64_t i = 0; i < n; ++i) prio[i] = 1.0f;
            prio[n - 1] = NAN;
            if (n >= 2) prio[n / 2] = NAN;
            CHECK(calls[k](h, 0.2f, 4, NULL, 0, prio, keep, owner, n) == -3);
            snprintf(where, sizeof(where), "priority[%llu] is NaN", (unsigned long long)(n >= 2 ? n / 2 : 0));
            CHECK(strstr(STORM_hip_error(), where));
        }
    }
    /* several device slots in view: -5 from every call, which names itself, ahead of the other checks; one slot again after */
    {
        const int three[3] = {0, 0, 0}, one[1] = {0};
        CHECK(STORM_hip_set_devices(3, three) == 0);
        for (int k = 0; k < 4; ++k) {
            CHECK(calls[k](h, 0.2f, 4, pos, max_dist, NULL, keep, owner, n) == -5 && strstr(STORM_hip_error(), names[k]));
            CHECK(calls[k](h, NAN, 0, NULL, 0, NULL, keep, NULL, 0) == -5 && strstr(STORM_hip_error(), "ONE device"));
        }
        CHECK(STORM_hip_set_devices(1, one) == 0);
    }
    UNTOUCHED();
    STORM_dosage_free(h);
    free(v), free(keep), free(owner), free(prio), free(pos);
}

int main(void) {
    const uint64_t samples[] = {1, 2, 33, 65};
    const uint64_t rows[] = {0, 1, 2, 3, 12, 41};
    for (size_t s = 0; s < sizeof(samples) / sizeof(samples[0]); ++s)
        for (size_t r = 0; r < sizeof(rows) / sizeof(rows[0]); ++r) one_shape(samples[s], rows[r]);
    STORM_hip_shutdown();
    printf("dosage prune sanitize: ok\n");
    return 0;
}
