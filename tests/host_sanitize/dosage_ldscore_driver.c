/* dosage_ldscore_driver.c — TEST ONLY. The host entry points of the dosage container's LD scores
 * (stormbitmaps_amd/csrc/storm_dosage_ldscore.c on storm_dosage.c and storm_host.c's locked paths) as a stand-alone program
 * for AddressSanitizer / UBSan, on device_stub.c, dosage_complete_stub.c and dosage_band_stub.c: outputs of exactly n
 * elements (a write behind n is a heap overflow), lags below, at and beyond n - 1, every refusal (several device slots in
 * view among them), rows added between calls. Never linked into the product. */
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
static unsigned next_value(void) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_rng >> 61) & 3u;
}

typedef int (*ld_call)(STORM_dosage_t*, int, uint64_t, float*, uint32_t*, uint64_t);
static const ld_call calls[4] = {STORM_dosage_lag_ldscore, STORM_dosage_lag_ldscore_device, STORM_dosage_lag_ldscore_complete,
                                 STORM_dosage_lag_ldscore_complete_device};

/* the pair's term from the values themselves, in integers up to the one division: 0 when the pair is not summed */
static int pair_term(const uint8_t* v, uint64_t S, uint64_t i, uint64_t j, int missing, int stat, double* t) {
    uint64_t N = 0, P = 0, sx = 0, sy = 0, qx = 0, qy = 0;
    for (uint64_t s = 0; s < S; ++s) {
        const unsigned x = v[i * S + s], y = v[j * S + s];
        if (missing && (x == 3u || y == 3u)) continue;
        N += 1, P += x * y, sx += x, sy += y, qx += x * x, qy += y * y;
    }
    const uint64_t dx = N * qx - sx * sx, dy = N * qy - sy * sy;
    if (dx == 0 || dy == 0) return 0;
    const double num = (double)(N * P) - (double)(sx * sy);
    const double rho = (double)(float)(num * num / ((double)dx * (double)dy));
    if (stat == STORM_LDSCORE_R2_ADJ && N < 3) return 0;
    *t = stat == STORM_LDSCORE_R2_ADJ ? rho - (1.0 - rho) / (double)(N - 2) : rho;
    return 1;
}

static void check_outputs(const uint8_t* v, uint64_t S, uint64_t n, uint64_t max_lag, int missing, int stat, const float* score,
                          const uint32_t* n_pairs) {
    const uint64_t L = max_lag < n - 1 ? max_lag : n - 1;
    for (uint64_t i = 0; i < n; ++i) {
        double sum = 0, t;
        uint32_t m = 0;
        for (uint64_t j = i > L ? i - L : 0; j < n && j <= i + L; ++j)
            if (j != i && pair_term(v, S, j < i ? j : i, j < i ? i : j, missing, stat, &t)) sum += t, ++m;
        CHECK(!n_pairs || n_pairs[i] == m);
        CHECK(fabs((double)score[i] - sum) <= 1e-5 * (m + 1.0));
        if (m == 0) CHECK(score[i] == 0.0f && !signbit(score[i]));
    }
}

static void one_shape(uint64_t S, uint64_t n, uint64_t max_lag) {
    STORM_dosage_t* h = STORM_dosage_new(S);
    CHECK(h);
    uint8_t* v = (uint8_t*)malloc((size_t)(n + 2) * S);
    CHECK(v);
    for (uint64_t r = 0; r < n; ++r) {
        for (uint64_t s = 0; s < S; ++s) v[r * S + s] = (uint8_t)(r == 0 ? 3u : next_value());   /* row 0: all missing */
        CHECK(STORM_dosage_add(h, v + r * S, S) == 0);
    }
    /* outputs of exactly n elements: a write behind n is a heap overflow */
    float* score = (float*)malloc((n ? n : 1) * sizeof(float));
    uint32_t* pairs = (uint32_t*)malloc((n ? n : 1) * sizeof(uint32_t));
    CHECK(score && pairs);
    for (int k = 0; k < 4; ++k)
        for (int stat = 0; stat < 2; ++stat)
            for (int with_pairs = 0; with_pairs < 2; ++with_pairs) {
                const int missing = k >= 2;
                for (uint64_t i = 0; i < n; ++i) score[i] = -77.5f, pairs[i] = 0xDEADBEEFu;
                const int rc = calls[k](h, stat, max_lag, score, with_pairs ? pairs : NULL, n);
                if (!missing && stat == STORM_LDSCORE_R2_ADJ && S < 3) {   /* no n_samples - 2 to divide by */
                    CHECK(rc == -3 && strstr(STORM_hip_error(), "3 samples"));
                    for (uint64_t i = 0; i < n; ++i) CHECK(score[i] == -77.5f && pairs[i] == 0xDEADBEEFu);
                    continue;
                }
                CHECK(rc == 0);
                if (n < 2) {
                    for (uint64_t i = 0; i < n; ++i) CHECK(score[i] == -77.5f && pairs[i] == 0xDEADBEEFu);
                    continue;
                }
                check_outputs(v, S, n, max_lag, missing, stat, score, with_pairs ? pairs : NULL);
                if (!with_pairs)
                    for (uint64_t i = 0; i < n; ++i) CHECK(pairs[i] == 0xDEADBEEFu);
                if (missing && with_pairs) CHECK(pairs[0] == 0 && score[0] == 0.0f);   /* row 0 shares nothing with anybody */
            }
    /* refusals at this geometry: nothing is written */
    for (uint64_t i = 0; i < n; ++i) score[i] = -77.5f, pairs[i] = 0xDEADBEEFu;
    for (int k = 0; k < 4; ++k) {
        if (n) CHECK(calls[k](h, 0, max_lag, score, pairs, n - 1) == -4 && calls[k](h, 7, max_lag, score, NULL, n - 1) == -4);
        CHECK(calls[k](h, 0, 0, score, pairs, n) == -3 && strstr(STORM_hip_error(), "max_lag"));
        CHECK(calls[k](h, 1, 0, score, pairs, 0) == -3 && strstr(STORM_hip_error(), "max_lag"));
        CHECK(calls[k](h, 2, max_lag, score, pairs, n) == -3 && strstr(STORM_hip_error(), "stat"));
        CHECK(calls[k](h, -1, max_lag, score, pairs, n) == -3 && strstr(STORM_hip_error(), "stat"));
        CHECK(calls[k](h, 0, max_lag, NULL, pairs, n) == -2);
    }
    /* several device slots in view: -5 from every call, which names itself, ahead of the other checks; one slot again after */
    {
        static const char* const names[4] = {"STORM_dosage_lag_ldscore:", "STORM_dosage_lag_ldscore_device:",
                                             "STORM_dosage_lag_ldscore_complete:", "STORM_dosage_lag_ldscore_complete_device:"};
        const int three[3] = {0, 0, 0}, one[1] = {0};
        CHECK(STORM_hip_set_devices(3, three) == 0);
        for (int k = 0; k < 4; ++k) {
            CHECK(calls[k](h, 0, max_lag, score, pairs, n) == -5 && strstr(STORM_hip_error(), names[k]));
            CHECK(calls[k](h, 1, max_lag, score, NULL, n) == -5 && strstr(STORM_hip_error(), "ONE device"));
            CHECK(calls[k](h, 9, 0, score, pairs, 0) == -5);
        }
        CHECK(STORM_hip_set_devices(1, one) == 0);
    }
    for (uint64_t i = 0; i < n; ++i) CHECK(score[i] == -77.5f && pairs[i] == 0xDEADBEEFu);
    free(score), free(pairs);

    /* rows added after a compute call travel on the next one: outputs of exactly n + 2 elements */
    for (uint64_t r = n; r < n + 2; ++r) {
        for (uint64_t s = 0; s < S; ++s) v[r * S + s] = (uint8_t)(next_value() % 3u);
        CHECK(STORM_dosage_add(h, v + r * S, S) == 0);
    }
    float* score2 = (float*)malloc((size_t)(n + 2) * sizeof(float));
    uint32_t* pairs2 = (uint32_t*)malloc((size_t)(n + 2) * sizeof(uint32_t));
    CHECK(score2 && pairs2);
    CHECK(STORM_dosage_lag_ldscore(h, STORM_LDSCORE_R2, max_lag, score2, pairs2, n + 1) == -4);
    CHECK(STORM_dosage_lag_ldscore(h, STORM_LDSCORE_R2, max_lag, score2, pairs2, n + 2) == 0);
    check_outputs(v, S, n + 2, max_lag, 0, STORM_LDSCORE_R2, score2, pairs2);
    CHECK(STORM_dosage_lag_ldscore_complete_device(h, STORM_LDSCORE_R2_ADJ, max_lag, score2, pairs2, n + 2) == 0);
    check_outputs(v, S, n + 2, max_lag, 1, STORM_LDSCORE_R2_ADJ, score2, pairs2);
    STORM_dosage_free(h);
    free(v), free(score2), free(pairs2);
}

int main(void) {
    float fword = 0;
    uint32_t word = 0;
    STORM_dosage_t* h = STORM_dosage_new(5);
    CHECK(h);
    for (int k = 0; k < 4; ++k) {
        CHECK(calls[k](NULL, 0, 1, &fword, &word, 1) == -1 && calls[k](h, 0, 1, NULL, &word, 1) == -2);
        CHECK(calls[k](h, 0, 0, &fword, &word, 1) == -3);   /* max_lag 0 on an empty container */
        CHECK(calls[k](h, 1, 4, &fword, NULL, 0) == 0);     /* empty: nothing to do */
    }
    CHECK(fword == 0 && word == 0);
    STORM_dosage_free(h);
    const uint64_t samples[] = {1, 2, 31, 33, 65, 300};
    const uint64_t shapes[][2] = {{0, 3}, {1, 1}, {2, 1}, {2, 5}, {3, 1}, {40, 1}, {40, 38}, {40, 39}, {40, 1000}, {70, 64}};   /* rows, max_lag */
    for (size_t s = 0; s < sizeof(samples) / sizeof(samples[0]); ++s)
        for (size_t r = 0; r < sizeof(shapes) / sizeof(shapes[0]); ++r) one_shape(samples[s], shapes[r][0], shapes[r][1]);
    STORM_hip_shutdown();
    printf("dosage ldscore sanitize: ok\n");
    return 0;
}
