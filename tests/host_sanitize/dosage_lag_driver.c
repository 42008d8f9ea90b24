/* dosage_lag_driver.c — TEST ONLY. The host entry points of the dosage container's lag calls
 * (stormbitmaps_amd/csrc/storm_dosage_lag.c on storm_dosage.c and storm_host.c's locked paths) as a stand-alone program for
 * AddressSanitizer / UBSan, on device_stub.c, dosage_complete_stub.c and dosage_lag_stub.c: outputs of exactly n x L entries
 * and with a pitch, lags below, at and beyond n - 1, every refusal, rows added between calls. Never linked into the product. */
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

typedef int (*u32_call)(STORM_dosage_t*, uint64_t, uint32_t*, uint64_t, uint64_t);
typedef int (*f32_call)(STORM_dosage_t*, int, uint64_t, float*, uint64_t, uint64_t);

static void one_shape(uint64_t S, uint64_t n, uint64_t max_lag) {
    STORM_dosage_t* h = STORM_dosage_new(S);
    CHECK(h);
    uint8_t* v = (uint8_t*)malloc((size_t)(n ? n : 1) * S);
    CHECK(v);
    for (uint64_t r = 0; r < n; ++r) {
        for (uint64_t s = 0; s < S; ++s) v[r * S + s] = (uint8_t)(r == 0 ? 3u : next_value());   /* row 0: all missing */
        CHECK(STORM_dosage_add(h, v + r * S, S) == 0);
    }
    const uint64_t L = n ? (max_lag < n - 1 ? max_lag : n - 1) : 0;
    const u32_call u32[4] = {STORM_dosage_pairw_lag_dot, STORM_dosage_pairw_lag_dot_device, STORM_dosage_pairw_lag_nobs,
                             STORM_dosage_pairw_lag_nobs_device};
    const f32_call f32[4] = {STORM_dosage_pairw_lag_corr, STORM_dosage_pairw_lag_corr_device, STORM_dosage_pairw_lag_corr_complete,
                             STORM_dosage_pairw_lag_corr_complete_device};
    /* two geometries: exactly n x L (an allocation of that size: a write outside the layout is a heap overflow), and a pitch */
    for (int pitch = 0; pitch < 2; ++pitch) {
        const uint64_t rows = n + (pitch ? 1 : 0), ld = L + (pitch ? 3 : 0);
        const size_t count = (size_t)rows * ld;
        uint32_t* out = (uint32_t*)malloc((count ? count : 1) * sizeof(uint32_t));
        CHECK(out);
        for (int k = 0; k < 8; ++k) {
            const int device = k & 1, is_float = k >= 4, missing = (k & 3) >= 2;
            for (size_t t = 0; t < count; ++t) out[t] = 0xDEADBEEFu;
            const int rc = is_float ? f32[k - 4](h, (k >> 1) & 1, max_lag, (float*)out, rows, ld) : u32[k](h, max_lag, out, rows, ld);
            CHECK(rc == 0);
            for (uint64_t i = 0; i < rows; ++i)
                for (uint64_t d = 0; d < ld; ++d) {
                    const uint32_t got = out[i * ld + d];
                    if (n < 2 || i >= n || d >= L) {
                        CHECK(got == 0xDEADBEEFu);
                        continue;
                    }
                    const uint64_t j = i + 1 + d;
                    if (j >= n) {   /* the corner: host forms 0, device forms untouched */
                        CHECK(got == (device ? 0xDEADBEEFu : 0u));
                        continue;
                    }
                    if (is_float) {
                        float f;
                        memcpy(&f, &got, sizeof(f));
                        CHECK(!(missing && i == 0) || isnan(f));   /* row 0 shares nothing with anybody */
                        CHECK(isnan(f) || (f >= -1.0001f && f <= 1.0001f));
                        continue;
                    }
                    uint32_t want = 0;
                    for (uint64_t s = 0; s < S; ++s) {
                        const unsigned x = v[i * S + s], y = v[j * S + s];
                        want += missing ? (x != 3 && y != 3) : x * y;
                    }
                    CHECK(got == want);
                }
        }
        /* refusals at this geometry: nothing is written */
        for (size_t t = 0; t < count; ++t) out[t] = 0xDEADBEEFu;
        for (int k = 0; k < 4; ++k) {
            if (n) CHECK(u32[k](h, max_lag, out, n - 1, ld) == -4 && f32[k](h, 0, max_lag, (float*)out, n - 1, ld) == -4);
            if (L) CHECK(u32[k](h, max_lag, out, rows, L - 1) == -4 && f32[k](h, 1, max_lag, (float*)out, rows, L - 1) == -4);
            CHECK(u32[k](h, 0, out, rows, ld) == -3 && f32[k](h, 0, 0, (float*)out, rows, ld) == -3);
            CHECK(f32[k](h, 2, max_lag, (float*)out, rows, ld) == -3 && f32[k](h, -1, max_lag, (float*)out, rows, ld) == -3);
            CHECK(STORM_hip_error()[0] != '\0');
        }
        for (size_t t = 0; t < count; ++t) CHECK(out[t] == 0xDEADBEEFu);
        free(out);
    }

    /* a row added after a compute call travels on the next one */
    uint8_t* row = (uint8_t*)malloc(S);
    CHECK(row);
    for (uint64_t s = 0; s < S; ++s) row[s] = 2;
    CHECK(STORM_dosage_add(h, row, S) == 0 && STORM_dosage_add(h, row, S) == 0);
    uint32_t* out2 = (uint32_t*)calloc((size_t)(n + 2), sizeof(uint32_t));
    CHECK(out2);
    CHECK(STORM_dosage_pairw_lag_dot(h, 1, out2, n + 2, 1) == 0 && out2[n] == 4 * S && out2[n + 1] == 0);
    STORM_dosage_free(h);
    free(v), free(row), free(out2);
}

int main(void) {
    uint32_t word = 0;
    float fword = 0;
    STORM_dosage_t* h = STORM_dosage_new(5);
    CHECK(h);
    CHECK(STORM_dosage_pairw_lag_dot(NULL, 1, &word, 1, 1) == -1 && STORM_dosage_pairw_lag_dot_device(h, 1, NULL, 1, 1) == -2);
    CHECK(STORM_dosage_pairw_lag_nobs(NULL, 1, &word, 1, 1) == -1 && STORM_dosage_pairw_lag_nobs_device(h, 1, NULL, 1, 1) == -2);
    CHECK(STORM_dosage_pairw_lag_corr(NULL, 0, 1, &fword, 1, 1) == -1 && STORM_dosage_pairw_lag_corr_device(h, 0, 1, NULL, 1, 1) == -2);
    CHECK(STORM_dosage_pairw_lag_corr_complete(NULL, 0, 1, &fword, 1, 1) == -1 &&
          STORM_dosage_pairw_lag_corr_complete_device(h, 0, 1, NULL, 1, 1) == -2);
    STORM_dosage_free(h);
    const uint64_t samples[] = {1, 31, 33, 65, 1000};
    const uint64_t shapes[][2] = {{0, 3}, {1, 1}, {2, 1}, {2, 5}, {3, 1}, {70, 1}, {70, 69}, {70, 1000}, {130, 64}};   /* rows, max_lag */
    for (size_t s = 0; s < sizeof(samples) / sizeof(samples[0]); ++s)
        for (size_t r = 0; r < sizeof(shapes) / sizeof(shapes[0]); ++r) one_shape(samples[s], shapes[r][0], shapes[r][1]);
    STORM_hip_shutdown();
    printf("dosage lag sanitize: ok\n");
    return 0;
}
