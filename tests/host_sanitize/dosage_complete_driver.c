/* dosage_complete_driver.c — TEST ONLY. The host entry points of the dosage container's rectangle and of its calls for rows
 * with missing genotypes (stormbitmaps_amd/csrc/storm_dosage_pairs.c on storm_dosage.c and storm_host.c's locked paths) as
 * a stand-alone program for AddressSanitizer / UBSan, on device_stub.c, dosage_complete_stub.c and dosage_pairs_stub.c: what reaches the
 * "device" from two containers, outputs with a pitch, every refusal, growth between calls. Never linked into the product. */
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

static uint8_t* fill(STORM_dosage_t* h, uint64_t S, uint64_t n_rows) {
    uint8_t* vals = (uint8_t*)malloc((size_t)(n_rows ? n_rows : 1) * S);
    CHECK(vals);
    for (uint64_t r = 0; r < n_rows; ++r) {
        for (uint64_t s = 0; s < S; ++s) vals[r * S + s] = (uint8_t)(r == 0 ? 3u : next_value()); /* row 0: all missing */
        CHECK(STORM_dosage_add(h, vals + r * S, S) == 0);
    }
    return vals;
}

static void one_shape(uint64_t S, uint64_t na, uint64_t nb) {
    STORM_dosage_t* a = STORM_dosage_new(S);
    STORM_dosage_t* b = STORM_dosage_new(S);
    CHECK(a && b);
    uint8_t* va = fill(a, S, na);
    uint8_t* vb = fill(b, S, nb);

    /* the rectangle: an output with a pitch, the whole n_a x n_b window and nothing outside it */
    const uint64_t ld = nb + 3;
    uint32_t* out = (uint32_t*)malloc((size_t)(na + 1) * ld * sizeof(uint32_t));
    CHECK(out);
    for (int device = 0; device < 2; ++device) {
        for (uint64_t k = 0; k < (na + 1) * ld; ++k) out[k] = 0xDEADBEEFu;
        CHECK((device ? STORM_dosage_square_dot_device(a, b, out, na + 1, ld) : STORM_dosage_square_dot(a, b, out, na + 1, ld)) == 0);
        for (uint64_t i = 0; i <= na; ++i)
            for (uint64_t j = 0; j < ld; ++j) {
                if (i >= na || j >= nb || na == 0 || nb == 0) {
                    CHECK(out[i * ld + j] == 0xDEADBEEFu);
                    continue;
                }
                uint32_t p = 0;
                for (uint64_t s = 0; s < S; ++s) p += (uint32_t)va[i * S + s] * vb[j * S + s];
                CHECK(out[i * ld + j] == p);
            }
    }
    if (na) CHECK(STORM_dosage_square_dot(a, b, out, na - 1, ld) == -4);
    if (nb) CHECK(STORM_dosage_square_dot(a, b, out, na, nb - 1) == -4);

    /* the rectangle's statistics go through the same body: the shared samples, r with row 0 (all missing) sharing nothing */
    float* fout = (float*)malloc((size_t)(na + 1) * ld * sizeof(float));
    CHECK(fout);
    for (int device = 0; device < 2; ++device) {
        for (uint64_t k = 0; k < (na + 1) * ld; ++k) out[k] = 0xDEADBEEFu, fout[k] = -7.5f;
        CHECK((device ? STORM_dosage_square_nobs_device(a, b, out, na + 1, ld) : STORM_dosage_square_nobs(a, b, out, na + 1, ld)) == 0);
        CHECK((device ? STORM_dosage_square_corr_complete_device(a, b, STORM_DOSAGE_R, fout, na + 1, ld)
                      : STORM_dosage_square_corr_complete(a, b, STORM_DOSAGE_R, fout, na + 1, ld)) == 0);
        for (uint64_t i = 0; i <= na; ++i)
            for (uint64_t j = 0; j < ld; ++j) {
                if (i >= na || j >= nb || na == 0 || nb == 0) {
                    CHECK(out[i * ld + j] == 0xDEADBEEFu && fout[i * ld + j] == -7.5f);
                    continue;
                }
                uint32_t c = 0;
                for (uint64_t s = 0; s < S; ++s) c += va[i * S + s] != 3 && vb[j * S + s] != 3;
                CHECK(out[i * ld + j] == c);
                CHECK((i != 0 && j != 0) || (c == 0 && isnan(fout[i * ld + j])));
            }
        CHECK((device ? STORM_dosage_square_corr_device(a, b, STORM_DOSAGE_R2, fout, na + 1, ld)
                      : STORM_dosage_square_corr(a, b, STORM_DOSAGE_R2, fout, na + 1, ld)) == 0);
    }
    CHECK(STORM_dosage_square_corr(a, b, 2, fout, na + 1, ld) == -3 && STORM_dosage_square_corr_complete_device(a, b, -1, fout, na + 1, ld) == -3);
    if (na) CHECK(STORM_dosage_square_nobs(a, b, out, na - 1, ld) == -4 && STORM_dosage_square_corr(a, b, 0, fout, na - 1, ld) == -4);
    free(out), free(fout);

    /* missing genotypes on `a`: the triangle with a pitch, host zeros at i >= j, nothing outside the n x n window */
    const uint64_t n = na, ldn = n + 3;
    uint32_t* miss = (uint32_t*)malloc((n + 1) * sizeof(uint32_t));
    uint32_t* nobs = (uint32_t*)malloc((size_t)(n + 1) * ldn * sizeof(uint32_t));
    float* corr = (float*)malloc((size_t)(n + 1) * ldn * sizeof(float));
    CHECK(miss && nobs && corr);
    miss[n] = 0xDEADBEEFu;
    CHECK(STORM_dosage_row_missing(a, miss) == 0 && miss[n] == 0xDEADBEEFu);
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t c = 0;
        for (uint64_t s = 0; s < S; ++s) c += va[i * S + s] == STORM_DOSAGE_MISSING;
        CHECK(miss[i] == c && (i != 0 || c == S));
    }
    for (uint64_t k = 0; k < (n + 1) * ldn; ++k) nobs[k] = 0xDEADBEEFu, corr[k] = -7.5f;
    CHECK(STORM_dosage_pairw_nobs(a, nobs, n + 1, ldn) == 0);
    CHECK(STORM_dosage_pairw_corr_complete(a, STORM_DOSAGE_R, corr, n + 1, ldn) == 0);
    for (uint64_t i = 0; i <= n; ++i)
        for (uint64_t j = 0; j < ldn; ++j) {
            const int inside = n >= 2 && i < n && j < n;
            if (!inside) CHECK(nobs[i * ldn + j] == 0xDEADBEEFu && corr[i * ldn + j] == -7.5f);
            else if (j <= i) CHECK(nobs[i * ldn + j] == 0 && corr[i * ldn + j] == 0.0f);
            else {
                uint32_t c = 0;
                for (uint64_t s = 0; s < S; ++s) c += va[i * S + s] != 3 && va[j * S + s] != 3;
                CHECK(nobs[i * ldn + j] == c);
                CHECK(i != 0 || (c == 0 && isnan(corr[i * ldn + j])));   /* row 0 shares nothing with anybody */
            }
        }
    CHECK(STORM_dosage_pairw_nobs_device(a, nobs, n, ldn) == 0);
    CHECK(STORM_dosage_pairw_corr_complete_device(a, STORM_DOSAGE_R2, corr, n, ldn) == 0);
    if (n) {
        CHECK(STORM_dosage_pairw_nobs(a, nobs, n, n - 1) == -4 && STORM_dosage_pairw_nobs_device(a, nobs, n - 1, n) == -4);
        CHECK(STORM_dosage_pairw_corr_complete(a, 0, corr, n - 1, n) == -4);
    }
    CHECK(STORM_dosage_pairw_corr_complete(a, 2, corr, n + 1, ldn) == -3 && STORM_dosage_pairw_corr_complete(a, -1, corr, n + 1, ldn) == -3);

    /* rows added after a compute call travel on the next one, to both operands of the rectangle */
    uint8_t* row = (uint8_t*)malloc(S);
    CHECK(row);
    for (uint64_t s = 0; s < S; ++s) row[s] = 2;
    CHECK(STORM_dosage_add(a, row, S) == 0 && STORM_dosage_add(b, row, S) == 0);
    uint32_t* out2 = (uint32_t*)malloc((size_t)(na + 1) * ((na > nb ? na : nb) + 1) * sizeof(uint32_t));
    CHECK(out2);
    CHECK(STORM_dosage_square_dot(a, b, out2, na + 1, nb + 1) == 0);
    CHECK(out2[na * (nb + 1) + nb] == 4 * S);
    CHECK(STORM_dosage_square_dot(a, a, out2, na + 1, na + 1) == 0 && out2[na * (na + 1) + na] == 4 * S);   /* against itself */

    /* containers of different sample counts: refused before anything is written */
    STORM_dosage_t* c = STORM_dosage_new(S + 1);
    CHECK(c);
    out2[0] = 0xDEADBEEFu;
    CHECK(STORM_dosage_square_dot(a, c, out2, na + 1, na + 1) == -3 && STORM_dosage_square_dot_device(c, a, out2, na + 1, na + 1) == -3);
    CHECK(out2[0] == 0xDEADBEEFu && STORM_hip_error()[0] != '\0');

    STORM_dosage_free(a);
    STORM_dosage_free(b);
    STORM_dosage_free(c);
    free(va), free(vb), free(miss), free(nobs), free(corr), free(row), free(out2);
}

int main(void) {
    uint32_t word = 0;
    float fword = 0;
    STORM_dosage_t* h = STORM_dosage_new(5);
    CHECK(h);
    CHECK(STORM_dosage_square_dot(NULL, h, &word, 1, 1) == -1 && STORM_dosage_square_dot(h, NULL, &word, 1, 1) == -1);
    CHECK(STORM_dosage_square_dot(h, h, NULL, 1, 1) == -2 && STORM_dosage_square_dot_device(h, h, NULL, 1, 1) == -2);
    CHECK(STORM_dosage_row_missing(NULL, &word) == -1 && STORM_dosage_row_missing(h, NULL) == -2);
    CHECK(STORM_dosage_pairw_nobs(NULL, &word, 1, 1) == -1 && STORM_dosage_pairw_nobs_device(h, NULL, 1, 1) == -2);
    CHECK(STORM_dosage_pairw_corr_complete(NULL, 0, &fword, 1, 1) == -1 && STORM_dosage_pairw_corr_complete_device(h, 0, NULL, 1, 1) == -2);
    STORM_dosage_free(h);
    const uint64_t samples[] = {1, 31, 32, 33, 65, 1000};
    const uint64_t rows[][2] = {{0, 3}, {1, 1}, {2, 3}, {3, 70}, {70, 2}, {130, 66}};   /* 70, 130: beyond the first allocation */
    for (size_t s = 0; s < sizeof(samples) / sizeof(samples[0]); ++s)
        for (size_t r = 0; r < sizeof(rows) / sizeof(rows[0]); ++r) one_shape(samples[s], rows[r][0], rows[r][1]);
    STORM_hip_shutdown();
    printf("dosage complete sanitize: ok\n");
    return 0;
}
