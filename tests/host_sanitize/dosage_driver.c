/* dosage_driver.c — TEST ONLY. The host side of the dosage container (stormbitmaps_amd/csrc/storm_dosage.c: packing, growth,
 * refusals, the upload towards the device) as a stand-alone program for AddressSanitizer / UBSan, on device_stub.c. The
 * dosage entry points of the device library are stubbed HERE (the stub's matrix is host memory): they keep the words that
 * reached them and compute sums and dot products from those words on the CPU, so the driver can compare what
 * STORM_dosage_add packed with what STORM_dosage_add_packed was given, word for word, and with the values it fed in.
 * Never linked into the product. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "storm.h"
#include "stub_dosage.h"

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                        \
        }                                                                   \
    } while (0)

static const storm_hip_matrix_t* g_seen; /* the matrix of the last dosage call */

int storm_hip_dosage_row_sums(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint32_t* h_sum, uint32_t* h_sum_sq) {
    (void)ctx;
    g_seen = m;
    for (uint64_t i = 0; i < m->n_rows; ++i) {
        h_sum[i] = h_sum_sq[i] = 0;
        for (uint64_t s = 0; s < (uint64_t)m->n_words * 32; ++s) {
            h_sum[i] += value_at(m, i, s);
            h_sum_sq[i] += value_at(m, i, s) * value_at(m, i, s);
        }
    }
    return STORM_HIP_OK;
}
int storm_hip_pairw_dosage_matrix_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint32_t* d_out, uint64_t ld) {
    (void)ctx;
    g_seen = m;
    if (ld < m->n_rows) return STORM_HIP_EINVAL;
    for (uint64_t i = 0; i < m->n_rows; ++i)
        for (uint64_t j = i + 1; j < m->n_rows; ++j) {
            uint32_t p = 0;
            for (uint64_t s = 0; s < (uint64_t)m->n_words * 32; ++s) p += value_at(m, i, s) * value_at(m, j, s);
            d_out[i * ld + j] = p;
        }
    return STORM_HIP_OK;
}
int storm_hip_pairw_dosage_matrix(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint32_t* h_out, uint64_t ld) {
    for (uint64_t i = 0; i < m->n_rows; ++i)
        for (uint64_t j = 0; j < m->n_rows; ++j) h_out[i * ld + j] = 0;
    return storm_hip_pairw_dosage_matrix_device(ctx, m, h_out, ld);
}
int storm_hip_pairw_dosage_corr_device(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples,
                                       float* d_out, uint64_t ld) {
    (void)ctx;
    g_seen = m;
    if (ld < m->n_rows || (n_samples + 31) / 32 != m->n_words || measure < 0 || measure > 1) return STORM_HIP_EINVAL;
    for (uint64_t i = 0; i < m->n_rows; ++i) /* (touches the window the real call writes) */
        for (uint64_t j = i + 1; j < m->n_rows; ++j) d_out[i * ld + j] = 0.5f;
    return STORM_HIP_OK;
}
int storm_hip_pairw_dosage_corr(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int measure, uint64_t n_samples, float* h_out,
                                uint64_t ld) {
    for (uint64_t i = 0; i < m->n_rows; ++i)
        for (uint64_t j = 0; j < m->n_rows; ++j) h_out[i * ld + j] = 0.0f;
    return storm_hip_pairw_dosage_corr_device(ctx, m, measure, n_samples, h_out, ld);
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static unsigned next_value(void) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_rng >> 61) & 3u;
}

static void one_shape(uint64_t S, uint64_t n_rows) {
    const uint32_t n_words = (uint32_t)((S + 31) / 32);
    uint8_t* vals = (uint8_t*)malloc((size_t)n_rows * S);
    uint64_t* want = (uint64_t*)calloc((size_t)n_rows * n_words, sizeof(uint64_t));
    CHECK(vals && want);
    for (uint64_t r = 0; r < n_rows; ++r)
        for (uint64_t s = 0; s < S; ++s) {
            const unsigned v = r == 0 ? 3u : next_value(); /* row 0: every bit of the row set */
            vals[r * S + s] = (uint8_t)v;
            want[r * n_words + s / 32] |= (uint64_t)v << (2 * (s % 32));
        }
    STORM_dosage_t* a = STORM_dosage_new(S);
    STORM_dosage_t* b = STORM_dosage_new(S);
    CHECK(a && b);
    for (uint64_t r = 0; r < n_rows; ++r) CHECK(STORM_dosage_add(a, vals + r * S, S) == 0);
    /* packed rows in two calls, so that the container grows in between */
    CHECK(STORM_dosage_add_packed(b, want, n_rows / 2) == 0);
    CHECK(STORM_dosage_add_packed(b, want + (n_rows / 2) * n_words, n_rows - n_rows / 2) == 0);
    CHECK(STORM_dosage_n_rows(a) == n_rows && STORM_dosage_n_rows(b) == n_rows);

    uint32_t* sum = (uint32_t*)malloc(n_rows * sizeof(uint32_t));
    uint32_t* sq = (uint32_t*)malloc(n_rows * sizeof(uint32_t));
    CHECK(sum && sq);
    /* what reached the "device" from either handle, word for word against the layout */
    CHECK(STORM_dosage_row_sums(a, sum, sq) == 0);
    CHECK(g_seen && g_seen->n_rows == n_rows && g_seen->n_words == n_words);
    CHECK(!memcmp(g_seen->rows, want, (size_t)n_rows * n_words * sizeof(uint64_t)));
    for (uint64_t r = 0; r < n_rows; ++r) {
        uint32_t s1 = 0, s2 = 0;
        for (uint64_t s = 0; s < S; ++s) s1 += vals[r * S + s], s2 += (uint32_t)vals[r * S + s] * vals[r * S + s];
        CHECK(sum[r] == s1 && sq[r] == s2); /* the stub sums over the tail too: tail bits are zero */
    }
    CHECK(STORM_dosage_row_sums(b, sum, sq) == 0);
    CHECK(g_seen->n_rows == n_rows && !memcmp(g_seen->rows, want, (size_t)n_rows * n_words * sizeof(uint64_t)));

    /* the per-pair calls: an output with a pitch, nothing outside the n x n window */
    const uint64_t ld = n_rows + 3;
    uint32_t* out = (uint32_t*)malloc((size_t)(n_rows + 1) * ld * sizeof(uint32_t));
    float* fout = (float*)malloc((size_t)(n_rows + 1) * ld * sizeof(float));
    CHECK(out && fout);
    for (uint64_t k = 0; k < (n_rows + 1) * ld; ++k) out[k] = 0xDEADBEEFu, fout[k] = -7.5f;
    CHECK(STORM_dosage_pairw_dot(a, out, n_rows + 1, ld) == 0);
    CHECK(STORM_dosage_pairw_corr(a, STORM_DOSAGE_R, fout, n_rows + 1, ld) == 0);
    for (uint64_t i = 0; i <= n_rows; ++i)
        for (uint64_t j = 0; j < ld; ++j) {
            const int inside = n_rows >= 2 && i < n_rows && j < n_rows;
            if (!inside) CHECK(out[i * ld + j] == 0xDEADBEEFu && fout[i * ld + j] == -7.5f);
            else if (j <= i) CHECK(out[i * ld + j] == 0 && fout[i * ld + j] == 0.0f);
            else {
                uint32_t p = 0;
                for (uint64_t s = 0; s < S; ++s) p += (uint32_t)vals[i * S + s] * vals[j * S + s];
                CHECK(out[i * ld + j] == p);
            }
        }
    CHECK(STORM_dosage_pairw_dot_device(b, out, n_rows, ld) == 0);
    CHECK(STORM_dosage_pairw_corr_device(b, STORM_DOSAGE_R2, fout, n_rows, ld) == 0);
    CHECK(STORM_dosage_pairw_dot(a, out, n_rows, n_rows ? n_rows - 1 : 0) == (n_rows ? -4 : 0));

    /* rows added after a compute call travel on the next one; clear forgets the device copy */
    CHECK(STORM_dosage_add(a, vals, S) == 0);
    uint32_t* sum2 = (uint32_t*)malloc((n_rows + 1) * sizeof(uint32_t));
    uint32_t* sq2 = (uint32_t*)malloc((n_rows + 1) * sizeof(uint32_t));
    CHECK(sum2 && sq2);
    CHECK(STORM_dosage_row_sums(a, sum2, sq2) == 0);
    CHECK(g_seen->n_rows == n_rows + 1 && sum2[n_rows] == sum2[0] && sum2[0] == 3 * S && sq2[n_rows] == 9 * S);
    CHECK(STORM_dosage_clear(a) == 0 && STORM_dosage_n_rows(a) == 0);
    CHECK(STORM_dosage_add(a, vals, S) == 0 && STORM_dosage_row_sums(a, sum2, sq2) == 0 && g_seen->n_rows == 1);

    /* refusals append nothing */
    if (S > 1) CHECK(STORM_dosage_add(a, vals, S - 1) == -3);
    vals[S - 1] = 4;
    CHECK(STORM_dosage_add(a, vals, S) == -3);
    if (S % 32) {
        want[n_words - 1] |= 1ull << (2 * (S % 32));
        CHECK(STORM_dosage_add_packed(a, want, 1) == -3);
    }
    CHECK(STORM_dosage_n_rows(a) == 1);
    CHECK(STORM_hip_error()[0] != '\0');

    STORM_dosage_free(a);
    STORM_dosage_free(b);
    free(vals), free(want), free(sum), free(sq), free(sum2), free(sq2), free(out), free(fout);
}

int main(void) {
    CHECK(STORM_dosage_new(0) == NULL && STORM_dosage_new((1ull << 24) + 1) == NULL);
    CHECK(STORM_dosage_add(NULL, (const uint8_t*)"", 0) == -1 && STORM_dosage_clear(NULL) == -1);
    STORM_dosage_free(NULL);
    const uint64_t samples[] = {1, 2, 31, 32, 33, 63, 64, 65, 1000, 4099};
    const uint64_t rows[] = {1, 2, 3, 70, 130};   /* 70, 130: beyond the first allocation of 64 rows */
    for (size_t a = 0; a < sizeof(samples) / sizeof(samples[0]); ++a)
        for (size_t b = 0; b < sizeof(rows) / sizeof(rows[0]); ++b) one_shape(samples[a], rows[b]);
    /* a handle that is freed while it still holds a device copy, and one that never had one */
    STORM_dosage_t* h = STORM_dosage_new(1 << 24);
    CHECK(h);
    STORM_dosage_free(h);
    STORM_hip_shutdown();
    printf("dosage sanitize: ok\n");
    return 0;
}
