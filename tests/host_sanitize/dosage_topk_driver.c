/* dosage_topk_driver.c — TEST ONLY. The host entry points of the dosage container's top-k calls
 * (stormbitmaps_amd/csrc/storm_dosage_topk.c on storm_dosage.c and storm_host.c's locked paths) as a stand-alone program for
 * AddressSanitizer / UBSan, on device_stub.c, dosage_complete_stub.c, dosage_band_stub.c and dosage_topk_stub.c: outputs of
 * exactly n x k entries — a write outside the window is a heap overflow there — and with a pitch, every refusal, empty
 * containers on either side, rows added between calls. Never linked into the product. */
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

#define FILL 0xDEADBEEFu
#define NAN_BITS 0x7FC00000u
#define NO_INDEX 0xFFFFFFFFu

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static unsigned next_value(void) {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(g_rng >> 61) & 3u;
}

typedef int (*pairw_call)(STORM_dosage_t*, int, uint64_t, uint64_t, uint32_t*, void*, uint64_t, uint64_t);
typedef int (*square_call)(STORM_dosage_t*, STORM_dosage_t*, int, uint64_t, uint64_t, uint32_t*, void*, uint64_t, uint64_t);
static const pairw_call PAIRW[4] = {STORM_dosage_pairw_topk, STORM_dosage_pairw_topk_device, STORM_dosage_pairw_topk_complete,
                                    STORM_dosage_pairw_topk_complete_device};
static const square_call SQUARE[4] = {STORM_dosage_square_topk, STORM_dosage_square_topk_device, STORM_dosage_square_topk_complete,
                                      STORM_dosage_square_topk_complete_device};

/* form 0 .. 3: PAIRW (b unused), 4 .. 7: SQUARE */
static int call_form(int form, STORM_dosage_t* a, STORM_dosage_t* b, int score, uint64_t k, uint64_t panel_rows, uint32_t* idx, void* val,
                     uint64_t rows, uint64_t ld) {
    return form < 4 ? PAIRW[form](a, score, k, panel_rows, idx, val, rows, ld) : SQUARE[form - 4](a, b, score, k, panel_rows, idx, val, rows, ld);
}

static STORM_dosage_t* filled(uint64_t S, uint64_t n, uint8_t** values) {
    STORM_dosage_t* h = STORM_dosage_new(S);
    CHECK(h);
    uint8_t* v = (uint8_t*)malloc((size_t)(n ? n : 1) * S);
    CHECK(v);
    for (uint64_t r = 0; r < n; ++r) {
        for (uint64_t s = 0; s < S; ++s) v[r * S + s] = (uint8_t)(r == 1 ? 3u : next_value());   /* row 1: all missing */
        CHECK(STORM_dosage_add(h, v + r * S, S) == 0);
    }
    *values = v;
    return h;
}

static void one_shape(uint64_t S, uint64_t na, uint64_t nb, uint64_t k) {
    uint8_t *va, *vb;
    STORM_dosage_t* a = filled(S, na, &va);
    STORM_dosage_t* b = filled(S, nb, &vb);
    /* two geometries: exactly n_a x k (an allocation of that size), and a row more with a pitch */
    for (int pitch = 0; pitch < 2; ++pitch) {
        const uint64_t rows = na + (pitch ? 1 : 0), ld = k + (pitch ? 3 : 0);
        const size_t count = (size_t)rows * ld;
        uint32_t* idx = (uint32_t*)malloc((count ? count : 1) * sizeof(uint32_t));
        uint32_t* val = (uint32_t*)malloc((count ? count : 1) * sizeof(uint32_t));
        CHECK(idx && val);
        for (int form = 0; form < 8; ++form) {
            const int complete = (form & 2) != 0, square = form >= 4;
            const uint64_t n_cols = square ? nb : na;
            const uint8_t* vc = square ? vb : va;
            for (int score = 0; score < (complete ? 2 : 3); ++score) {
                for (size_t t = 0; t < count; ++t) idx[t] = val[t] = FILL;
                CHECK(call_form(form, a, b, score, k, pitch ? 256 : 0, idx, val, rows, ld) == 0);
                for (uint64_t i = 0; i < rows; ++i)
                    for (uint64_t t = 0; t < ld; ++t) {
                        const uint32_t gi = idx[i * ld + t], gv = val[i * ld + t];
                        if (i >= na || t >= k) {   /* outside the window */
                            CHECK(gi == FILL && gv == FILL);
                            continue;
                        }
                        if (gi == NO_INDEX) {      /* padding, and only padding behind it */
                            CHECK(gv == (score == STORM_DOSAGE_TOPK_DOT ? 0u : NAN_BITS));
                            CHECK(t + 1 == k || idx[i * ld + t + 1] == NO_INDEX);
                            continue;
                        }
                        CHECK(gi < n_cols && (square || gi != i));
                        CHECK(!(complete && (gi == 1 || i == 1)));   /* the row without a sample is nobody's neighbour */
                        if (score == STORM_DOSAGE_TOPK_DOT) {
                            uint32_t want = 0;
                            for (uint64_t s = 0; s < S; ++s) want += (uint32_t)va[i * S + s] * vc[gi * S + s];
                            CHECK(gv == want);
                            /* every candidate is listed while there is room */
                            CHECK(t < (square ? n_cols : n_cols - 1));
                        } else {
                            float f;
                            memcpy(&f, &gv, sizeof(f));
                            CHECK(!isnan(f) && f >= -1.0001f && f <= 1.0001f);
                        }
                        if (t > 0) {               /* value descending, then row ascending */
                            const uint32_t pi = idx[i * ld + t - 1], pv = val[i * ld + t - 1];
                            if (score == STORM_DOSAGE_TOPK_DOT) CHECK(pv > gv || (pv == gv && pi < gi));
                            else {
                                float f, g;
                                memcpy(&f, &pv, sizeof(f));
                                memcpy(&g, &gv, sizeof(g));
                                CHECK(f > g || (f == g && pi < gi));
                            }
                        }
                    }
                if (score == STORM_DOSAGE_TOPK_DOT)   /* the dot product pads only when the candidates run out */
                    for (uint64_t i = 0; i < na; ++i) {
                        const uint64_t cand = square ? n_cols : n_cols - 1;
                        for (uint64_t t = 0; t < k; ++t) CHECK((idx[i * ld + t] == NO_INDEX) == (t >= cand));
                    }
            }
            /* refusals at this geometry: nothing is written */
            for (size_t t = 0; t < count; ++t) idx[t] = val[t] = FILL;
            if (na) CHECK(call_form(form, a, b, 0, k, 0, idx, val, na - 1, ld) == -4);
            CHECK(call_form(form, a, b, 0, k, 0, idx, val, rows, k - 1) == -4);
            CHECK(call_form(form, a, b, 0, k, 0, NULL, val, rows, ld) == -2 && call_form(form, a, b, 0, k, 0, idx, NULL, rows, ld) == -2);
            CHECK(call_form(form, a, b, 3, k, 0, idx, val, rows, ld) == -3 && call_form(form, a, b, -1, k, 0, idx, val, rows, ld) == -3);
            if (complete) CHECK(call_form(form, a, b, STORM_DOSAGE_TOPK_DOT, k, 0, idx, val, rows, ld) == -3);
            CHECK(call_form(form, a, b, 0, 0, 0, idx, val, rows, ld) == -3);
            CHECK(call_form(form, a, b, 0, k, 100, idx, val, rows, ld) == -3);
            CHECK(STORM_hip_error()[0] != '\0');
            for (size_t t = 0; t < count; ++t) CHECK(idx[t] == FILL && val[t] == FILL);
        }
        free(idx), free(val);
    }

    /* a row added after a compute call travels on the next one: two copies of one row are each other's best neighbour */
    if (S >= 2) {
        uint8_t* row = (uint8_t*)malloc(S);
        CHECK(row);
        for (uint64_t s = 0; s < S; ++s) row[s] = (uint8_t)(s % 3);
        CHECK(STORM_dosage_add(a, row, S) == 0 && STORM_dosage_add(a, row, S) == 0);
        const uint64_t n2 = na + 2;
        uint32_t* idx2 = (uint32_t*)malloc(n2 * sizeof(uint32_t));
        float* val2 = (float*)malloc(n2 * sizeof(float));
        CHECK(idx2 && val2);
        CHECK(STORM_dosage_pairw_topk(a, STORM_DOSAGE_R2, 1, 0, idx2, val2, n2, 1) == 0);
        CHECK(idx2[na] == na + 1 && val2[na] == 1.0f);
        CHECK(STORM_dosage_pairw_topk_complete_device(a, STORM_DOSAGE_R, 1, 256, idx2, val2, n2, 1) == 0);
        CHECK(idx2[na + 1] == na && val2[na + 1] == 1.0f);
        free(row), free(idx2), free(val2);
    }
    STORM_dosage_free(a);
    STORM_dosage_free(b);
    free(va), free(vb);
}

int main(void) {
    uint32_t word = 0;
    STORM_dosage_t *h = STORM_dosage_new(5), *wider = STORM_dosage_new(6);
    CHECK(h && wider);
    for (int form = 0; form < 8; ++form) {
        CHECK(call_form(form, NULL, h, 0, 1, 0, &word, &word, 1, 1) == -1);
        if (form >= 4) CHECK(call_form(form, h, NULL, 0, 1, 0, &word, &word, 1, 1) == -1);
        if (form >= 4) CHECK(call_form(form, h, wider, 0, 1, 0, &word, &word, 1, 1) == -3);   /* unequal samples, ahead of the empty a */
        CHECK(call_form(form, h, h, 0, 129, 0, &word, &word, 1, 129) == -3);
        CHECK(call_form(form, h, h, 0, 1, 0, &word, &word, 0, 1) == 0 && word == 0);           /* an empty a: nothing written */
    }
    STORM_dosage_free(h);
    STORM_dosage_free(wider);
    const uint64_t samples[] = {1, 31, 33, 65, 300};
    const uint64_t shapes[][3] = {{0, 3, 2}, {1, 0, 3}, {1, 1, 1}, {2, 5, 8}, {5, 3, 8}, {70, 9, 4}, {40, 130, 128}, {130, 40, 17}};   /* n_a, n_b, k */
    for (size_t s = 0; s < sizeof(samples) / sizeof(samples[0]); ++s)
        for (size_t r = 0; r < sizeof(shapes) / sizeof(shapes[0]); ++r) one_shape(samples[s], shapes[r][0], shapes[r][1], shapes[r][2]);
    STORM_hip_shutdown();
    printf("dosage topk sanitize: ok\n");
    return 0;
}
