/* dosage_ldscore_annot_driver.c — TEST ONLY. The host entry points of the dosage container's stratified LD scores
 * (stormbitmaps_amd/csrc/storm_dosage_ldscore_annot.c and the planner storm_ldscore_window.c, on storm_dosage.c and
 * storm_host.c's locked paths) as a stand-alone program for AddressSanitizer / UBSan, on device_stub.c,
 * dosage_complete_stub.c and dosage_band_stub.c: outputs of exactly n x C elements (a write
 * behind them is a heap overflow), score_ld > C with the pitch elements untouched, windows that need exactly max_lag rows
 * and one row more than max_lag, every refusal with nothing written. Never linked into the product. */
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

typedef int (*annot_call)(STORM_dosage_t*, int, uint64_t, const double*, double, const float*, uint64_t, uint64_t, float*, uint64_t,
                          uint32_t*, uint64_t);
static const annot_call calls[4] = {STORM_dosage_lag_ldscore_annot, STORM_dosage_lag_ldscore_annot_device,
                                    STORM_dosage_lag_ldscore_annot_complete, STORM_dosage_lag_ldscore_annot_complete_device};
static const char* const names[4] = {"STORM_dosage_lag_ldscore_annot:", "STORM_dosage_lag_ldscore_annot_device:",
                                     "STORM_dosage_lag_ldscore_annot_complete:", "STORM_dosage_lag_ldscore_annot_complete_device:"};

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

/* pos NULL: the window is L rows on each side; else the rows within max_dist, at most L away (the call was not refused) */
static void check_outputs(const uint8_t* v, uint64_t S, uint64_t n, uint64_t L, const double* pos, double max_dist, int missing,
                          int stat, const float* annot, uint64_t annot_ld, uint64_t C, const float* score, uint64_t score_ld,
                          const uint32_t* n_pairs) {
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t c = 0; c < C; ++c) {
            double sum = 0, mag = 0, t;
            uint32_t m = 0;
            for (uint64_t j = 0; j < n; ++j) {
                if (j == i) continue;
                if (pos ? fabs(pos[j] - pos[i]) > max_dist : (j > i ? j - i : i - j) > L) continue;
                if (pair_term(v, S, j < i ? j : i, j < i ? i : j, missing, stat, &t))
                    sum += t * annot[j * annot_ld + c], mag += fabs(t * annot[j * annot_ld + c]), ++m;
            }
            CHECK(!n_pairs || n_pairs[i] == m);
            CHECK(fabs((double)score[i * score_ld + c] - sum) <= 1e-5 * (mag + 1.0));
            if (m == 0) CHECK(score[i * score_ld + c] == 0.0f && !signbit(score[i * score_ld + c]));
        }
}

static void one_shape(uint64_t S, uint64_t n, uint64_t C, uint64_t extra) {
    STORM_dosage_t* h = STORM_dosage_new(S);
    CHECK(h);
    uint8_t* v = (uint8_t*)malloc((size_t)(n ? n : 1) * S);
    CHECK(v);
    for (uint64_t r = 0; r < n; ++r) {
        for (uint64_t s = 0; s < S; ++s) v[r * S + s] = (uint8_t)(r == 0 ? 3u : next_bits() & 3u);   /* row 0: all missing */
        CHECK(STORM_dosage_add(h, v + r * S, S) == 0);
    }
    /* buffers of exactly n rows: the last row of score and annot ends at column C, not at the pitch */
    const uint64_t annot_ld = C + extra, score_ld = C + 2 * extra;
    const size_t annot_len = n ? (size_t)(n - 1) * annot_ld + C : 1, score_len = n ? (size_t)(n - 1) * score_ld + C : 1;
    float* annot = (float*)malloc(annot_len * sizeof(float));
    float* score = (float*)malloc(score_len * sizeof(float));
    uint32_t* pairs = (uint32_t*)malloc((n ? n : 1) * sizeof(uint32_t));
    double* pos = (double*)malloc((n ? n : 1) * sizeof(double));
    CHECK(annot && score && pairs && pos);
    for (size_t k = 0; k < annot_len; ++k) annot[k] = (float)((int)(next_bits() % 9u) - 4) * 0.25f;   /* zeros and negatives */
    /* positions with a tie and a gap; need = the lag the windows need under max_dist 3 */
    for (uint64_t i = 0; i < n; ++i) pos[i] = (double)(i - (i % 5 == 1 ? 1 : 0)) + (i >= n / 2 ? 10.0 : 0.0);
    const double max_dist = 3.0;
    uint64_t need = 777;
    CHECK(STORM_ldscore_window_lag(pos, n, max_dist, &need) == 0);
    CHECK(n >= 3 ? need >= 1 && need < n : need == 0);   /* (two rows: the gap lies between them) */

#define FILL()                                                            \
    do {                                                                  \
        for (size_t k_ = 0; k_ < score_len; ++k_) score[k_] = -77.5f;     \
        for (uint64_t k_ = 0; k_ < n; ++k_) pairs[k_] = 0xDEADBEEFu;      \
    } while (0)
#define UNTOUCHED()                                                               \
    do {                                                                          \
        for (size_t k_ = 0; k_ < score_len; ++k_) CHECK(score[k_] == -77.5f);     \
        for (uint64_t k_ = 0; k_ < n; ++k_) CHECK(pairs[k_] == 0xDEADBEEFu);      \
    } while (0)
#define PITCH_UNTOUCHED()                                                                             \
    do {                                                                                              \
        for (uint64_t i_ = 0; i_ + 1 < n; ++i_)                                                       \
            for (uint64_t c_ = C; c_ < score_ld; ++c_) CHECK(score[i_ * score_ld + c_] == -77.5f);    \
    } while (0)

    for (int k = 0; k < 4; ++k)
        for (int stat = 0; stat < 2; ++stat)
            for (int with_pairs = 0; with_pairs < 2; ++with_pairs) {
                const int missing = k >= 2;
                uint32_t* const p = with_pairs ? pairs : NULL;
                if (!missing && stat == STORM_LDSCORE_R2_ADJ && S < 3) {   /* no n_samples - 2 to divide by */
                    FILL();
                    CHECK(calls[k](h, stat, 4, NULL, 0, annot, C, annot_ld, score, score_ld, p, n) == -3);
                    CHECK(strstr(STORM_hip_error(), "3 samples"));
                    UNTOUCHED();
                    continue;
                }
                /* a count window: pos NULL, max_dist ignored (NaN) */
                FILL();
                CHECK(calls[k](h, stat, 4, NULL, NAN, annot, C, annot_ld, score, score_ld, p, n) == 0);
                if (n < 2) {
                    UNTOUCHED();
                } else {
                    check_outputs(v, S, n, 4, NULL, 0, missing, stat, annot, annot_ld, C, score, score_ld, p);
                    PITCH_UNTOUCHED();
                    if (!with_pairs)
                        for (uint64_t i = 0; i < n; ++i) CHECK(pairs[i] == 0xDEADBEEFu);
                    if (missing && with_pairs) CHECK(pairs[0] == 0 && score[0] == 0.0f);   /* row 0 shares nothing with anybody */
                }
                /* positions: max_lag 0 (what the windows need), exactly what they need, far more, and one row too few */
                const uint64_t lags[3] = {0, need, need + 1000};
                for (int l = 0; l < 3; ++l) {
                    if (n >= 2 && l == 1 && need == 0) continue;
                    FILL();
                    CHECK(calls[k](h, stat, lags[l], pos, max_dist, annot, C, annot_ld, score, score_ld, p, n) == 0);
                    if (n < 2) {
                        UNTOUCHED();
                        continue;
                    }
                    check_outputs(v, S, n, 0, pos, max_dist, missing, stat, annot, annot_ld, C, score, score_ld, p);
                    PITCH_UNTOUCHED();
                }
                if (need >= 2) {
                    char both[64];
                    FILL();
                    CHECK(calls[k](h, stat, need - 1, pos, max_dist, annot, C, annot_ld, score, score_ld, p, n) == -3);
                    snprintf(both, sizeof(both), "%llu rows, max_lag is %llu", (unsigned long long)need, (unsigned long long)(need - 1));
                    CHECK(strstr(STORM_hip_error(), both) && strstr(STORM_hip_error(), names[k]));
                    UNTOUCHED();
                }
                /* every window empty: max_dist 0 on distinct positions still answers (+0.0f, 0 pairs) */
                if (n >= 2) {
                    double* apart = (double*)malloc(n * sizeof(double));
                    CHECK(apart);
                    for (uint64_t i = 0; i < n; ++i) apart[i] = (double)i;
                    FILL();
                    CHECK(calls[k](h, stat, 0, apart, 0.0, annot, C, annot_ld, score, score_ld, p, n) == 0);
                    check_outputs(v, S, n, 0, apart, 0.0, missing, stat, annot, annot_ld, C, score, score_ld, p);
                    for (uint64_t i = 0; i < n; ++i) CHECK(!p || p[i] == 0);
                    free(apart);
                }
            }

    /* refusals at this geometry, in their order: nothing is written */
    FILL();
    for (int k = 0; k < 4; ++k) {
        CHECK(calls[k](NULL, 0, 4, NULL, 0, annot, C, annot_ld, score, score_ld, pairs, n) == -1);
        CHECK(calls[k](h, 0, 4, NULL, 0, annot, C, annot_ld, NULL, score_ld, pairs, n) == -2);
        CHECK(calls[k](h, 0, 4, NULL, 0, NULL, C, annot_ld, score, score_ld, pairs, n) == -2);
        if (n) CHECK(calls[k](h, 0, 4, NULL, 0, annot, C, annot_ld, score, score_ld, pairs, n - 1) == -4);
        if (n) CHECK(calls[k](h, 7, 4, pos, -1.0, annot, 0, 0, score, 0, NULL, n - 1) == -4);   /* the size before the rest */
        CHECK(calls[k](h, 0, 0, NULL, 0, annot, C, annot_ld, score, score_ld, pairs, n) == -3 && strstr(STORM_hip_error(), "max_lag"));
        CHECK(calls[k](h, 0, 0, NULL, 0, annot, C, annot_ld, score, score_ld, pairs, 0) == -3 && strstr(STORM_hip_error(), "max_lag"));
        CHECK(calls[k](h, 2, 4, NULL, 0, annot, C, annot_ld, score, score_ld, pairs, n) == -3 && strstr(STORM_hip_error(), "stat"));
        CHECK(calls[k](h, -1, 4, pos, -1.0, annot, 0, annot_ld, score, score_ld, pairs, n) == -3 && strstr(STORM_hip_error(), "stat"));
        if (S >= 3 || k >= 2) {
            CHECK(calls[k](h, 1, 4, NULL, 0, annot, 0, annot_ld, score, score_ld, pairs, n) == -3 && strstr(STORM_hip_error(), "n_annot"));
            CHECK(calls[k](h, 1, 4, NULL, 0, annot, 1025, 1025, score, 1025, pairs, n) == -3 && strstr(STORM_hip_error(), "n_annot"));
            CHECK(calls[k](h, 1, 4, pos, -1.0, annot, C, C - 1, score, score_ld, pairs, n) == -4);   /* before the positions */
            CHECK(calls[k](h, 1, 4, NULL, 0, annot, C, annot_ld, score, C - 1, pairs, n) == -4);
            CHECK(calls[k](h, 1, 4, pos, -1.0, annot, C, annot_ld, score, score_ld, pairs, n) == -3 && strstr(STORM_hip_error(), "max_dist"));
            CHECK(calls[k](h, 1, 0, pos, NAN, annot, C, annot_ld, score, score_ld, pairs, n) == -3 && strstr(STORM_hip_error(), "max_dist"));
            if (n >= 3) {
                const double keep = pos[n - 2];
                pos[n - 2] = INFINITY;
                CHECK(calls[k](h, 1, 0, pos, 3.0, annot, C, annot_ld, score, score_ld, pairs, n) == -3);
                CHECK(strstr(STORM_hip_error(), "is not finite") && strstr(STORM_hip_error(), "pos["));
                pos[n - 2] = pos[n - 3] - 1.0;
                CHECK(calls[k](h, 1, 0, pos, 3.0, annot, C, annot_ld, score, score_ld, pairs, n) == -3);
                CHECK(strstr(STORM_hip_error(), "must not decrease"));
                pos[n - 2] = keep;
            }
            if (n && !(k & 1)) {   /* the host forms look at every annotation; the first offender is named */
                char where[64];
                const uint64_t r = n - 1, c = C - 1;
                const float keep = annot[r * annot_ld + c];
                annot[r * annot_ld + c] = NAN;
                CHECK(calls[k](h, 1, 4, NULL, 0, annot, C, annot_ld, score, score_ld, pairs, n) == -3);
                snprintf(where, sizeof(where), "annot[%llu][%llu] is not finite", (unsigned long long)r, (unsigned long long)c);
                CHECK(strstr(STORM_hip_error(), where));
                annot[r * annot_ld + c] = keep;
            }
        }
    }
    /* several device slots in view: -5 from every call, which names itself, ahead of the other checks; one slot again after */
    {
        const int three[3] = {0, 0, 0}, one[1] = {0};
        CHECK(STORM_hip_set_devices(3, three) == 0);
        for (int k = 0; k < 4; ++k) {
            CHECK(calls[k](h, 0, 4, pos, max_dist, annot, C, annot_ld, score, score_ld, pairs, n) == -5 && strstr(STORM_hip_error(), names[k]));
            CHECK(calls[k](h, 9, 0, NULL, 0, annot, 0, 0, score, 0, NULL, 0) == -5 && strstr(STORM_hip_error(), "ONE device"));
        }
        CHECK(STORM_hip_set_devices(1, one) == 0);
    }
    UNTOUCHED();
    STORM_dosage_free(h);
    free(v), free(annot), free(score), free(pairs), free(pos);
}

int main(void) {
    uint64_t lag = 5;
    CHECK(STORM_ldscore_window_lag(NULL, 0, 1.0, &lag) == 0 && lag == 0);
    CHECK(STORM_ldscore_window_lag(NULL, 3, 1.0, &lag) == -2 && STORM_ldscore_window_lag(NULL, 0, 1.0, NULL) == -2);
    const uint64_t samples[] = {1, 2, 33, 65};
    const uint64_t shapes[][3] = {{0, 1, 0}, {1, 1, 0}, {1, 3, 2}, {2, 1, 0}, {2, 2, 1}, {3, 5, 0}, {12, 1, 1}, {12, 3, 2}, {41, 4, 0}};   /* rows, columns, pitch extra */
    for (size_t s = 0; s < sizeof(samples) / sizeof(samples[0]); ++s)
        for (size_t r = 0; r < sizeof(shapes) / sizeof(shapes[0]); ++r) one_shape(samples[s], shapes[r][0], shapes[r][1], shapes[r][2]);
    STORM_hip_shutdown();
    printf("dosage ldscore annot sanitize: ok\n");
    return 0;
}
