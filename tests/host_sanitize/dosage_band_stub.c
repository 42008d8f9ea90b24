/* dosage_band_stub.c — TEST ONLY. The entry points of the device library that reduce the band of r^2 (LD scores, stratified LD
 * scores, prune / clump) and storm_hip_ctx_synchronize, for dosage_ldscore_driver.c, dosage_ldscore_annot_driver.c and
 * dosage_prune_driver.c, beside device_stub.c (whose matrix is host memory): every call computes its result from the words
 * that reached it, sample by sample on the CPU, in host memory, and writes exactly what the real call writes — rows [0, n)
 * of its outputs (columns [0, n_annot) of the stratified scores) and, where given, of n_pairs / owner. Never linked into the
 * product. */
#include <stdlib.h>

#include "stub_dosage.h"

int storm_hip_ctx_synchronize(storm_hip_ctx_t* ctx) { return ctx ? STORM_HIP_OK : STORM_HIP_EINVAL; }

/* the refusals every band call makes first */
static int band_refusal(const storm_hip_matrix_t* m, const void* out, uint64_t n_samples, uint64_t max_lag) {
    return !m || !out || max_lag == 0 || (n_samples + 31) / 32 != m->n_words;
}
static int stat_refusal(int stat) { return stat != STORM_HIP_LDSCORE_R2 && stat != STORM_HIP_LDSCORE_R2_ADJ; }

/* pair (i, j)'s term of an LD score, either way round; 0 where the real call skips the pair */
static int pair_term(const storm_hip_matrix_t* m, uint64_t i, uint64_t j, int stat, int missing, uint64_t n_samples, double* t) {
    uint64_t n_obs = 0;
    const float rho = j < i ? pair_r2(m, j, i, missing, n_samples, &n_obs) : pair_r2(m, i, j, missing, n_samples, &n_obs);
    if (isnan(rho) || (stat == STORM_HIP_LDSCORE_R2_ADJ && n_obs < 3)) return 0;
    *t = stat == STORM_HIP_LDSCORE_R2_ADJ ? (double)rho - (1.0 - (double)rho) / (double)(n_obs - 2) : (double)rho;
    return 1;
}

static int ldscore_call(const storm_hip_matrix_t* m, int stat, uint64_t n_samples, uint64_t max_lag, int missing, float* score,
                        uint32_t* n_pairs) {
    if (band_refusal(m, score, n_samples, max_lag) || stat_refusal(stat)) return STORM_HIP_EINVAL;
    const uint64_t n = m->n_rows;
    if (n < 2) return STORM_HIP_OK;
    const uint64_t lag = max_lag < n - 1 ? max_lag : n - 1;
    for (uint64_t i = 0; i < n; ++i) {
        double sum = 0, t;
        uint32_t pairs = 0;
        for (uint64_t j = i > lag ? i - lag : 0; j < n && j <= i + lag; ++j) {
            if (j == i || !pair_term(m, i, j, stat, missing, n_samples, &t)) continue;
            sum += t;
            ++pairs;
        }
        score[i] = (float)sum;
        if (n_pairs) n_pairs[i] = pairs;
    }
    return STORM_HIP_OK;
}

static int annot_call(const storm_hip_matrix_t* m, int stat, uint64_t n_samples, uint64_t max_lag, int missing, const uint32_t* lo,
                      const uint32_t* hi, const float* annot, uint64_t annot_ld, uint64_t n_annot, float* score, uint64_t score_ld,
                      uint32_t* n_pairs) {
    if (band_refusal(m, score, n_samples, max_lag) || stat_refusal(stat)) return STORM_HIP_EINVAL;
    if (!annot || n_annot < 1 || n_annot > 1024 || annot_ld < n_annot || score_ld < n_annot || !lo != !hi) return STORM_HIP_EINVAL;
    const uint64_t n = m->n_rows;
    if (n < 2) return STORM_HIP_OK;
    const uint64_t lag = max_lag < n - 1 ? max_lag : n - 1;
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t pairs = 0;
        for (uint64_t c = 0; c < n_annot; ++c) {
            double sum = 0, t;
            pairs = 0;
            for (uint64_t j = i > lag ? i - lag : 0; j < n && j <= i + lag; ++j) {
                if (j == i || (lo && (j < lo[i] || j > hi[i])) || !pair_term(m, i, j, stat, missing, n_samples, &t)) continue;
                sum = fma(t, (double)annot[j * annot_ld + c], sum);
                ++pairs;
            }
            score[i * score_ld + c] = (float)sum;
        }
        if (n_pairs) n_pairs[i] = pairs;
    }
    return STORM_HIP_OK;
}

/* the plain greedy over the pairs' r^2 */
static int prune_call(const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag, float min_r2, int missing,
                      const uint32_t* lo, const uint32_t* hi, const uint32_t* order, uint8_t* keep, uint32_t* owner) {
    if (band_refusal(m, keep, n_samples, max_lag)) return STORM_HIP_EINVAL;
    if (!lo != !hi || m->n_rows > (1u << 20) || isnan(min_r2)) return STORM_HIP_EINVAL;
    const uint64_t n = m->n_rows;
    if (n == 0) return STORM_HIP_OK;
    const uint64_t lag = max_lag < n - 1 ? max_lag : n - 1;
    uint8_t* marked = (uint8_t*)calloc(n, 1);
    if (!marked) return STORM_HIP_ENOMEM;
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t v = order ? order[k] : k;
        if (marked[v]) {
            keep[v] = 0;
            continue;
        }
        keep[v] = 1;
        if (owner) owner[v] = (uint32_t)v;
        for (uint64_t j = v > lag ? v - lag : 0; j < n && j <= v + lag; ++j) {
            if (j == v || marked[j]) continue;
            const uint64_t a = j < v ? j : v, b = j < v ? v : j;
            uint64_t n_obs = 0;
            if (lo && !(b <= hi[a] && a >= lo[b])) continue;
            if (pair_r2(m, a, b, missing, n_samples, &n_obs) > min_r2) {   /* (a row kept earlier is never adjacent: v would be marked) */
                marked[j] = 1;
                if (owner) owner[j] = (uint32_t)v;
            }
        }
    }
    free(marked);
    return STORM_HIP_OK;
}

/* ---- the entry points: host and _device forms are one here, `missing` tells the pairwise-complete ones ---- */
#define LDSCORE_ENTRY(name, missing)                                                                                        \
    int name(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples, uint64_t max_lag, float* score, \
             uint32_t* n_pairs) {                                                                                           \
        (void)ctx;                                                                                                          \
        return ldscore_call(m, stat, n_samples, max_lag, missing, score, n_pairs);                                          \
    }
LDSCORE_ENTRY(storm_hip_lag_dosage_ldscore_device, 0)
LDSCORE_ENTRY(storm_hip_lag_dosage_ldscore, 0)
LDSCORE_ENTRY(storm_hip_lag_dosage_ldscore_complete_device, 1)
LDSCORE_ENTRY(storm_hip_lag_dosage_ldscore_complete, 1)

#define ANNOT_ENTRY(name, missing)                                                                                             \
    int name(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples, uint64_t max_lag,                \
             const uint32_t* h_lo, const uint32_t* h_hi, const float* annot, uint64_t annot_ld, uint64_t n_annot, float* score, \
             uint64_t score_ld, uint32_t* n_pairs) {                                                                           \
        (void)ctx;                                                                                                             \
        return annot_call(m, stat, n_samples, max_lag, missing, h_lo, h_hi, annot, annot_ld, n_annot, score, score_ld, n_pairs); \
    }
ANNOT_ENTRY(storm_hip_lag_dosage_ldscore_annot_device, 0)
ANNOT_ENTRY(storm_hip_lag_dosage_ldscore_annot, 0)
ANNOT_ENTRY(storm_hip_lag_dosage_ldscore_annot_complete_device, 1)
ANNOT_ENTRY(storm_hip_lag_dosage_ldscore_annot_complete, 1)

#define PRUNE_ENTRY(name, missing)                                                                                         \
    int name(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, uint64_t n_samples, uint64_t max_lag, float min_r2,         \
             const uint32_t* h_lo, const uint32_t* h_hi, const uint32_t* h_order, uint8_t* keep, uint32_t* owner) {         \
        (void)ctx;                                                                                                         \
        return prune_call(m, n_samples, max_lag, min_r2, missing, h_lo, h_hi, h_order, keep, owner);                       \
    }
PRUNE_ENTRY(storm_hip_lag_dosage_prune_device, 0)
PRUNE_ENTRY(storm_hip_lag_dosage_prune, 0)
PRUNE_ENTRY(storm_hip_lag_dosage_prune_complete_device, 1)
PRUNE_ENTRY(storm_hip_lag_dosage_prune_complete, 1)
