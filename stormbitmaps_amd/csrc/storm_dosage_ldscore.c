/* storm_dosage_ldscore.c — the dosage container's LD scores (storm.h: STORM_dosage_lag_ldscore, _ldscore_complete and
 * their _device forms): for every row the sum of r^2 over the rows within max_lag on both sides of it, reduced on the
 * device from the band storm_dosage_lag.c's corr calls write (storm_hip.h: storm_hip_lag_dosage_ldscore). The container,
 * its device copy and the locked paths are storm_dosage.c's; the order of the checks is storm_dosage_lag.c's. No CPU
 * fallback. */
#include <stdint.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"
#include "storm_dosage_internal.h"

/* the shim call on the container's device copy: 0 or -3 */
static int ldscore_run(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples, uint64_t max_lag,
                       float* score, uint32_t* n_pairs, int complete, int device) {
    static const char* const names[] = {"storm_hip_lag_dosage_ldscore", "storm_hip_lag_dosage_ldscore_complete"};
    int rc;
    if (complete)
        rc = device ? storm_hip_lag_dosage_ldscore_complete_device(ctx, m, stat, n_samples, max_lag, score, n_pairs)
                    : storm_hip_lag_dosage_ldscore_complete(ctx, m, stat, n_samples, max_lag, score, n_pairs);
    else
        rc = device ? storm_hip_lag_dosage_ldscore_device(ctx, m, stat, n_samples, max_lag, score, n_pairs)
                    : storm_hip_lag_dosage_ldscore(ctx, m, stat, n_samples, max_lag, score, n_pairs);
    return storm_dosage_band_result(ctx, rc, device, names[complete]);
}

static int dosage_ldscore(STORM_dosage_t* h, int stat, uint64_t max_lag, float* score, uint32_t* n_pairs, uint64_t out_len,
                          int complete, int device, const char* who) {
    if (!h) return -1;
    if (!score) return -2;
    int rc = storm_host_begin(who);
    const uint64_t n = h->n_rows;
    if (!rc && max_lag != 0 && out_len < n) rc = -4;
    if (!rc && max_lag == 0) rc = storm_host_refuse(who, "max_lag must be at least 1");
    if (!rc) rc = storm_dosage_ldscore_stat_refusal(who, stat, complete, h->n_samples);
    if (!rc && n >= 2) {
        storm_hip_ctx_t* ctx = NULL;
        const storm_hip_matrix_t* m = NULL;
        rc = storm_dosage_operands(h, NULL, &ctx, &m, NULL);
        if (!rc) rc = ldscore_run(ctx, m, stat, h->n_samples, max_lag, score, n_pairs, complete, device);
    }
    return storm_host_end(rc);
}

int STORM_dosage_lag_ldscore(STORM_dosage_t* h, int stat, uint64_t max_lag, float* score, uint32_t* n_pairs, uint64_t out_len) {
    return dosage_ldscore(h, stat, max_lag, score, n_pairs, out_len, 0, 0, "STORM_dosage_lag_ldscore");
}
int STORM_dosage_lag_ldscore_device(STORM_dosage_t* h, int stat, uint64_t max_lag, float* d_score, uint32_t* d_n_pairs,
                                    uint64_t out_len) {
    return dosage_ldscore(h, stat, max_lag, d_score, d_n_pairs, out_len, 0, 1, "STORM_dosage_lag_ldscore_device");
}
int STORM_dosage_lag_ldscore_complete(STORM_dosage_t* h, int stat, uint64_t max_lag, float* score, uint32_t* n_pairs,
                                      uint64_t out_len) {
    return dosage_ldscore(h, stat, max_lag, score, n_pairs, out_len, 1, 0, "STORM_dosage_lag_ldscore_complete");
}
int STORM_dosage_lag_ldscore_complete_device(STORM_dosage_t* h, int stat, uint64_t max_lag, float* d_score, uint32_t* d_n_pairs,
                                             uint64_t out_len) {
    return dosage_ldscore(h, stat, max_lag, d_score, d_n_pairs, out_len, 1, 1, "STORM_dosage_lag_ldscore_complete_device");
}
