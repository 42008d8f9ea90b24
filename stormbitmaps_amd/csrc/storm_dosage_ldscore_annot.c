/* storm_dosage_ldscore_annot.c — the dosage container's stratified LD scores in a distance window (storm.h:
 * STORM_dosage_lag_ldscore_annot, _annot_complete and their _device forms): for every row and every annotation column the sum
 * of a[j][c] r^2(i, j) over the rows j of row i's window, reduced on the device from the band storm_dosage_lag.c's corr
 * calls write (storm_hip.h: storm_hip_lag_dosage_ldscore_annot). The windows are resolved in storm_dosage_band.c; the
 * container, its device copy and the locked paths are storm_dosage.c's; the order of the checks is storm_dosage_ldscore.c's,
 * then the new ones. No CPU fallback. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"
#include "storm_dosage_internal.h"

/* the shim call on the container's device copy: 0 or -3 */
static int annot_run(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* m, int stat, uint64_t n_samples, uint64_t lag,
                     const uint32_t* lo, const uint32_t* hi, const float* annot, uint64_t annot_ld, uint64_t n_annot, float* score,
                     uint64_t score_ld, uint32_t* n_pairs, int complete, int device) {
    static const char* const names[] = {"storm_hip_lag_dosage_ldscore_annot", "storm_hip_lag_dosage_ldscore_annot_complete"};
    int rc;
    if (complete)
        rc = device ? storm_hip_lag_dosage_ldscore_annot_complete_device(ctx, m, stat, n_samples, lag, lo, hi, annot, annot_ld, n_annot,
                                                                         score, score_ld, n_pairs)
                    : storm_hip_lag_dosage_ldscore_annot_complete(ctx, m, stat, n_samples, lag, lo, hi, annot, annot_ld, n_annot, score,
                                                                  score_ld, n_pairs);
    else
        rc = device ? storm_hip_lag_dosage_ldscore_annot_device(ctx, m, stat, n_samples, lag, lo, hi, annot, annot_ld, n_annot, score,
                                                                score_ld, n_pairs)
                    : storm_hip_lag_dosage_ldscore_annot(ctx, m, stat, n_samples, lag, lo, hi, annot, annot_ld, n_annot, score,
                                                         score_ld, n_pairs);
    return storm_dosage_band_result(ctx, rc, device, names[complete]);
}

static int dosage_ldscore_annot(STORM_dosage_t* h, int stat, uint64_t max_lag, const double* pos, double max_dist, const float* annot,
                                uint64_t n_annot, uint64_t annot_ld, float* score, uint64_t score_ld, uint32_t* n_pairs,
                                uint64_t out_rows, int complete, int device, const char* who) {
    if (!h) return -1;
    if (!score || !annot) return -2;
    int rc = storm_host_begin(who);
    const uint64_t n = h->n_rows;
    const int no_lag = max_lag == 0 && !pos;   /* (with positions, max_lag 0 asks for the lag the windows need) */
    if (!rc && !no_lag && out_rows < n) rc = -4;
    if (!rc && no_lag) rc = storm_host_refuse(who, "max_lag must be at least 1 where no positions are given");
    if (!rc) rc = storm_dosage_ldscore_stat_refusal(who, stat, complete, h->n_samples);
    /* ---- the new checks */
    if (!rc && (n_annot < 1 || n_annot > STORM_LDSCORE_MAX_ANNOT))
        rc = storm_host_refuse(who, "n_annot = %llu: 1 .. %d annotation columns", (unsigned long long)n_annot, STORM_LDSCORE_MAX_ANNOT);
    if (!rc && (annot_ld < n_annot || score_ld < n_annot)) rc = -4;
    uint32_t* bounds = NULL;   /* lo, then hi: where positions are given */
    uint64_t lag = max_lag;
    if (!rc) rc = storm_dosage_band_windows(who, n, max_lag, pos, max_dist, 0, &bounds, &lag);
    if (!rc && !device) {
        for (uint64_t i = 0; i < n && !rc; ++i)
            for (uint64_t c = 0; c < n_annot; ++c)
                if (!isfinite(annot[i * annot_ld + c])) {
                    rc = storm_host_refuse(who, "annot[%llu][%llu] is not finite", (unsigned long long)i, (unsigned long long)c);
                    break;
                }
    }
    if (!rc && n >= 2) {
        storm_hip_ctx_t* ctx = NULL;
        const storm_hip_matrix_t* m = NULL;
        rc = storm_dosage_operands(h, NULL, &ctx, &m, NULL);
        if (!rc)
            rc = annot_run(ctx, m, stat, h->n_samples, lag, bounds, bounds ? bounds + n : NULL, annot, annot_ld, n_annot, score,
                           score_ld, n_pairs, complete, device);
    }
    free(bounds);
    return storm_host_end(rc);
}

int STORM_dosage_lag_ldscore_annot(STORM_dosage_t* h, int stat, uint64_t max_lag, const double* pos, double max_dist,
                                   const float* annot, uint64_t n_annot, uint64_t annot_ld, float* score, uint64_t score_ld,
                                   uint32_t* n_pairs, uint64_t out_rows) {
    return dosage_ldscore_annot(h, stat, max_lag, pos, max_dist, annot, n_annot, annot_ld, score, score_ld, n_pairs, out_rows, 0, 0,
                                "STORM_dosage_lag_ldscore_annot");
}
int STORM_dosage_lag_ldscore_annot_device(STORM_dosage_t* h, int stat, uint64_t max_lag, const double* pos, double max_dist,
                                          const float* d_annot, uint64_t n_annot, uint64_t annot_ld, float* d_score,
                                          uint64_t score_ld, uint32_t* d_n_pairs, uint64_t out_rows) {
    return dosage_ldscore_annot(h, stat, max_lag, pos, max_dist, d_annot, n_annot, annot_ld, d_score, score_ld, d_n_pairs, out_rows, 0,
                                1, "STORM_dosage_lag_ldscore_annot_device");
}
int STORM_dosage_lag_ldscore_annot_complete(STORM_dosage_t* h, int stat, uint64_t max_lag, const double* pos, double max_dist,
                                            const float* annot, uint64_t n_annot, uint64_t annot_ld, float* score, uint64_t score_ld,
                                            uint32_t* n_pairs, uint64_t out_rows) {
    return dosage_ldscore_annot(h, stat, max_lag, pos, max_dist, annot, n_annot, annot_ld, score, score_ld, n_pairs, out_rows, 1, 0,
                                "STORM_dosage_lag_ldscore_annot_complete");
}
int STORM_dosage_lag_ldscore_annot_complete_device(STORM_dosage_t* h, int stat, uint64_t max_lag, const double* pos, double max_dist,
                                                   const float* d_annot, uint64_t n_annot, uint64_t annot_ld, float* d_score,
                                                   uint64_t score_ld, uint32_t* d_n_pairs, uint64_t out_rows) {
    return dosage_ldscore_annot(h, stat, max_lag, pos, max_dist, d_annot, n_annot, annot_ld, d_score, score_ld, d_n_pairs, out_rows, 1,
                                1, "STORM_dosage_lag_ldscore_annot_complete_device");
}
