/* storm_dosage_internal.h — the dosage container as storm_dosage.c and the storm_dosage_*.c units beside it share it. */
#pragma once
#include <stdint.h>

#include "storm.h"
#include "storm_hip.h"

struct STORM_dosage_s {
    uint64_t n_samples;
    uint32_t n_words;    /* ceil(n_samples / 32) */
    uint64_t n_rows, m_rows;
    uint64_t* rows;      /* n_rows x n_words, packed */
    /* the device copy: rows [0, synced) of `m` on device slot `slot`, made under view generation `generation` */
    storm_hip_matrix_t* m;
    int slot;
    uint32_t generation;
    uint64_t synced;
};

/* ---- storm_dosage.c: what the storm_dosage_*.c units resolve and check alike. Each returns 0, or -3 with the reason
 * reported; the caller holds the lock. ---- */

/* the device copies of one container or two brought up to date on the calling thread's slot: *ctx, *ma and, where mb is
 * given, *mb (b NULL or the same container as a: *mb = *ma) */
int storm_dosage_operands(STORM_dosage_t* a, STORM_dosage_t* b, storm_hip_ctx_t** ctx, const storm_hip_matrix_t** ma,
                          const storm_hip_matrix_t** mb);
/* measure is neither STORM_DOSAGE_R2 nor STORM_DOSAGE_R */
int storm_dosage_measure_refusal(const char* who, int measure);
/* two containers whose rows have different numbers of samples */
int storm_dosage_samples_refusal(const char* who, const STORM_dosage_t* a, const STORM_dosage_t* b);

/* ---- storm_dosage_band.c: shared by the calls on the band of r^2. Each returns 0, or -3 with the reason reported; the
 * caller holds the lock. ---- */

/* a band call's return code `rc` as storm.h's (storm_host_shim_result), a _device form waited for */
int storm_dosage_band_result(storm_hip_ctx_t* ctx, int rc, int device, const char* name);

/* stat is neither STORM_LDSCORE_R2 nor _R2_ADJ, or the complete-case adjusted statistic has fewer than 3 samples */
int storm_dosage_ldscore_stat_refusal(const char* who, int stat, int complete, uint64_t n_samples);

/* (max_lag, pos, max_dist) into the lag to ask the device for and the rows' windows. *plan: NULL, or malloc'd n x (2 +
 * extra_words_per_row) words for the caller to free in every case: lo, then hi (filled where pos is given), then the
 * caller's own. It is allocated where there are rows and positions or extra words. *lag: max_lag, or with max_lag 0 what
 * the windows need. Refused: no memory, positions or max_dist the planner refuses, windows wider than a max_lag > 0. */
int storm_dosage_band_windows(const char* who, uint64_t n, uint64_t max_lag, const double* pos, double max_dist,
                              unsigned extra_words_per_row, uint32_t** plan, uint64_t* lag);
