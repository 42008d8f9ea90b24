/* storm_dosage.c — the container of 2-bit dosage rows (storm.h: STORM_dosage_*): n_samples values 0 .. 3 per row, packed
 * 32 to a 64-bit word, and the per-pair dot products and genotype correlations (PLINK --r / --r2) of its rows.
 *
 * The host keeps the packed rows; they go up into an ordinary storm_hip_matrix_t on the first compute call after a change
 * (whole, from the row the device copy ends at: rows never change once added). On storm_host.c's locked paths without
 * adding to them, like storm_lag.c and storm_topk.c: one device slot and one process. No CPU fallback. Here too: what the
 * storm_dosage_*.c units beside it resolve and check alike (storm_dosage_internal.h). The per-pair matrices of one or two
 * containers are storm_dosage_pairs.c's. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"
#include "storm_dosage_internal.h"

#define DOSAGE_MAX_SAMPLES (1ull << 24)

STORM_dosage_t* STORM_dosage_new(uint64_t n_samples) {
    if (n_samples == 0 || n_samples > DOSAGE_MAX_SAMPLES) return NULL;
    STORM_dosage_t* h = (STORM_dosage_t*)calloc(1, sizeof(*h));
    if (!h) return NULL;
    h->n_samples = n_samples;
    h->n_words = (uint32_t)((n_samples + 31u) / 32u);
    return h;
}

/* (the caller holds the device lock) */
static void dosage_drop_device(STORM_dosage_t* h) {
    if (h->m) storm_hip_matrix_destroy(storm_host_open_ctx(h->slot), h->m);
    h->m = NULL;
    h->synced = 0;
}

void STORM_dosage_free(STORM_dosage_t* h) {
    if (!h) return;
    storm_host_lock();
    dosage_drop_device(h);
    storm_host_unlock();
    free(h->rows);
    free(h);
}

int STORM_dosage_clear(STORM_dosage_t* h) {
    if (!h) return -1;
    storm_host_lock();
    dosage_drop_device(h);
    storm_host_unlock();
    h->n_rows = 0;
    return 0;
}

uint64_t STORM_dosage_n_rows(const STORM_dosage_t* h) { return h ? h->n_rows : 0; }

/* room for `more` rows: 0, or -3 with the reason */
static int dosage_reserve(STORM_dosage_t* h, uint64_t more) {
    if (h->n_rows + more <= h->m_rows) return 0;
    uint64_t want = h->m_rows ? h->m_rows : 64;
    while (want < h->n_rows + more) want *= 2;
    if (want > SIZE_MAX / sizeof(uint64_t) / h->n_words)
        return storm_host_refuse("STORM_dosage_add", "the container would exceed the address space");
    uint64_t* p = (uint64_t*)realloc(h->rows, (size_t)want * h->n_words * sizeof(uint64_t));
    if (!p) return storm_host_refuse("STORM_dosage_add", "out of host memory");
    h->rows = p;
    h->m_rows = want;
    return 0;
}

int STORM_dosage_add(STORM_dosage_t* h, const uint8_t* values, uint64_t n_values) {
    if (!h) return -1;
    if (!values) return -2;
    if (n_values != h->n_samples)
        return storm_host_refuse("STORM_dosage_add", "%llu values for rows of %llu samples", (unsigned long long)n_values,
                                 (unsigned long long)h->n_samples);
    for (uint64_t s = 0; s < n_values; ++s)
        if (values[s] > 3)
            return storm_host_refuse("STORM_dosage_add", "value %u at sample %llu (a dosage is 0 .. 3)", (unsigned)values[s],
                                     (unsigned long long)s);
    if (dosage_reserve(h, 1)) return -3;
    uint64_t* row = h->rows + h->n_rows * h->n_words;
    for (uint32_t w = 0; w < h->n_words; ++w) {
        const uint64_t s0 = (uint64_t)w * 32u, s1 = s0 + 32u < n_values ? s0 + 32u : n_values;
        uint64_t word = 0;
        for (uint64_t s = s0; s < s1; ++s) word |= (uint64_t)values[s] << (2u * (s - s0));
        row[w] = word;
    }
    ++h->n_rows;
    return 0;
}

int STORM_dosage_add_packed(STORM_dosage_t* h, const uint64_t* words, uint64_t n_rows) {
    if (!h) return -1;
    if (!words) return -2;
    if (n_rows == 0) return 0;
    const uint32_t tail = (uint32_t)(h->n_samples % 32u); /* values in the last word (0: all 32) */
    if (tail)
        for (uint64_t r = 0; r < n_rows; ++r)
            if (words[r * h->n_words + h->n_words - 1u] >> (2u * tail))
                return storm_host_refuse("STORM_dosage_add_packed", "row %llu has bits beyond sample %llu", (unsigned long long)r,
                                         (unsigned long long)h->n_samples);
    if (n_rows > UINT64_MAX - h->n_rows) return storm_host_refuse("STORM_dosage_add_packed", "too many rows");
    if (dosage_reserve(h, n_rows)) return -3;
    memcpy(h->rows + h->n_rows * h->n_words, words, (size_t)n_rows * h->n_words * sizeof(uint64_t));
    h->n_rows += n_rows;
    return 0;
}

/* the device copy brought up to date on the calling thread's slot (the caller holds the lock): NULL with the reason reported */
static storm_hip_matrix_t* storm_dosage_mirror(STORM_dosage_t* h, storm_hip_ctx_t** ctx_out) {
    const uint32_t generation = storm_host_view_generation();
    if (h->m && (h->generation != generation || h->slot != storm_host_slot() || h->synced > h->n_rows)) dosage_drop_device(h);
    storm_hip_ctx_t* ctx = storm_host_ctx();
    if (!ctx) return NULL;
    if (!h->m) {
        if (storm_hip_matrix_create(ctx, h->n_rows, h->n_words, &h->m) != STORM_HIP_OK) {
            storm_host_device_error("storm_hip_matrix_create");
            h->m = NULL;
            return NULL;
        }
        h->slot = storm_host_slot();
        h->generation = generation;
        h->synced = 0;
    }
    if (h->synced != h->n_rows) {
        if (storm_hip_matrix_resize(ctx, h->m, h->n_rows) != STORM_HIP_OK ||
            storm_hip_matrix_upload(ctx, h->m, h->synced, h->n_rows - h->synced, h->rows + h->synced * h->n_words, h->n_words) !=
                STORM_HIP_OK) {
            storm_host_device_error("dosage upload");
            dosage_drop_device(h);
            return NULL;
        }
        h->synced = h->n_rows;
    }
    *ctx_out = ctx;
    return h->m;
}

int storm_dosage_operands(STORM_dosage_t* a, STORM_dosage_t* b, storm_hip_ctx_t** ctx, const storm_hip_matrix_t** ma,
                          const storm_hip_matrix_t** mb) {
    storm_hip_ctx_t* ctx_b = NULL;
    if (!(*ma = storm_dosage_mirror(a, ctx))) return -3;
    if (mb && !(*mb = b && b != a ? storm_dosage_mirror(b, &ctx_b) : *ma)) return -3;
    return 0;
}

int storm_dosage_measure_refusal(const char* who, int measure) {
    if (measure == STORM_DOSAGE_R2 || measure == STORM_DOSAGE_R) return 0;
    return storm_host_refuse(who, "measure must be 0 (STORM_DOSAGE_R2) or 1 (STORM_DOSAGE_R)");
}

int storm_dosage_samples_refusal(const char* who, const STORM_dosage_t* a, const STORM_dosage_t* b) {
    if (a->n_samples == b->n_samples) return 0;
    return storm_host_refuse(who, "containers of %llu and of %llu samples", (unsigned long long)a->n_samples,
                             (unsigned long long)b->n_samples);
}

/* a count per row: the sums and sums of squares, or (`missing`: into `sum`) the numbers of 3s */
static int dosage_rows(STORM_dosage_t* h, uint32_t* sum, uint32_t* sum_sq, int missing, const char* who) {
    int rc = storm_host_begin(who);
    if (!rc && h->n_rows != 0) {
        storm_hip_ctx_t* ctx = NULL;
        const storm_hip_matrix_t* m = NULL;
        rc = storm_dosage_operands(h, NULL, &ctx, &m, NULL);
        if (!rc)
            rc = storm_host_shim_result(ctx, missing ? storm_hip_dosage_row_missing(ctx, m, h->n_samples, sum)
                                                     : storm_hip_dosage_row_sums(ctx, m, sum, sum_sq),
                                        0, missing ? "storm_hip_dosage_row_missing" : "storm_hip_dosage_row_sums");
    }
    return storm_host_end(rc);
}

int STORM_dosage_row_sums(STORM_dosage_t* h, uint32_t* sum, uint32_t* sum_sq) {
    if (!h) return -1;
    if (!sum || !sum_sq) return -2;
    return dosage_rows(h, sum, sum_sq, 0, "STORM_dosage_row_sums");
}

/* (the value 3 means "missing" there and only there, as in the _nobs and _complete calls) */
int STORM_dosage_row_missing(STORM_dosage_t* h, uint32_t* missing) {
    if (!h) return -1;
    if (!missing) return -2;
    return dosage_rows(h, missing, NULL, 1, "STORM_dosage_row_missing");
}
