/* storm_dosage_internal.h — the dosage container as storm_dosage.c and storm_dosage_complete.c share it. */
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

/* the device copy brought up to date on the calling thread's slot (the caller holds the lock): NULL with the reason reported */
storm_hip_matrix_t* storm_dosage_mirror(STORM_dosage_t* h, storm_hip_ctx_t** ctx_out);
