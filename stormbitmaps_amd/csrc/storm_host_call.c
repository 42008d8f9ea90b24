/* storm_host_call.c — the frame of the container entry points of the per-pair calls (storm_host_internal.h): the lock and
 * the one-slot check around a call, the one way a refusal and a shim call's failure are reported, and what several calls
 * check or resolve alike. On storm_host.c's locked paths without adding to them. */
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"

int storm_host_begin(const char* who) {
    storm_host_lock();
    return who ? storm_host_one_slot_or_refuse(who) : 0;
}

int storm_host_end(int rc) {
    storm_host_unlock();
    return rc;
}

int storm_host_refuse(const char* who, const char* fmt, ...) {
    char msg[320];
    const int at = snprintf(msg, sizeof(msg), "%s: ", who);
    if (at > 0 && (size_t)at < sizeof(msg)) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg + at, sizeof(msg) - (size_t)at, fmt, ap);
        va_end(ap);
    }
    storm_host_error(msg);
    return -3;
}

int storm_host_shim_result(storm_hip_ctx_t* ctx, int rc, int wait, const char* name) {
    if (rc == STORM_HIP_OK && wait) rc = storm_hip_ctx_synchronize(ctx);
    if (rc != STORM_HIP_OK) {
        storm_host_device_error(name);
        return -3;
    }
    return 0;
}

int storm_host_ld_n_bits(const char* who, uint64_t* n_bits, uint64_t n_bits_default) {
    if (*n_bits == 0) *n_bits = n_bits_default;
    if (*n_bits == 0 || *n_bits > (1ull << 32))
        return storm_host_refuse(who, "the LD measures need n_bits, the size of the universe, in [1, 2^32]%s",
                                 n_bits_default ? "" : " (a STORM_t declares none: 0 is refused)");
    return 0;
}

int storm_host_contig_operand(STORM_contiguous_t* h, storm_hip_ctx_t** ctx, const storm_hip_matrix_t** m) {
    *m = storm_host_contig_matrix(h);
    *ctx = *m ? storm_host_ctx() : NULL;
    return *ctx ? 0 : -3;
}

int storm_host_dense_operand(STORM_t* h, storm_hip_ctx_t** ctx, const storm_hip_matrix_t** m) {
    *ctx = storm_host_ctx();
    /* the handle's state checked against the container as it is now; its dense replica, whatever else it keeps */
    sparse_state_t* st = *ctx ? storm_host_checked_state(h) : NULL;
    if (!st || (!st->have_dense && storm_host_build(h, st, 1, NULL, 0))) return -3;
    *m = st->m[storm_host_slot()];
    return 0;
}
