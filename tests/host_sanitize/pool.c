/* pool.c — TEST ONLY: the worker pool of storm_host.c (pool_main / run_on_devices: one thread per device slot beyond the
 * first) on the device stub, under ThreadSanitizer (tests/test_host_pool_sanitize.py). The same ordinal listed three times
 * keeps the pool off by default, so STORM_HIP_HOST_THREADS decides: argv[1] = "1" forces the pool, "0" keeps every slot on
 * the caller's thread. The variable is read per call but a process is started per mode, as a job would be.
 *   - three slots, twenty generations of the contig, STORM_t, STORM_wrapper_square and serialized totals: each equals what
 *     ONE slot gives at the end of the same run;
 *   - who launched each shard (stub_hooks.h): slots 1 and 2 by other threads with the pool, by the caller without;
 *   - one launch fails (a return code from the stub): the call fails, stderr names the slot, the NEXT call is right again;
 *   - three slots -> two -> three: the worker of slot 2 launches nothing while two are configured. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "storm.h"
#include "storm_synth.h"
#include "stub_hooks.h"

#define FAILED ((uint64_t)-1)
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            fprintf(stderr, "POOL CHECK line %d: ", __LINE__);  \
            fprintf(stderr, __VA_ARGS__);                       \
            fprintf(stderr, "\n");                              \
            exit(1);                                            \
        }                                                       \
    } while (0)

enum { N1 = 130, N2 = 70, W = 16 };
static STORM_contiguous_t* g_c;
static STORM_t* g_s;
static uint64_t *g_a, *g_b;
static void* g_ser;
static uint64_t g_ser_bytes;
static int g_pool; /* 1: the pool is forced on */

enum { CONTIG, STORM, SQUARE, SERIAL, N_CALLS };
static const char* const g_name[N_CALLS] = {"contig", "STORM_t", "wrapper_square", "serialized"};
static uint64_t call(int which) {
    switch (which) {
        case CONTIG: return STORM_contig_pairw_intersect_cardinality(g_c);
        case STORM: return STORM_pairw_intersect_cardinality(g_s);
        case SQUARE: return STORM_wrapper_square(N1, g_a, N2, g_b, W, NULL);
        default: return STORM_serialized_pairw_intersect_cardinality(g_ser, g_ser_bytes);
    }
}

/* one call over `n_slots` configured slots, and who launched what during it */
static uint64_t call_and_check_drivers(int which, int n_slots) {
    stub_hook_caller();
    const uint64_t t = call(which);
    const int others = g_pool && n_slots > 1 ? STUB_DRIVER_OTHER : STUB_DRIVER_CALLER;
    if (which == CONTIG || which == STORM) {
        CHECK(stub_hook_driver(0) == STUB_DRIVER_CALLER, "%s: slot 0 driven by %d", g_name[which], stub_hook_driver(0));
        for (int d = 1; d < 3; ++d)
            CHECK(stub_hook_driver((uint32_t)d) == (d < n_slots ? others : 0), "%s over %d slots: slot %d driven by %d, expected %d",
                  g_name[which], n_slots, d, stub_hook_driver((uint32_t)d), d < n_slots ? others : 0);
    } else if (which == SQUARE) {
        CHECK(stub_hook_square_foreign() == (g_pool ? n_slots - 1 : 0), "wrapper_square over %d slots: %d products on other threads",
              n_slots, stub_hook_square_foreign());
    } else { /* the serialized form launches every slot from the caller's thread, pool or not */
        for (int d = 0; d < n_slots; ++d)
            CHECK(stub_hook_driver((uint32_t)d) == STUB_DRIVER_CALLER, "serialized: slot %d driven by %d", d, stub_hook_driver((uint32_t)d));
    }
    return t;
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "1";
    g_pool = mode[0] == '1';
    setenv("STORM_HIP_HOST_THREADS", mode, 1);
    const int ids[3] = {0, 0, 0}; /* (on the stub every slot is its own device) */
    CHECK(STORM_hip_set_devices(3, ids) == 0, "set_devices(3)");

    g_c = STORM_contig_new(4096);
    g_s = STORM_new();
    g_a = (uint64_t*)calloc((size_t)N1 * W, sizeof(uint64_t));
    g_b = (uint64_t*)calloc((size_t)N2 * W, sizeof(uint64_t));
    CHECK(g_c && g_s && g_a && g_b, "allocation");
    storm_synth_fill_contig(g_c, 4096, 0, 600, 900, 3);
    storm_synth_fill_storm(g_s, 3 * 65536, 0, 400, 40, 4);
    storm_synth_fill_dense(g_a, W, W * 64, 0, N1, 200, 5);
    storm_synth_fill_dense(g_b, W, W * 64, 0, N2, 200, 6);
    g_ser_bytes = STORM_serialized_size(g_s);
    g_ser = malloc(g_ser_bytes);
    CHECK(g_ser && STORM_serialize(g_s, g_ser, g_ser_bytes) == g_ser_bytes, "serialize");

    /* twenty generations over three slots */
    uint64_t three[N_CALLS] = {0};
    for (int gen = 0; gen < 20; ++gen)
        for (int w = 0; w < N_CALLS; ++w) {
            const uint64_t t = call_and_check_drivers(w, 3);
            CHECK(t != FAILED && t != 0, "%s failed in generation %d: %s", g_name[w], gen, STORM_hip_error());
            CHECK(gen == 0 || t == three[w], "%s: generation %d gave %llu, generation 0 %llu", g_name[w], gen,
                  (unsigned long long)t, (unsigned long long)three[w]);
            three[w] = t;
        }

    /* one launch fails: on a worker's slot, then on the caller's. The call fails, the next one is right again (the pool's
     * pending count and generation are not left wedged: a wedged pool would hang or fail here). */
    for (int w = CONTIG; w <= STORM; ++w)
        for (int slot = 2; slot >= 0; slot -= 2) {
            stub_hook_fail_launch(slot);
            fprintf(stderr, "-- injected: %s, slot %d\n", g_name[w], slot);
            CHECK(call(w) == FAILED, "%s: the failed launch on slot %d went unnoticed", g_name[w], slot);
            CHECK(strstr(STORM_hip_error(), "injected") != NULL, "%s: STORM_hip_error() is \"%s\"", g_name[w], STORM_hip_error());
            const uint64_t t = call_and_check_drivers(w, 3);
            CHECK(t == three[w], "%s after a failed launch on slot %d: %llu, expected %llu", g_name[w], slot,
                  (unsigned long long)t, (unsigned long long)three[w]);
        }

    /* three slots -> two -> three: slot 2's worker stays parked while two are configured */
    for (int round = 0; round < 3; ++round) {
        CHECK(STORM_hip_set_devices(2, ids) == 0, "set_devices(2)");
        for (int w = 0; w < N_CALLS; ++w) {
            const uint64_t t = call_and_check_drivers(w, 2);
            CHECK(t == three[w], "%s over two slots: %llu, expected %llu", g_name[w], (unsigned long long)t, (unsigned long long)three[w]);
        }
        CHECK(STORM_hip_set_devices(3, ids) == 0, "set_devices(3) again");
        for (int w = 0; w < N_CALLS; ++w) {
            const uint64_t t = call_and_check_drivers(w, 3);
            CHECK(t == three[w], "%s over three slots again: %llu, expected %llu", g_name[w], (unsigned long long)t, (unsigned long long)three[w]);
        }
    }

    /* what one slot gives */
    CHECK(STORM_hip_set_devices(1, ids) == 0, "set_devices(1)");
    for (int w = 0; w < N_CALLS; ++w) {
        const uint64_t t = call_and_check_drivers(w, 1);
        CHECK(t == three[w], "%s: one slot gives %llu, three gave %llu", g_name[w], (unsigned long long)t, (unsigned long long)three[w]);
    }

    STORM_contig_free(g_c);
    STORM_free(g_s);
    free(g_a);
    free(g_b);
    free(g_ser);
    STORM_hip_shutdown();
    printf("pool ok (host threads %s)\n", g_pool ? "on" : "off");
    return 0;
}
