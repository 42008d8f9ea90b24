/* env_config.c — TEST ONLY: what the host side makes of STORM_HIP_DEVICES, STORM_HIP_SHARD and STORM_HIP_OPTIONS, on the
 * device stub under AddressSanitizer + UBSan (tests/test_host_pool_sanitize.py sets the variables and starts this program
 * once per case: they are read once per process). Prints the number of configured device slots and one contig total; on the
 * stub a total is the container's set bits on the process that holds shard 0 and 0 on every other. */
#include <stdio.h>

#include "storm.h"
#include "storm_synth.h"

int main(void) {
    int slots = 0;
    while (slots < 32 && STORM_hip_set_thread_devices(slots, 1) == 0) ++slots; /* -1 from the first slot outside the configuration */
    if (STORM_hip_set_thread_devices(0, 0) != 0) return 1;
    STORM_contiguous_t* c = STORM_contig_new(4096);
    if (!c) return 1;
    const int64_t bits = storm_synth_fill_contig(c, 4096, 0, 300, 700, 5);
    const uint64_t total = STORM_contig_pairw_intersect_cardinality(c);
    STORM_contig_free(c);
    STORM_hip_shutdown();
    printf("slots=%d total=%s\n", slots, total == (uint64_t)-1 ? "failed" : total == 0 ? "none" : "whole");
    return bits > 0 ? 0 : 1;
}
