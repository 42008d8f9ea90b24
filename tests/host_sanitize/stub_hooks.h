/* stub_hooks.h — TEST ONLY. What device_stub.c lets a driver see and provoke: which thread launched each shard of a pass
 * (the host's worker pool drives device slots 1 .. n - 1 from threads of its own), and one launch that fails, as a
 * return code on the CPU. Never linked into the product. */
#pragma once
#include <stdint.h>

#define STUB_DRIVER_CALLER 1 /* launched by the thread that called stub_hook_caller() */
#define STUB_DRIVER_OTHER 2  /* launched by another thread */

/* the calling thread is "the caller" from now on; forgets every launch noted so far */
void stub_hook_caller(void);
/* who has launched shard `shard_rank` of a dense or STORM_t pass since: 0 nobody, else STUB_DRIVER_* OR-ed */
int stub_hook_driver(uint32_t shard_rank);
/* products of STORM_wrapper_square run by a thread other than the caller since */
int stub_hook_square_foreign(void);
/* the next launch of shard `shard_rank` fails (once) with "stub: injected launch failure"; -1 takes it back */
void stub_hook_fail_launch(int shard_rank);
