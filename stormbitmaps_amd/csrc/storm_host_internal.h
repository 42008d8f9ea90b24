/* storm_host_internal.h — what the host side of the storm.h containers shares between its files: the device state of a
 * STORM_t handle (storm_host.c), the helpers the rectangle of two containers (storm_square.c), the lag forms (storm_lag.c),
 * the top-k forms (storm_topk.c) and the dosage container (storm_dosage*.c) run on, and the frame of their entry points
 * (storm_host_call.c). Not installed. */
#ifndef STORM_HOST_INTERNAL_H_
#define STORM_HOST_INTERNAL_H_
#include <stdint.h>

#include "storm.h"
#include "storm_hip.h"

#define MAX_DEVICES 16

/* device state of a STORM_t handle, per configured GPU: a replica of the block arena (what the all-pairs totals run
 * on) and/or of the rows as a dense bit matrix (what STORM_pairw_matrix runs on); each is built by its first user */
typedef struct {
    storm_hip_sparse_t* a[MAX_DEVICES];
    storm_hip_matrix_t* m[MAX_DEVICES];
    storm_hip_rowlists_t* l[MAX_DEVICES]; /* [r5] a list-only container's rows as window-ordered positions (K5) */
    int have_arena, have_dense;
    int have_lists; /* 0 not tried, 1 built (on every slot of the view), -1 not eligible */
} sparse_state_t;

/* a dense replica builder with a minimum row width (storm_hip_matrix_create_from_blocks_wide) */
typedef int (*storm_dense_builder_t)(storm_hip_ctx_t* ctx, uint64_t n_rows, uint64_t n_blocks,
                                     const uint64_t* row_block_offset, const uint32_t* block_id, const uint8_t* block_kind,
                                     const uint32_t* block_n, const void* const* block_ptr, uint32_t min_blocks,
                                     storm_hip_matrix_t** out);

/* storm_host.c */
void storm_host_lock(void);   /* the calling thread's device slots */
void storm_host_unlock(void);
void storm_host_error(const char* msg);
void storm_host_device_error(const char* where);
int storm_host_one_slot_or_refuse(const char* who);  /* 0, or -5 with the reason */
int storm_host_single_device(void);                  /* 1: one device slot and one shard */
storm_hip_matrix_t* storm_host_contig_matrix(STORM_contiguous_t* h); /* its device mirror on that slot (NULL: reported) */
/* the operand of STORM_pairw_matrix_device's path choice: *from_lists ? st->l[slot] (K5) : st->m[slot]. 0 or -3 */
int storm_host_matrix_operand(STORM_t* h, sparse_state_t** st, int* from_lists);
int storm_host_slot(void);                           /* the calling thread's first device slot */
storm_hip_ctx_t* storm_host_ctx(void);               /* its context (NULL: no device, the reason reported) */
sparse_state_t* storm_host_checked_state(STORM_t* h);
/* storm_build_device: dense = 0 arena, 1 dense replica (`wide` with min_blocks, or NULL: own width), 2 row lists */
int storm_host_build(STORM_t* h, sparse_state_t* st, int dense, storm_dense_builder_t wide, uint32_t min_blocks);
void storm_host_drop_dense(sparse_state_t* st);
/* what a device copy kept in a handle is valid for: changes with the device configuration and the thread's view */
uint32_t storm_host_view_generation(void);
storm_hip_ctx_t* storm_host_open_ctx(int slot);      /* the context of `slot` if one is open (NULL: none; nothing is created) */

/* storm_square.c: the dense replicas of two containers at one common width (the wider of the two, or of a replica one of
 * them already keeps) on device slot `slot`; 0, or nonzero with the reason reported */
int storm_host_common_dense(STORM_t* a, sparse_state_t* sa, STORM_t* b, sparse_state_t* sb, int slot);

/* ---- storm_host_call.c: the frame of a container entry point. After its NULL checks (-1 handle, -2 output) an entry point
 * runs `int rc = storm_host_begin(who);`, its own checks and its shim call as `if (!rc) rc = ...;` lines in the order
 * storm.h documents, and `return storm_host_end(rc);`. */
int storm_host_begin(const char* who);   /* the lock, then the one-slot check (none for who NULL): 0, or -5 with the reason */
int storm_host_end(int rc);              /* the unlock, in either case; rc */
/* "<who>: <text>" into STORM_hip_error(); -3 */
int storm_host_refuse(const char* who, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
/* a shim call's return code `rc` as storm.h's: 0, or -3 reported under the shim call's `name`. `wait`: the work the call
 * queued on the context's stream is waited for first (a host form has waited itself; for a _device form see the callers) */
int storm_host_shim_result(storm_hip_ctx_t* ctx, int rc, int wait, const char* name);
/* the universe of the LD measures: n_bits 0 stands for `n_bits_default` (a STORM_contiguous_t's vector_length; 0 for a
 * STORM_t, which declares none). 0, or -3 where it is not in [1, 2^32] */
int storm_host_ld_n_bits(const char* who, uint64_t* n_bits, uint64_t n_bits_default);
/* the operand of a call on one container, on the calling thread's slot: a STORM_contiguous_t's device mirror, or a STORM_t's
 * dense replica (built when the handle has only its arena or its row lists). 0, or -3 with the reason reported */
int storm_host_contig_operand(STORM_contiguous_t* h, storm_hip_ctx_t** ctx, const storm_hip_matrix_t** m);
int storm_host_dense_operand(STORM_t* h, storm_hip_ctx_t** ctx, const storm_hip_matrix_t** m);

#endif /* STORM_HOST_INTERNAL_H_ */
