/* storm_square.c — the rectangle of two STORM_t (storm.h: STORM_intersect_cardinality_square, STORM_square_matrix,
 * STORM_square_matrix_device). The reference declares the first (storm.h:231) and never defines it (storm.c:975).
 *
 * Both handles keep their device copies exactly as for STORM_pairw_matrix (storm_host.c: state, fingerprint / epoch /
 * block stamps, one build per kind, all under the calling thread's device lock). Two list-only containers that the K5
 * rule (option matrix_lists, applied to the two together) sends to the lists are joined from their row lists (K5x,
 * storm_hip_lists.hip); any other pair is multiplied as dense replicas of one common width (the wider of the two; a
 * handle keeps its widened replica, whose extra zero columns change no count of its own triangle). One device slot and
 * one process: the rectangle is not split over devices or shards, and every rank refuses alike.
 *
 * Also here, because they too sit on storm_host.c's locked paths without adding to them: the similarity forms of all three
 * per-pair matrices (storm.h: STORM_contig_pairw_similarity, STORM_pairw_similarity, STORM_square_similarity and _device). */
#include <stdint.h>
#include <stdlib.h>

#include "storm.h"
#include "storm_hip.h"
#include "storm_host_internal.h"

#define BLOCK_WORDS ((uint32_t)STORM_DEFAULT_BLOCK_SIZE / 64u)

/* listed positions and the width in bits of a list-only container (0: it holds a bitmap block) */
static int list_counts(const STORM_t* h, uint64_t* n_elems, uint64_t* n_bits) {
    uint64_t e = 0, max_id = 0;
    for (uint32_t i = 0; i < h->n_conts; ++i)
        for (uint32_t b = 0; b < h->conts[i].n_bitmaps; ++b) {
            const STORM_bitmap_t* blk = &h->conts[i].bitmaps[b];
            if (blk->n_bitmap) return 0;
            e += blk->n_scalar;
            if (blk->n_scalar && blk->id > max_id) max_id = blk->id;
        }
    *n_elems = e;
    *n_bits = (max_id + 1) * 65536ull;
    return 1;
}

/* blocks per row of a container's own dense replica (storm_hip_matrix_create_from_blocks: largest block id + 1) */
static uint32_t dense_blocks(const STORM_t* h) {
    uint32_t max_id = 0;
    for (uint32_t i = 0; i < h->n_conts; ++i)
        for (uint32_t b = 0; b < h->conts[i].n_bitmaps; ++b)
            if (h->conts[i].bitmaps[b].id > max_id) max_id = h->conts[i].bitmaps[b].id;
    return max_id + 1u;
}

static uint32_t replica_blocks(const sparse_state_t* st, int slot) {
    return st->have_dense ? storm_hip_matrix_words(st->m[slot]) / BLOCK_WORDS : 0u;
}

/* the dense replica of `h` at least `blocks` wide: a narrower one is rebuilt, a wider one kept */
static int dense_at_width(STORM_t* h, sparse_state_t* st, int slot, uint32_t blocks) {
    if (st->have_dense && replica_blocks(st, slot) >= blocks) return 0;
    storm_host_drop_dense(st);
    return storm_host_build(h, st, 1, storm_hip_matrix_create_from_blocks_wide, blocks);
}

/* dense replicas of one common width: the wider of the two containers, or of a replica one of them already keeps
 * (storm_host_internal.h: the top-k rectangle of storm_topk.c runs on them too). 0, or nonzero with the reason reported. */
int storm_host_common_dense(STORM_t* a, sparse_state_t* sa, STORM_t* b, sparse_state_t* sb, int slot) {
    uint32_t blocks = dense_blocks(a), x = dense_blocks(b);
    if (x > blocks) blocks = x;
    if ((x = replica_blocks(sa, slot)) > blocks) blocks = x;
    if ((x = replica_blocks(sb, slot)) > blocks) blocks = x;
    return dense_at_width(a, sa, slot, blocks) || (b != a && dense_at_width(b, sb, slot, blocks));
}

/* what = 0: *total; 1: the window into host `out`; 2: into device `out`. measure < 0: counts under `op`; else the window
 * finished into that similarity measure (float entries in `out`, universe n_bits). 0, or -3 with the reason in
 * STORM_hip_error(). */
static int square_locked(STORM_t* a, STORM_t* b, int what, int op, uint32_t* out, uint64_t out_ld, uint64_t* total,
                         int measure, uint64_t n_bits) {
    if (!storm_host_single_device()) {
        storm_host_error("STORM_intersect_cardinality_square / STORM_square_matrix / STORM_square_similarity: the rectangle of two containers is "
                         "computed on ONE device slot by ONE process; it is not split over devices or shards "
                         "(STORM_hip_set_devices, STORM_hip_set_thread_devices, STORM_hip_set_shard)");
        return -3;
    }
    storm_hip_ctx_t* ctx = storm_host_ctx();
    if (!ctx) return -3;
    const int slot = storm_host_slot();
    sparse_state_t* sa = storm_host_checked_state(a);
    sparse_state_t* sb = sa && b != a ? storm_host_checked_state(b) : sa;
    if (!sa || !sb) return -3;
    /* [K5x] both list-only, and the K5 rule sends the two together to the lists */
    uint64_t ea = 0, eb = 0, wa = 0, wb = 0;
    if (storm_hip_rowlists_worthwhile(ctx, NULL) && sa->have_lists != -1 && sb->have_lists != -1 &&
        list_counts(a, &ea, &wa) && list_counts(b, &eb, &wb) &&
        storm_hip_rowlists_worthwhile_counts(ctx, (uint64_t)a->n_conts + b->n_conts, ea + eb, wa > wb ? wa : wb)) {
        if (sa->have_lists == 0 && storm_host_build(a, sa, 2, NULL, 0)) return -3;
        if (sb->have_lists == 0 && storm_host_build(b, sb, 2, NULL, 0)) return -3;
        if (sa->have_lists == 1 && sb->have_lists == 1) {
            storm_hip_rowlists_t* la = sa->l[slot];
            const storm_hip_rowlists_t* lb = sb->l[slot];
            const int rc = what == 0    ? storm_hip_rowlists_square_total(ctx, la, lb, total)
                           : measure >= 0 ? (what == 1 ? storm_hip_rowlists_square_similarity(ctx, la, lb, measure, n_bits, (float*)out, out_ld)
                                                       : storm_hip_rowlists_square_similarity_device(ctx, la, lb, measure, n_bits, (float*)out, out_ld))
                           : what == 1  ? storm_hip_rowlists_square_matrix(ctx, la, lb, op, out, out_ld)
                                        : storm_hip_rowlists_square_matrix_device(ctx, la, lb, op, out, out_ld);
            return storm_host_shim_result(ctx, rc, 0, "storm_hip_rowlists_square");
        }
    }
    if (storm_host_common_dense(a, sa, b, sb, slot)) return -3;
    const int rc = what == 0    ? storm_hip_cross_dense_total(ctx, sa->m[slot], sb->m[slot], total)
                   : measure >= 0 ? (what == 1 ? storm_hip_cross_dense_similarity(ctx, sa->m[slot], sb->m[slot], measure, n_bits, (float*)out, out_ld)
                                               : storm_hip_cross_dense_similarity_device(ctx, sa->m[slot], sb->m[slot], measure, n_bits, (float*)out, out_ld))
                   : what == 1  ? storm_hip_cross_dense_matrix(ctx, sa->m[slot], sb->m[slot], op, out, out_ld)
                                : storm_hip_cross_dense_matrix_device(ctx, sa->m[slot], sb->m[slot], op, out, out_ld);
    return storm_host_shim_result(ctx, rc, 0, "storm_hip_cross_dense");
}

uint64_t STORM_intersect_cardinality_square(const STORM_t* STORM_RESTRICT bitmap1, const STORM_t* STORM_RESTRICT bitmap2) {
    if (!bitmap1 || !bitmap2) {
        storm_host_error("STORM_intersect_cardinality_square: NULL handle");
        return (uint64_t)-1;
    }
    if (bitmap1->n_conts == 0 || bitmap2->n_conts == 0) return 0;
    uint64_t total = 0;
    storm_host_begin(NULL);   /* (no one-slot check of the frame's: square_locked refuses several slots or shards in its own words) */
    /* (the containers are const; the device copies behind them are built and kept as for every other call) */
    const int rc = storm_host_end(square_locked((STORM_t*)bitmap1, (STORM_t*)bitmap2, 0, 0, NULL, 0, &total, -1, 0));
    return rc ? (uint64_t)-1 : total;
}

int STORM_square_matrix(STORM_t* a, STORM_t* b, int op, uint32_t* out, uint64_t out_rows, uint64_t out_ld) {
    if (!a || !b) return -1;
    if (!out) return -2;
    if (out_rows < a->n_conts || out_ld < b->n_conts) return -4;
    if (op < 0 || op > 2) return storm_host_refuse("STORM_square_matrix", "op must be 0 (and), 1 (or) or 2 (xor)");
    if (a->n_conts == 0 || b->n_conts == 0) return 0;
    storm_host_begin(NULL);   /* (as above) */
    return storm_host_end(square_locked(a, b, 1, op, out, out_ld, NULL, -1, 0));
}

int STORM_square_matrix_device(STORM_t* a, STORM_t* b, int op, uint32_t* d_out, uint64_t out_rows, uint64_t out_ld) {
    if (!a || !b) return -1;
    if (!d_out) return -2;
    int rc = storm_host_begin("STORM_square_matrix_device");
    if (!rc && (out_rows < a->n_conts || out_ld < b->n_conts)) rc = -4;
    if (!rc && (op < 0 || op > 2)) rc = storm_host_refuse("STORM_square_matrix_device", "op must be 0 (and), 1 (or) or 2 (xor)");
    if (!rc && a->n_conts != 0 && b->n_conts != 0) rc = square_locked(a, b, 2, op, d_out, out_ld, NULL, -1, 0);
    return storm_host_end(rc);
}


/* ---- Extension (storm.h): the per-pair matrices finished into a similarity statistic on the device — the AND-count path of
 * the matrix calls as it is (same kernels, same choice), the rows' counts, then finish_tiles_kernel<SimilarityStat>
 * (storm_hip_similarity.hip) behind the count kernel. One device slot and one process, host forms too. */
/* The measure and the universe size as the shim takes them: 0, or -3 with the reason. Jaccard and cosine do not read n_bits;
 * the LD measures take `n_bits_default` (a STORM_contiguous_t's vector_length; 0 for a STORM_t, which declares none) for 0. */
static int similarity_args(const char* who, int measure, uint64_t* n_bits, uint64_t n_bits_default) {
    if (measure < STORM_SIM_JACCARD || measure > STORM_SIM_LD_R2)
        return storm_host_refuse(who, "measure must be 0 (Jaccard), 1 (cosine), 2 (LD D) or 3 (LD r^2)");
    if (measure < STORM_SIM_LD_D) {
        *n_bits = 1;
        return 0;
    }
    return storm_host_ld_n_bits(who, n_bits, n_bits_default);
}

static int contig_pairw_similarity(STORM_contiguous_t* h, int measure, uint64_t n_bits, float* out, uint64_t out_rows,
                                   uint64_t out_ld, int device, const char* who) {
    if (!h) return -1;
    if (!out) return -2;
    int rc = storm_host_begin(who);
    const uint64_t n = h->n_data;
    if (!rc && (out_rows < n || out_ld < n)) rc = -4;
    if (!rc) rc = similarity_args(who, measure, &n_bits, h->vector_length);
    if (!rc && n != 0) {
        storm_hip_ctx_t* ctx = NULL;
        const storm_hip_matrix_t* m = NULL;
        rc = storm_host_contig_operand(h, &ctx, &m);
        if (!rc)
            rc = storm_host_shim_result(ctx, device ? storm_hip_pairw_similarity_device(ctx, m, measure, n_bits, out, out_ld)
                                                    : storm_hip_pairw_similarity(ctx, m, measure, n_bits, out, out_ld),
                                        0, "storm_hip_pairw_similarity");
    }
    return storm_host_end(rc);
}

int STORM_contig_pairw_similarity(STORM_contiguous_t* h, int measure, uint64_t n_bits, float* out, uint64_t out_rows,
                                  uint64_t out_ld) {
    return contig_pairw_similarity(h, measure, n_bits, out, out_rows, out_ld, 0, "STORM_contig_pairw_similarity");
}

int STORM_contig_pairw_similarity_device(STORM_contiguous_t* h, int measure, uint64_t n_bits, float* d_out, uint64_t out_rows,
                                         uint64_t out_ld) {
    return contig_pairw_similarity(h, measure, n_bits, d_out, out_rows, out_ld, 1, "STORM_contig_pairw_similarity_device");
}

/* (the operand by the path choice of STORM_pairw_matrix_device: the row lists or the dense replica) */
static int storm_pairw_similarity(STORM_t* h, int measure, uint64_t n_bits, float* out, uint64_t out_rows, uint64_t out_ld,
                                  int device, const char* who) {
    if (!h) return -1;
    if (!out) return -2;
    int rc = storm_host_begin(who);
    const uint64_t n = h->n_conts;
    if (!rc && (out_rows < n || out_ld < n)) rc = -4;
    if (!rc) rc = similarity_args(who, measure, &n_bits, 0);
    if (!rc && n != 0) {
        sparse_state_t* st = NULL;
        int from_lists = 0;
        rc = storm_host_matrix_operand(h, &st, &from_lists);
        storm_hip_ctx_t* ctx = rc ? NULL : storm_host_ctx();
        const int slot = storm_host_slot();
        if (!rc && !ctx) rc = -3;
        if (!rc && from_lists)
            rc = storm_host_shim_result(
                ctx, device ? storm_hip_rowlists_pairw_similarity_device(ctx, st->l[slot], measure, n_bits, out, out_ld)
                            : storm_hip_rowlists_pairw_similarity(ctx, st->l[slot], measure, n_bits, out, out_ld),
                0, "storm_hip_rowlists_pairw_similarity");
        else if (!rc)
            rc = storm_host_shim_result(ctx, device ? storm_hip_pairw_similarity_device(ctx, st->m[slot], measure, n_bits, out, out_ld)
                                                    : storm_hip_pairw_similarity(ctx, st->m[slot], measure, n_bits, out, out_ld),
                                        0, "storm_hip_pairw_similarity");
    }
    return storm_host_end(rc);
}

int STORM_pairw_similarity(STORM_t* h, int measure, uint64_t n_bits, float* out, uint64_t out_rows, uint64_t out_ld) {
    return storm_pairw_similarity(h, measure, n_bits, out, out_rows, out_ld, 0, "STORM_pairw_similarity");
}

int STORM_pairw_similarity_device(STORM_t* h, int measure, uint64_t n_bits, float* d_out, uint64_t out_rows, uint64_t out_ld) {
    return storm_pairw_similarity(h, measure, n_bits, d_out, out_rows, out_ld, 1, "STORM_pairw_similarity_device");
}

/* the rectangle: what = 1 host, 2 device */
static int square_similarity(STORM_t* a, STORM_t* b, int measure, uint64_t n_bits, float* out, uint64_t out_rows, uint64_t out_ld,
                             int what, const char* who) {
    if (!a || !b) return -1;
    if (!out) return -2;
    int rc = storm_host_begin(who);
    if (!rc && (out_rows < a->n_conts || out_ld < b->n_conts)) rc = -4;
    if (!rc) rc = similarity_args(who, measure, &n_bits, 0);
    if (!rc && a->n_conts != 0 && b->n_conts != 0) rc = square_locked(a, b, what, 0, (uint32_t*)out, out_ld, NULL, measure, n_bits);
    return storm_host_end(rc);
}

int STORM_square_similarity(STORM_t* a, STORM_t* b, int measure, uint64_t n_bits, float* out, uint64_t out_rows,
                            uint64_t out_ld) {
    return square_similarity(a, b, measure, n_bits, out, out_rows, out_ld, 1, "STORM_square_similarity");
}

int STORM_square_similarity_device(STORM_t* a, STORM_t* b, int measure, uint64_t n_bits, float* d_out, uint64_t out_rows,
                                   uint64_t out_ld) {
    return square_similarity(a, b, measure, n_bits, d_out, out_rows, out_ld, 2, "STORM_square_similarity_device");
}
