"""Round-6 GPU parity tests. Everything goes through the C-ABI; the oracle is the checker only."""
import numpy as np
import pytest

import stormbitmaps_amd as sb
from stormbitmaps_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip_ctx():
    ctx = sb.HipContext(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def orc():
    from tests._orc import Oracle
    return Oracle()


def _reset_tiles(ctx):
    for k, v in (("k2_tile_shape", 0), ("k2_wave_below", 400), ("k2_part_slots", 0), ("k2_part_min_chunks", 8),
                 ("k2_part_cost_diag", 80)):
        ctx.set_option(k, v)


WAVE_SHAPES = ((4096, 256, 2048), (640, 65, 200), (1000, 257, 300), (9000, 700, 3000), (300, 130, 100), (512, 300, 100),
               (520, 31, 100), (70000, 1029, 20000), (1536, 1301, 500), (64, 97, 20), (131072 + 64, 190, 40000))


def test_tile128_kernel_against_the_oracle(hip_ctx, orc):
    """tile128_kernel (K2h, k2_tile_shape = 6: 128 x 128 tiles, rows staged through the LDS, k-parts whose sums meet inside
    the launch — windows in register layout, a ticket per tile, the last part adds and writes) against the oracle's per-pair
    counts (storm.c:1199-1238 with the leaf's result kept per pair): triangle, AND / OR / XOR, rows of zero, ragged last
    tiles (1 .. 127 rows beyond a multiple of 128), row lengths that are not whole 512-bit chunks or whole trips of four
    chunks, one chunk, one tile; with whole tiles, with one and two segments per CU and with parts down to one chunk."""
    try:
        hip_ctx.set_option("k2_tile_shape", 6)
        for M, N, d in WAVE_SHAPES:
            mat = synth.dense_matrix_c(M, N, d, seed=N + M)
            mat[N // 3] = 0
            m = hip_ctx.matrix_from_host(mat)
            want = {"and": np.triu(orc.tile_counts(mat, 0, N, 0, N), k=1).astype(np.uint32)}
            rc = m.row_counts().astype(np.uint32)
            s = rc[:, None] + rc[None, :]
            want["or"] = np.triu(s - want["and"], k=1)
            want["xor"] = np.triu(s - 2 * want["and"], k=1)
            for slots, min_chunks in ((0, 8), (1, 1), (2, 1), (2, 3)):
                hip_ctx.set_option("k2_part_slots", slots)
                hip_ctx.set_option("k2_part_min_chunks", min_chunks)
                for op in ("and", "or", "xor"):
                    for rep in range(2):   # (again: the tickets of the call before must have been left at zero)
                        got = m.pairw_matrix(op)
                        assert hip_ctx.get_option("k2_tile_shape_used") == 6
                        assert np.array_equal(want[op], got), (M, N, slots, min_chunks, op, rep,
                                                               np.argwhere(want[op] != got)[:3].tolist())
            m.close()
    finally:
        _reset_tiles(hip_ctx)


def test_tile128_kernel_bands_rectangles_and_the_automatic_rule(hip_ctx, orc):
    """K2h on a band of the triangle left in device memory (rows that start inside a tile), on the rectangle of two matrices
    (STORM_wrapper_square's shape, storm.c:153-171), and as what k2_tile_shape = 0 chooses for matrices of few 256 x 256 tiles —
    against the oracle on sampled tiles and against tilebits8_kernel entry by entry."""
    import torch
    try:
        for M, N, d in ((9000, 700, 3000), (4096, 2309, 1500), (1536, 4700, 500)):
            mat = synth.dense_matrix_c(M, N, d, seed=N + M)
            m = hip_ctx.matrix_from_host(mat)
            hip_ctx.set_option("k2_tile_shape", 2)
            ref = m.pairw_matrix("and")
            assert np.array_equal(ref[:200, :N], np.triu(orc.tile_counts(mat, 0, 200, 0, N), k=1)[:200].astype(np.uint32))
            for wt in (1, 2):
                hip_ctx.set_option("k2_tile_shape", 6)
                hip_ctx.set_option("k2_part_slots", wt)
                got = m.pairw_matrix("and")
                assert np.array_equal(ref, got), (M, N, wt, np.argwhere(ref != got)[:3].tolist())
                band = torch.zeros((300, N + 5), dtype=torch.int32, device="cuda:0")
                m.pairw_matrix_band_device(band.data_ptr(), N + 5, 333, 300, "xor")
                rcn = m.row_counts().astype(np.int64)
                want = np.triu((rcn[:, None] + rcn[None, :] - 2 * ref.astype(np.int64)), k=1)[333:633]
                assert np.array_equal(np.triu(band.cpu().numpy().astype(np.int64)[:, :N], k=334), want), (M, N, wt)
                na = N // 3
                ma, mb = hip_ctx.matrix_from_host(mat[:na]), hip_ctx.matrix_from_host(mat[na:])
                got = ma.square_matrix(mb, "and")
                assert hip_ctx.get_option("k2_tile_shape_used") == 6
                full = ref + ref.T
                assert np.array_equal(got, full[:na, na:]), (M, N, wt)
                if N <= 800:
                    assert np.array_equal(got, orc.tile_counts(mat, 0, na, na, N).astype(np.uint32))
                ma.close()
                mb.close()
            # the automatic rule: few tiles -> K2w, and the same numbers
            _reset_tiles(hip_ctx)
            got = m.pairw_matrix("or")
            hip_ctx.set_option("k2_tile_shape", 2)
            assert np.array_equal(got, m.pairw_matrix("or"))
            m.close()
        _reset_tiles(hip_ctx)
        m = hip_ctx.matrix(2048, 1024)
        m.fill_synthetic(65536, 20000, seed=5)
        out = torch.zeros((2048, 2048), dtype=torch.int32, device="cuda:0")
        m.pairw_matrix_device(out.data_ptr(), 2048, "and")
        assert hip_ctx.get_option("k2_tile_shape_used") == 6
        assert int(out.to(torch.int64).sum().item()) == m.pairw() == m.column_identity()
        m.close()
    finally:
        _reset_tiles(hip_ctx)


def test_lists_matrix_at_the_readme_storm_shape_against_the_oracle_on_sampled_blocks(orc):
    """VERDICT r5 (thin spot a): K5 — the per-pair matrix of a list-only STORM_t straight from its lists — at BASELINE c4's
    shape (N = 10000, M = 524288) used to be checked against the handle's own total and the product's own dense-replica
    kernels only. Here two 64-row blocks of the matrix (one inside, one at the ragged end) against the oracle's row-pair
    function (storm.c:790-814: block-id merge + STORM_intersect_vector16_cardinality, storm.c:4-73, per pair) at the two
    sparsest README loads, for the kernel the automatic rule picks and for both list kernels forced."""
    import torch
    lib = sb.load()
    N, M = 10000, 524288
    try:
        dev = torch.zeros((N, N), dtype=torch.int32, device="cuda:0")
        for d in (104, 524):
            s = sb.Storm()
            assert s.add_synthetic(M, N, d, seed=42) == N
            o = orc.storm(synth.positions(M, N, d, seed=42))
            want = {i0: o.pair_counts(i0, i0 + 64) for i0 in (4032, N - 64)}
            for lists, kernel in ((-1, 0), (1, 1), (1, 2)):
                assert lib.STORM_hip_set_option(b"matrix_lists", lists) == 0
                assert lib.STORM_hip_set_option(b"matrix_lists_kernel", kernel) == 0
                dev.zero_()
                s.pairw_matrix_device(dev.data_ptr(), N, N)
                for i0, w in want.items():
                    got = dev[i0:i0 + 64].cpu().numpy().astype(np.uint32)
                    cols = np.arange(N)[None, :] > (i0 + np.arange(64))[:, None]
                    assert np.array_equal(got * cols, w * cols), (d, lists, kernel, i0)
            s.free()
    finally:
        lib.STORM_hip_set_option(b"matrix_lists", -1)
        lib.STORM_hip_set_option(b"matrix_lists_kernel", 0)


def test_tile_kernels_with_more_tiles_than_cus_against_the_oracle_on_sampled_tiles(hip_ctx, orc):
    """VERDICT r5 (thin spot b): tilering_kernel with more tiles than CUs (whole rounds + a cut last round of k-parts) had only
    tilebits8_kernel as its reference. N = 4700 short rows = 190 tiles of 256 x 256 on 256 CUs is below that; N = 6000 = 300
    tiles: one whole round and a last round of 44 tiles in k-parts. Sampled 256 x 256 tiles — first, interior, on the
    diagonal, in the ragged last column, the very last (all of the cut round) — against the oracle's per-pair counts
    (storm.c:1199-1238 with the leaf's result kept), for both 256 x 256 kernels and K2h."""
    import torch
    try:
        for M, N, d in ((1536, 6000, 500), (1000, 4700, 300)):
            mat = synth.dense_matrix_c(M, N, d, seed=N + M)
            m = hip_ctx.matrix_from_host(mat)
            out = torch.zeros((N, N), dtype=torch.int32, device="cuda:0")
            nT = (N + 255) // 256
            picks = [(0, 1), (3, 11), (5, 5), (nT - 1, nT - 1), (nT - 2, nT - 1), (2, nT - 1), (nT - 2, nT - 2), (nT // 2, nT // 2)]
            want = {}
            for I, J in picks:
                i1, j1 = min(N, 256 * I + 256), min(N, 256 * J + 256)
                want[(I, J)] = orc.tile_counts(mat, 256 * I, i1, 256 * J, j1).astype(np.uint32)
            for shape in (5, 2, 6):
                hip_ctx.set_option("k2_tile_shape", shape)
                out.zero_()
                m.pairw_matrix_device(out.data_ptr(), N, "and")
                assert hip_ctx.get_option("k2_tile_shape_used") == shape
                for (I, J), w in want.items():
                    i0, j0 = 256 * I, 256 * J
                    got = out[i0:i0 + w.shape[0], j0:j0 + w.shape[1]].cpu().numpy().astype(np.uint32)
                    upper = (j0 + np.arange(w.shape[1]))[None, :] > (i0 + np.arange(w.shape[0]))[:, None]
                    assert np.array_equal(got * upper, w * upper), (M, N, shape, I, J)
            m.close()
    finally:
        _reset_tiles(hip_ctx)


def test_pair_space_shards_against_the_oracle(hip_ctx, orc):
    """VERDICT r5 (thin spot c): the pair-space shard sums at N = 6144 / 8192 (worlds 3 and 5, where the automatic run length
    once differed by rank) were checked against the device's own column identity only: here also against the oracle's
    blocked loop (storm.c:1199-1238) over the downloaded matrix."""
    try:
        for N in (6144, 8192):
            M = 65536
            m = hip_ctx.matrix(N, M // 64)
            m.fill_synthetic(M, M // 3, seed=N)
            want = orc.wrapper_diag_blocked(m.download(), 31)
            assert m.column_identity() == want and m.pairw() == want
            for pairs, world in ((1, 3), (1, 5), (0, 3)):
                hip_ctx.set_option("k2_shard_pairs", pairs)
                assert sum(m.pairw(r, world) for r in range(world)) == want, (N, pairs, world)
            hip_ctx.set_option("k2_shard_pairs", 0)
            m.close()
    finally:
        hip_ctx.set_option("k2_shard_pairs", 0)


def test_rows_added_out_of_order_fall_back_to_the_dense_replica(orc):
    """a list block that is not strictly ascending (a row filled by STORM_add with unsorted values) made
    storm_hip_rowlists_create_blocks fail with EINVAL, and with it every later STORM_pairw_matrix call on the handle, where
    the dense replica — which sets bits in any order — had worked before the lists path existed. Such a container is
    simply not eligible for K5 now."""
    rng = np.random.default_rng(7)
    M, N = 200000, 300
    rows = [np.unique(rng.integers(0, M, size=60)).astype(np.uint32) for _ in range(N)]
    s_sorted, s_mixed = sb.Storm(), sb.Storm()
    for i, r in enumerate(rows):
        s_sorted.add(r)
        if i % 7 == 3:   # some rows arrive with the positions of every 65536-bit block out of order (the blocks themselves in order)
            r = np.concatenate([rng.permutation(r[r // 65536 == b]) for b in np.unique(r // 65536)]).astype(np.uint32)
        s_mixed.add(r)
    want = s_sorted.pairw_matrix("and")
    assert np.array_equal(np.triu(want, k=1), np.triu(orc.storm(rows).pair_counts(), k=1))
    for _ in range(2):
        assert np.array_equal(s_mixed.pairw_matrix("and"), want)
    s_sorted.free()
    s_mixed.free()


def test_list_probe_with_bundles_of_four_groups_against_the_oracle(orc):
    """K4's second form (probe_bundle = 4: probe_lists_fat_kernel, four 128-row groups' tables per workgroup, the far
    stream read once per bundle) is an option, not the default (measured slower, profiles/r06_a_probe_bundle.txt); it must
    still give the reference's totals (storm.c:790-814 per pair, :1088-1115 blocked): row counts that leave a ragged last
    bundle (1 .. 3 groups), a ragged last group, lists only and mixed kinds, then back to one group per workgroup on the
    same handle (the work list is rebuilt when the option changes)."""
    lib = sb._lib.load()
    rng = np.random.default_rng(23)
    M = 2 * 65536 + 999
    try:
        for n_rows, draws in ((130, 60), (517, 500), (640, 3000), (1100, 900), (385, 9000)):
            rows = []
            for r in range(n_rows):
                d = draws if r % 9 else (0 if r % 18 == 0 else 1)
                if draws == 9000 and r % 4 == 0:
                    d = 50000                                        # some blocks become bitmaps
                rows.append(np.unique(rng.integers(0, M, size=d, dtype=np.uint64)).astype(np.uint32))
            want = orc.storm(rows).pairw_blocked(0)
            s = sb.Storm()
            for v in rows:
                s.add(v)
            got = []
            for bundle in (4, 1, 4):
                assert lib.STORM_hip_set_option(b"probe_bundle", bundle) == 0
                got.append(s.pairw_intersect_cardinality_blocked(0))
                got.append(s.pairw_intersect_cardinality())
            assert got == [want] * 6, (n_rows, draws, got, want)
            s.free()
    finally:
        lib.STORM_hip_set_option(b"probe_bundle", -1)


def test_first_matrix_call_on_the_row_lists_equals_the_steady_calls_and_the_oracle(orc):
    """The reference's harness times ONE call right after construction (benchmark.cpp:605-613). On K5 that call uploads the
    raw lists through the pinned ring and orders them by window on the device (lists_expand / lists_count / lists_place
    kernels); the handle is then changed (rows added: the epoch moves, the lists are rebuilt) and called again. Every call
    == the oracle's per-pair counts (storm.c:790-814), for both K5 kernels and for the automatic rule."""
    lib = sb._lib.load()
    rng = np.random.default_rng(31)
    M = 5 * 65536 + 4242
    try:
        for n_rows, draws, lists, kernel in ((300, 90, 1, 1), (530, 700, 1, 2), (257, 2500, 1, 0), (400, 300, -1, 0)):
            rows = [np.unique(rng.integers(0, M, size=(draws if r % 11 else r % 2), dtype=np.uint64)).astype(np.uint32)
                    for r in range(n_rows)]
            assert lib.STORM_hip_set_option(b"matrix_lists", lists) == 0
            assert lib.STORM_hip_set_option(b"matrix_lists_kernel", kernel) == 0
            s = sb.Storm()
            for v in rows[:n_rows - 70]:
                s.add(v)
            want = np.triu(orc.storm(rows[:n_rows - 70]).pair_counts(), k=1)
            first = s.pairw_matrix("and")
            again = s.pairw_matrix("and")
            assert np.array_equal(np.triu(first, k=1), want) and np.array_equal(again, first), (n_rows, draws, lists, kernel)
            for v in rows[n_rows - 70:]:
                s.add(v)
            want = np.triu(orc.storm(rows).pair_counts(), k=1)
            first = s.pairw_matrix("and")
            again = s.pairw_matrix("and")
            assert np.array_equal(np.triu(first, k=1), want) and np.array_equal(again, first), (n_rows, draws, lists, kernel)
            s.free()
    finally:
        lib.STORM_hip_set_option(b"matrix_lists", -1)
        lib.STORM_hip_set_option(b"matrix_lists_kernel", 0)


def test_bit_operand_strips_with_512_row_tiles_against_the_oracle(hip_ctx, orc):
    """K2b's second form (k2_strip_operands = 6: strip16_bits2_kernel, 8 waves, 512-row A tiles, waves w and w + 4 behind one
    B image of which each writes one k-step): an option. Shapes around the edges of its decomposition — one tile (only the
    diagonal phase of eight blocks runs), 2 .. 5 tiles, ragged last blocks, one k-slice, ragged last chunks, an empty row,
    runs of 1 .. 3 stages — for one device and for shards, with the fold in the launch and behind it. A matrix whose zero
    rows do not reach the next multiple of 512 runs the 256-row form (k2_operands_used says which)."""
    shapes = ((64, 300), (100, 448), (4096, 511), (4096, 512), (640, 1000), (4096, 769), (8192, 1500), (4160, 2000),
              (9000, 1300), (30000, 1536), (12345, 2500), (1000, 3000), (65536, 1024))
    try:
        for M, N in shapes:
            for d in (M // 2, max(1, M // 50)):
                mat = synth.dense_matrix_c(M, N, d, seed=N + M)
                mat[N // 2] = 0
                want = orc.wrapper_diag_blocked(mat, 31)
                m = hip_ctx.matrix_from_host(mat)
                hip_ctx.set_option("k2_strip_operands", 6)
                for fold in (-1, 0, 1):
                    hip_ctx.set_option("k2_fold_inline", fold)
                    got = [m.pairw() for _ in range(3)]
                    assert got == [want] * 3, (M, N, d, fold, got, want)
                    assert hip_ctx.get_option("k2_operands_used") == 6
                hip_ctx.set_option("k2_fold_inline", -1)
                for world in (2, 3):
                    assert sum(m.pairw(r, world) for r in range(world)) == want, (M, N, d, world)
                hip_ctx.set_option("k2_strip_operands", 0)
                assert m.pairw() == want and hip_ctx.get_option("k2_operands_used") == 5
                m.close()
        mat = synth.dense_matrix_c(2048, 700, 300, seed=5)     # 700 rows: zero rows up to 768 only
        m = hip_ctx.matrix_from_host(mat)
        hip_ctx.set_option("k2_strip_operands", 6)
        assert m.pairw() == orc.wrapper_diag_blocked(mat, 31) and hip_ctx.get_option("k2_operands_used") == 5
        m.close()
    finally:
        hip_ctx.set_option("k2_strip_operands", 0)
        hip_ctx.set_option("k2_fold_inline", -1)


def test_blocks_edited_between_the_adds_and_the_first_call_do_not_come_from_the_stage(orc):
    """STORM_add stages every block it finishes (bitmaps and, since round 6, lists) on the device; the first all-pairs call
    gathers the arena from the stage ONLY while every block still is what was staged. A row extended through the public
    per-row adder (the reference's structs are public, storm.h:157-200) before that call — a list block more, a bitmap block
    more — must be seen as it is now (storm.c:790-814 per pair on the container's present state)."""
    import ctypes as C
    lib = sb._lib.load()
    lib.STORM_bitmap_cont_add.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    M, N, d = 3 * 65536, 260, 700
    for grow in (300, 9000):                                   # the new block: a list of 300, a bitmap of 9000 positions
        rows = [np.asarray(r, dtype=np.uint32) for r in synth.positions(2 * 65536, N, d, seed=80 + grow)]
        s = sb.Storm()
        for r in rows:
            s.add(r)
        for victim in (3, N - 1):                              # (the per-row adder appends blocks: the new positions lie beyond the row's last block)
            extra = np.arange(2 * 65536 + 17, 2 * 65536 + 17 + grow, dtype=np.uint32)
            conts = C.cast(s._h, C.POINTER(C.c_void_p))[0]     # STORM_s.conts
            assert lib.STORM_bitmap_cont_add(C.c_void_p(conts + victim * 32), extra.ctypes.data_as(C.c_void_p), extra.size) == 1
            rows[victim] = np.concatenate([rows[victim], extra])
        want = orc.storm(rows).pairw()
        assert [s.pairw_intersect_cardinality(), s.pairw_intersect_cardinality_blocked(0)] == [want, want], grow
        s.free()
    # ... and the untouched container does come out right through the stage (lists only; lists and bitmaps)
    for d2 in (700, 30000):
        rows = synth.positions(M, N, d2, seed=5 + d2)
        s = sb.Storm()
        for r in rows:
            s.add(r)
        assert s.pairw_intersect_cardinality() == orc.storm(rows).pairw(), d2
        s.free()


def test_block_stage_through_the_c_abi_with_some_lists_staged_and_some_from_the_host(hip_ctx, orc):
    """storm_hip_stage_* + storm_hip_sparse_create_blocks_staged / storm_hip_rowlists_create_blocks_staged called directly
    (storm.h hands over all of a container's blocks or none): every bitmap block staged, every SECOND list block staged and the
    others with token ~0 (they travel from block_ptr at build time); then every list staged for the row lists' build. About
    150 bitmap blocks and under 1 MiB of lists: one ring buffer of either kind, never sent before the build (the ring and
    chunk limits: tests/test_gpu_stage_edges.py). Totals and per-pair counts against the oracle's STORM_t restatement (storm.c:790-814)."""
    import ctypes as C
    import torch
    lib = sb._lib.load()
    rng = np.random.default_rng(41)
    M, N = 4 * 65536, 330
    rows = []
    for r in range(N):
        d = 40000 if r % 9 == 0 else (2500 if r % 2 else 300)       # some blocks become bitmaps (> 4096 positions in one block)
        rows.append(np.unique(rng.integers(0, M, size=d, dtype=np.uint64)).astype(np.uint32))
    for only_lists in (False, True):
        if only_lists:
            rows = [r[:3000] if len(r) > 3000 else r for r in rows]
            rows = [np.unique((r.astype(np.uint64) * 7919) % M).astype(np.uint32) for r in rows]   # spread: no block beyond 4096
        want_total = orc.storm(rows).pairw()
        stage = C.c_void_p()
        assert lib.storm_hip_stage_create(hip_ctx._h, C.byref(stage)) == 0
        off, ids, kinds, lens, ptrs, toks, keep = [0], [], [], [], [], [], []
        n_list = 0
        for r in rows:
            for b in np.unique(r // 65536):
                v = r[r // 65536 == b] % 65536
                tok = C.c_uint64(0)
                if len(v) >= 4096 and not only_lists:                 # a bitmap block: 1024 words
                    words = np.zeros(1024, dtype=np.uint64)
                    np.bitwise_or.at(words, v // 64, np.uint64(1) << (v % 64).astype(np.uint64))
                    keep.append(words)
                    assert lib.storm_hip_stage_add(hip_ctx._h, stage, words.ctypes.data_as(C.c_void_p), C.byref(tok)) == 0
                    kinds.append(1); lens.append(0)
                else:
                    lst = np.ascontiguousarray(v, dtype=np.uint16)
                    keep.append(lst)
                    n_list += 1
                    if only_lists or n_list % 2 == 0:
                        assert lib.storm_hip_stage_add_list(hip_ctx._h, stage, lst.ctypes.data_as(C.c_void_p), len(lst), C.byref(tok)) == 0
                    else:
                        tok = C.c_uint64(2 ** 64 - 1)
                    kinds.append(0); lens.append(len(lst))
                ids.append(int(b)); ptrs.append(keep[-1].ctypes.data); toks.append(tok.value)
            off.append(len(ids))
        a_off, a_id = np.array(off, dtype=np.uint64), np.array(ids, dtype=np.uint32)
        a_kind, a_len = np.array(kinds, dtype=np.uint8), np.array(lens, dtype=np.uint32)
        a_ptr, a_tok = np.array(ptrs, dtype=np.uint64), np.array(toks, dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        h = C.c_void_p()
        assert lib.storm_hip_sparse_create_blocks_staged(hip_ctx._h, N, len(ids), p(a_off), p(a_id), p(a_kind), p(a_len), p(a_ptr),
                                                         stage, p(a_tok), C.byref(h)) == 0, lib.storm_hip_last_error()
        out = C.c_uint64()
        for _ in range(2):
            assert lib.storm_hip_pairw_sparse(hip_ctx._h, h, 0, 1, C.byref(out)) == 0 and out.value == want_total
        lib.storm_hip_sparse_destroy(hip_ctx._h, h)
        if only_lists:
            l = C.c_void_p()
            assert lib.storm_hip_rowlists_create_blocks_staged(hip_ctx._h, N, len(ids), p(a_off), p(a_id), p(a_kind), p(a_len), p(a_ptr),
                                                               stage, p(a_tok), C.byref(l)) == 0 and l.value, lib.storm_hip_last_error()
            dev = torch.zeros((N, N), dtype=torch.int32, device="cuda:0")
            assert lib.storm_hip_rowlists_pairw_matrix_device(hip_ctx._h, l, 0, C.c_void_p(dev.data_ptr()), N) == 0
            assert np.array_equal(np.triu(dev.cpu().numpy(), k=1), np.triu(orc.storm(rows).pair_counts().astype(np.int32), k=1))
            lib.storm_hip_rowlists_destroy(hip_ctx._h, l)
        bad = a_tok.copy()
        bad[np.flatnonzero(a_kind == 0)[0]] = 1 << 40                # a list token beyond what was staged: refused, not read
        assert lib.storm_hip_sparse_create_blocks_staged(hip_ctx._h, N, len(ids), p(a_off), p(a_id), p(a_kind), p(a_len), p(a_ptr),
                                                         stage, p(bad), C.byref(h)) != 0
        lib.storm_hip_stage_destroy(hip_ctx._h, stage)
