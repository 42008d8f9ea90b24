"""GPU parity tests added in round 2 (run on the MI355X box: pytest -m gpu).

Same rules as tests/test_gpu_parity.py: the product is called through libstorm_hip.so (C-ABI,
via the ctypes mirror of storm.h), the CPU oracle is the checker only.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests.conftest import shipped

import stormbitmaps_amd as sb
from stormbitmaps_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
FAILED = (1 << 64) - 1


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _list_inputs(M, draws_per_row, seed):
    """Rows of mixed density with the caller-side list arrays of STORM_wrapper_diag_list
    (storm.h:95-148): n_alts[N], alt_positions (all rows' sorted set bits), alt_offsets[N]."""
    rows = []
    for i, d in enumerate(draws_per_row):
        rows.append(synth.positions(M, 1, d, seed=seed + i)[0])
    W = (M + 63) // 64
    mat = np.zeros((len(rows), W), dtype=np.uint64)
    for i, r in enumerate(rows):
        r64 = r.astype(np.uint64)
        np.bitwise_or.at(mat[i], (r64 >> np.uint64(6)).astype(np.int64), np.uint64(1) << (r64 & np.uint64(63)))
    n_alts = np.array([len(r) for r in rows], dtype=np.uint32)
    offs = np.zeros(len(rows), dtype=np.uint32)
    offs[1:] = np.cumsum(n_alts)[:-1]
    pos = np.concatenate(rows).astype(np.uint32)
    return mat, n_alts, pos, offs


@pytest.mark.parametrize("M,N", [(4096, 300), (65536, 700), (9000, 131)])
def test_wrapper_diag_list_and_list_blocked_against_oracle(lib, orc, M, N):
    """STORM_wrapper_diag_list / _diag_list_blocked (reference storm.c:190-219, :282-369) through
    libstorm_hip.so with real n_alts / alt_positions / alt_offsets, against the oracle's
    restatement of both loops. The two cutoff conventions differ (`<= cutoff` at :207, `< cutoff`
    at :309), so cutoffs equal to actual row counts are included."""
    rng = np.random.default_rng(M + N)
    draws = rng.choice([1, 3, 8, 20, 60, 200, M // 8, M // 2], size=N)
    mat, n_alts, pos, offs = _list_inputs(M, draws, seed=1000)
    W = mat.shape[1]
    f = orc.leaf(0)
    fl = C.cast(orc.lib.orc_intersect_bitmaps_scalar_list, C.c_void_p)
    truth = orc.truth_columns(mat)
    exact = sorted(set(int(x) for x in n_alts))
    for cutoff in (0, exact[0], exact[len(exact) // 2], exact[len(exact) // 2] + 1, 200, 1 << 30):
        want = orc.lib.orc_wrapper_diag_list(N, _p(mat), W, _p(n_alts), _p(pos), _p(offs), f, fl, cutoff)
        got = lib.STORM_wrapper_diag_list(N, _p(mat), W, _p(n_alts), _p(pos), _p(offs), None, None, cutoff)
        assert got == want == truth, (cutoff, got, want, truth)
        for bs in (0, 7, 31, 500):
            want_b = orc.lib.orc_wrapper_diag_list_blocked(N, _p(mat), W, _p(n_alts), _p(pos), _p(offs),
                                                           f, fl, cutoff, bs)
            got_b = lib.STORM_wrapper_diag_list_blocked(N, _p(mat), W, _p(n_alts), _p(pos), _p(offs),
                                                        None, None, cutoff, bs)
            assert got_b == want_b == truth, (cutoff, bs, got_b, want_b)
    # the library's own leaves are accepted as identity tokens, a foreign function pointer is not
    own_f = C.cast(lib.STORM_intersect_count_scalar, C.c_void_p)
    own_fl = C.cast(lib.STORM_intersect_count_scalar_list, C.c_void_p)
    assert lib.STORM_wrapper_diag_list(N, _p(mat), W, _p(n_alts), _p(pos), _p(offs), own_f, own_fl, 200) == truth
    assert lib.STORM_wrapper_diag_list(N, _p(mat), W, _p(n_alts), _p(pos), _p(offs), f, None, 200) == FAILED


def test_wrapper_diag_list_refuses_lists_that_contradict_the_bitmaps(lib):
    """The device path counts the bitmaps; it equals the reference's list path only when every list
    holds exactly its row's set bits. A list that says otherwise makes the call fail loudly."""
    mat, n_alts, pos, offs = _list_inputs(4096, [5, 9, 2000, 7], seed=7)
    args = lambda na, po: (4, _p(mat), mat.shape[1], _p(na), _p(po), _p(offs), None, None, 200)  # noqa: E731
    ok = lib.STORM_wrapper_diag_list(*args(n_alts, pos))
    assert ok != FAILED
    short = n_alts.copy(); short[1] -= 1                       # list shorter than the row's popcount
    assert lib.STORM_wrapper_diag_list(*args(short, pos)) == FAILED
    moved = pos.copy(); moved[0] ^= 1                            # a listed position whose bit is not set
    if (int(mat[0, moved[0] >> 6]) >> int(moved[0] & 63)) & 1 == 0:
        assert lib.STORM_wrapper_diag_list(*args(n_alts, moved)) == FAILED
        assert b"list" in lib.STORM_hip_error()
    # a dense row (n_alts > cutoff) is never routed to the list leaf: its list is not looked at
    junk = pos.copy(); junk[int(offs[2]):int(offs[2]) + 10] = 0
    assert lib.STORM_wrapper_diag_list(*args(n_alts, junk)) == ok


@pytest.mark.parametrize("draws", (524, 5242, 20971, 52428, 131072, 262144))
def test_sparse_container_at_full_c4_size(hip_ctx, orc, draws):
    """BASELINE config 4 at its real size: STORM_t, N = 10000 rows x M = 524288 bits, at all six
    README loads (README.md:70-77; benchmark.cpp:605-613), through STORM_add + both all-pairs entry
    points. A CPU pairwise oracle needs 30 s .. 1 h here, so the full-size total is checked
    against the column identity of the same bits on the device, and a 600-row subset (rows
    4700..5299 of the same matrix) is checked pairwise against the oracle's STORM_t restatement."""
    M, N = 524288, 10000
    m = hip_ctx.matrix(N, M // 64)
    m.fill_synthetic(M, draws, seed=42)
    want = m.column_identity()
    sub = m.download(4700, 600)
    m.close()
    s = sb.Storm()
    assert s.add_synthetic(M, N, draws, seed=42) == N
    assert s.pairw_intersect_cardinality_blocked(0) == want
    assert s.pairw_intersect_cardinality() == want          # second call: cached device arena
    s.free()
    rows = synth.positions_from_dense(sub)
    o = orc.storm(rows)
    sub_want = o.pairw_blocked(0) if draws <= 5242 or draws >= 131072 else orc.truth_columns(sub)
    s2 = sb.Storm()
    for r in rows:
        s2.add(r)
    assert s2.serialized_size() == o.serialized_size()
    assert s2.pairw_intersect_cardinality_blocked(0) == sub_want == orc.truth_columns(sub)
    s2.free()


def test_storm_t_under_in_process_multi_device_sharding(lib, orc):
    """STORM_hip_set_devices([0, 0, 0]) with a STORM_t handle: three contexts on the one GPU of
    the box, each takes a disjoint shard of the block-column work, partials added on the host."""
    M, N, d = 196608, 1500, 12690   # list- and bitmap-kind blocks mix (about 4230 draws per block)
    rows = synth.positions(M, N, d, seed=11)
    want = orc.storm(rows[:400]).pairw_blocked(0)
    s = sb.Storm()
    for r in rows[:400]:
        s.add(r)
    one = s.pairw_intersect_cardinality()
    assert one == want
    ids = (C.c_int * 3)(0, 0, 0)
    try:
        assert lib.STORM_hip_set_devices(3, ids) == 0
        assert s.pairw_intersect_cardinality() == want             # arena rebuilt for the new config
        assert s.pairw_intersect_cardinality_blocked(0) == want
        big = sb.Storm()
        assert big.add_synthetic(M, N, d, seed=11) == N
        m = sb.HipContext(0).matrix(N, M // 64)
        m.fill_synthetic(M, d, seed=11)
        assert big.pairw_intersect_cardinality() == m.column_identity()
        big.free()
    finally:
        one_dev = (C.c_int * 1)(0)
        assert lib.STORM_hip_set_devices(1, one_dev) == 0
    assert s.pairw_intersect_cardinality() == want
    s.free()


def test_strip_kernel_mfma_shapes_agree(hip_ctx, orc):
    """The default strips run on v_mfma 16x16x128 (option k2_shape = 16); the 32x32x64 form
    (k2_shape = 32) is kept as an independent operand path. Both against the oracle, incl. ragged
    row counts around the 64-row waves' own diagonal blocks, and shards."""
    try:
        for M, N, d in ((4096, 256, 2048), (1000, 131, 300), (65536, 513, 9000), (300, 65, 100), (20000, 1029, 7000)):
            mat = synth.dense_matrix_c(M, N, d, seed=N)
            want = orc.wrapper_diag_blocked(mat, 31)
            m = hip_ctx.matrix_from_host(mat)
            hip_ctx.set_option("k2_strip_operands", 4)     # (these sizes take K2q by default)
            for shape in shipped(hip_ctx, "k2_shape", (16, 32)):
                hip_ctx.set_option("k2_shape", shape)
                assert m.pairw() == want, (M, N, d, shape)
                assert sum(m.pairw(r, 5) for r in range(5)) == want, (M, N, d, shape)
            m.close()
    finally:
        hip_ctx.set_option("k2_shape", 16)
        hip_ctx.set_option("k2_strip_operands", 0)
    assert hip_ctx.get_option("k2_shape") == 16


@pytest.mark.parametrize("M,N,worlds", [(256, 3000, (2, 8)), (4096, 1500, (3, 5, 7)), (65536, 2600, (3, 6, 16)),
                                        (700, 513, (2, 3))])
def test_two_level_ownership_partitions_for_any_world(hip_ctx, orc, M, N, worlds):
    """Shards of the default path: whole k-slices per rank + leftover slices cut along the pair
    space (storm_hip_strip_plan). Also with fewer k-slices than ranks (M = 256: one slice, pure
    pair-space split) and world sizes that do not divide the slice count."""
    mat = synth.dense_matrix_c(M, N, max(1, M // 3), seed=M + N)
    want = orc.truth_columns(mat)
    m = hip_ctx.matrix_from_host(mat)
    assert m.pairw() == want
    for w in worlds:
        parts = [m.pairw(r, w) for r in range(w)]
        assert sum(parts) == want, (w, parts)
        if M <= 256 * w and N >= 2000:   # fewer slices than ranks: every rank still gets work
            assert min(parts) > 0, (w, parts)
    m.close()


def test_hbm_tiled_passes_under_a_shadow_budget(hip_ctx, orc):
    """Option k2_shadow_budget_mb: a matrix whose FP4 shadow (4 x the bits) exceeds the budget is
    multiplied k-chunk by k-chunk over a compact shadow of one chunk (bounded footprint for any
    M x N). Same totals as the one-piece pass, also per shard, with chunk counts that do and do not
    divide the slice count (the last chunk overhangs into zero columns)."""
    cases = (((70000, 1029, 20000), (4, 2, 1)),      # 274 slices, shadow 36 MiB
             ((65536, 6000, 32768), (64, 20)))       # 256 slices, shadow 192 MiB
    try:
        for (M, N, d), budgets in cases:
            m = hip_ctx.matrix(N, (M + 63) // 64)
            m.fill_synthetic(M, d, seed=N)
            want = m.column_identity()
            # (the default path, the strips on bit operands, has no
            #  shadow to bound: same total; the budget is a property of the FP4 strips, pinned here)
            assert m.pairw() == want and hip_ctx.get_option("k2_operands_used") == 5
            hip_ctx.set_option("k2_strip_operands", 4)
            hip_ctx.set_option("k2_shadow_budget_mb", 0)
            assert m.pairw() == want and hip_ctx.last_launch_info()["word_pairs_executed"] == 1
            if N < 2000:
                assert want == orc.truth_columns(m.download())
            for mb in budgets:
                hip_ctx.set_option("k2_shadow_budget_mb", mb)
                assert m.pairw() == want, (M, N, mb)
                chunks = hip_ctx.last_launch_info()["word_pairs_executed"]   # out[2]: k-chunks of the pass
                assert chunks > 1, (M, N, mb, chunks)
                assert sum(m.pairw(r, 3) for r in range(3)) == want, (M, N, mb)
                hip_ctx.set_option("keep_shadow", 1)     # a chunked pass keeps nothing: must still be right
                assert m.pairw() == want and m.pairw() == want
                hip_ctx.set_option("keep_shadow", 0)
                # the persistent-queue forms (32-row and wide strips) under chunks: their queue heads
                # are only re-zeroed at the end of a pass (soak seed 397310033 caught a lost chunk)
                for shape in shipped(hip_ctx, "k2_shape", (32, 16)):
                    hip_ctx.set_option("k2_shape", shape)
                    for persistent in shipped(hip_ctx, "k2_persistent", (1,)):
                        hip_ctx.set_option("k2_persistent", persistent)
                        assert m.pairw() == want and m.pairw() == want, (M, N, mb, shape)
                    hip_ctx.set_option("k2_persistent", 0)
                    assert m.pairw() == want, (M, N, mb, shape)
                hip_ctx.set_option("k2_shape", 16)
            hip_ctx.set_option("k2_strip_operands", 0)
            m.close()
    finally:
        hip_ctx.set_option("k2_strip_operands", 0)
        hip_ctx.set_option("k2_shadow_budget_mb", 96 * 1024)
        hip_ctx.set_option("keep_shadow", 0)
        hip_ctx.set_option("k2_shape", 16)
        hip_ctx.set_option("k2_persistent", 0)


def test_device_copies_follow_direct_edits_and_invalidate(lib, orc):
    """the reference structs are public. STORM_t: rows edited with the public per-row
    adder behind STORM_add's back are caught by the fingerprint; in-place edits of the dense
    buffer need STORM_contig_hip_invalidate."""
    M, N, d = 131072, 300, 900
    rows = synth.positions(M, N + 1, d, seed=21)
    s = sb.Storm()
    for r in rows[:N]:
        s.add(r)
    first = s.pairw_intersect_cardinality()
    assert first == orc.storm(rows[:N]).pairw()
    s.add(np.zeros(0, dtype=np.uint32))                       # an empty row (storm.c:864) ...
    assert s.pairw_intersect_cardinality() == first
    # ... filled directly through the public per-row API on h->conts[N]
    conts = C.cast(s._h, C.POINTER(C.c_void_p))[0]            # STORM_s.conts
    cont_size = 32                                            # sizeof(STORM_bitmap_cont_t): 2 ptrs + 3 u32 (+pad)
    extra = np.ascontiguousarray(rows[N], dtype=np.uint32)
    lib.STORM_bitmap_cont_add.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    assert lib.STORM_bitmap_cont_add(C.c_void_p(conts + N * cont_size), _p(extra), extra.size) == 1
    assert s.pairw_intersect_cardinality() == orc.storm(rows).pairw()
    s.free()
    # dense: flip bits in h->data in place
    c = sb.StormContig(4096)
    mat = synth.dense_matrix_c(4096, 200, 1000, seed=3)
    for r in synth.positions_from_dense(mat):
        c.add(r)
    assert c.pairw_intersect_cardinality() == orc.truth_columns(mat)
    data_ptr = C.cast(c._h, C.POINTER(C.c_void_p))[0]         # STORM_contiguous_s.data
    host = np.ctypeslib.as_array(C.cast(data_ptr, C.POINTER(C.c_uint64)), shape=(200, 64))
    host[:] = ~host
    c.hip_invalidate()
    assert c.pairw_intersect_cardinality() == orc.truth_columns(~mat)
    c.free()


def test_per_pair_matrix_in_bands_over_several_devices(lib, orc):
    """STORM_contig_pairw_matrix with [0, 0, 0] configured: three contexts, each writes one band of
    rows (bands cut for equal pair counts); buffer extent checked by the C entry point."""
    M, N, d = 9000, 1100, 3000
    mat = synth.dense_matrix_c(M, N, d, seed=5)
    want = np.triu(orc.tile_counts(mat, 0, N, 0, N), k=1)
    ids = (C.c_int * 3)(0, 0, 0)
    try:
        assert lib.STORM_hip_set_devices(3, ids) == 0
        c = sb.StormContig(M)
        for r in synth.positions_from_dense(mat):
            c.add(r)
        assert c.n_rows == N
        assert np.array_equal(c.pairw_matrix(), want)
        wide = np.full((N + 3, N + 7), 77, dtype=np.uint32)     # leading dimension > n_rows
        assert lib.STORM_contig_pairw_matrix(c._h, 0, _p(wide), N + 3, N + 7) == 0
        assert np.array_equal(wide[:N, :N], want) and (wide[N:] == 77).all() and (wide[:, N:] == 77).all()
        small = np.zeros((N - 1, N), dtype=np.uint32)
        assert lib.STORM_contig_pairw_matrix(c._h, 0, _p(small), N - 1, N) == -4
        c.free()
    finally:
        one_dev = (C.c_int * 1)(0)
        assert lib.STORM_hip_set_devices(1, one_dev) == 0


@pytest.mark.parametrize("M,N,d", [(196608, 1300, 12690), (524288, 2000, 524), (524288, 1200, 131072), (70000, 300, 7)])
def test_device_arena_from_a_serialized_container(hip_ctx, orc, M, N, d):
    """STORM_serialize -> bytes -> arena built on the device from the bytes
    (storm_hip_sparse_create_serialized: both block kinds unpacked from the uploaded stream) ->
    all-pairs total, against the container path and the column identity of the same bits."""
    s = sb.Storm()
    assert s.add_synthetic(M, N, d, seed=M + N) == N
    want = s.pairw_intersect_cardinality()
    m = hip_ctx.matrix(N, (M + 63) // 64)
    m.fill_synthetic(M, d, seed=M + N)
    assert want == m.column_identity()
    if N <= 300:
        assert want == orc.truth_columns(m.download())
    m.close()
    data = s.serialize()
    assert data.size == s.serialized_size()
    assert sb.Storm.serialized_pairw_intersect_cardinality(data) == want
    back = sb.Storm.deserialize(data)
    assert back.pairw_intersect_cardinality() == want
    back.free()
    s.free()
    with pytest.raises(sb.StormHipError):
        sb.Storm.serialized_pairw_intersect_cardinality(data[: data.size // 2 * 2 - 2])


def test_rows_stream_to_the_device_while_the_container_is_built(lib, orc):
    """STORM_contig_add sends every finished batch of 256 rows to the device mirror, so the first
    all-pairs call at the headline shape has < 256 rows left to copy: first call within 2 x the
    resident call. Totals against the raw-buffer wrapper and, on a subset, the
    oracle; rows added after a call extend the mirror instead of rebuilding it."""
    import time
    M, N, d = 65536, 10000, 32768
    c = sb.StormContig(M)
    assert c.add_synthetic(N - 300, d, seed=42) == N - 300
    t0 = time.perf_counter(); a = c.pairw_intersect_cardinality_blocked(31); t1 = time.perf_counter()
    b = c.pairw_intersect_cardinality_blocked(31); t2 = time.perf_counter()
    assert a == b
    first, resident = t1 - t0, t2 - t1
    print(f"first call {1e3 * first:.2f} ms, resident call {1e3 * resident:.2f} ms")
    assert c.add_synthetic(300, d, seed=42, row0=N - 300) == 300      # grows the mirror
    total = c.pairw_intersect_cardinality()
    ctx = sb.HipContext(0)
    m = ctx.matrix(N, M // 64)
    m.fill_synthetic(M, d, seed=42)
    assert total == m.column_identity()
    head = ctx.matrix(N - 300, M // 64)
    head.import_device(m.device_ptr, N - 300, m.stride_words)
    assert a == head.pairw()
    for x in (m, head):
        x.close()
    ctx.close()
    c.free()
    assert first < 2.0 * resident + 1e-3, (first, resident)


def test_materialised_output_for_rows_beyond_exact_f32_range(hip_ctx, orc):
    """Rows of 2^24 bits and more: one f32 accumulator cannot hold a whole row's count exactly, so
    every tile of the materialised output is cut along k and the parts are added.
    What this proves: the bookkeeping of the k-cut (parts that cover the row once, added as integers) on rows of more than
    2^24 bits against the oracle. What it cannot: exactness — the rows are ~63 % dense, pair counts ~6.7e6 stay below 2^24
    (f32 holds every integer up to there), and with 70 rows the planner cuts every tile into short parts for load balance
    anyway, so this test passes with the exactness cut removed. Rows whose counts are odd and beyond 2^24 in items that stay
    whole: tests/test_gpu_dense_edges.py::test_per_pair_output_of_odd_saturated_rows_around_two_to_the_24_bits."""
    M, N = (1 << 24) + 4096, 70
    m = hip_ctx.matrix(N, M // 64)
    m.fill_synthetic(M, M, seed=3)            # ~63 % density: pair counts ~ 6.7e6
    host = m.download()
    want = np.triu(orc.tile_counts(host, 0, N, 0, N), k=1)
    assert want.max() > (1 << 22)
    assert np.array_equal(m.pairw_matrix("and"), want)
    assert np.array_equal(m.pairw_matrix("xor"), np.triu(orc.tile_counts_op(host, 0, N, 0, N, 2), k=1))
    assert m.pairw() == int(want.sum(dtype=np.uint64)) == m.column_identity()
    m.close()


@pytest.mark.parametrize("M,N,d", [(524288, 2000, 524), (524288, 1037, 104), (196608, 2100, 40), (262144, 517, 1500),
                                   (65536, 300, 3)])
def test_list_probe_kernel_for_columns_of_short_lists(hip_ctx, orc, M, N, d):
    """K4 (reference regime: list x list blocks, storm.c:4-73 through the kind dispatch :618-656):
    block columns whose blocks are all short lists are counted by the probe kernel (transposed 16-row
    bitmap in the LDS, streamed (row, position) elements) instead of being expanded to dense pool
    rows. Same totals as the dense-on-present-blocks path and the oracle, per shard too; rows with
    no values and row counts that are not multiples of 16 included."""
    rows = synth.positions(M, N, d, seed=M + N + d)
    rows[7] = np.zeros(0, dtype=np.uint32)
    rows[N - 1] = rows[N - 1][:1]
    s = sb.Storm()
    for r in rows:
        s.add(r)
    ctx = sb.HipContext(0)                     # option changes must not leak into other tests' context
    lib = sb.load()
    want = orc.storm(rows).pairw_blocked(0) if N * d <= 2_000_000 else None
    data = s.serialize()
    h = C.c_void_p()
    assert lib.storm_hip_sparse_create_serialized(ctx._h, data.ctypes.data_as(C.c_void_p), data.size, C.byref(h)) == 0
    out = C.c_uint64()
    got = {}
    try:
        for probe in (0, 1, -1):
            ctx.set_option("sparse_probe", probe)
            assert lib.storm_hip_pairw_sparse(ctx._h, h, 0, 1, C.byref(out)) == 0, lib.storm_hip_last_error()
            got[probe] = out.value
            used = ctx.last_launch_info()["segments"]            # out[3]: columns the probe kernel counted
            auto = d * 65536 // M <= 1000                         # mean list length per block vs the auto rule
            assert (used > 0) == (probe == 1 or (probe == -1 and auto)), (probe, used)
            parts = []
            for r in range(3):
                assert lib.storm_hip_pairw_sparse(ctx._h, h, r, 3, C.byref(out)) == 0
                parts.append(out.value)
            assert sum(parts) == got[probe], (probe, parts)
    finally:
        lib.storm_hip_sparse_destroy(ctx._h, h)
        ctx.close()
    assert got[0] == got[1] == got[-1], got
    if want is not None:
        assert got[0] == want
    assert s.pairw_intersect_cardinality() == got[0]
    s.free()


@pytest.mark.parametrize("M,N,d", [(9000, 1100, 4000), (4096, 1024, 700), (70000, 777, 30000), (512, 1301, 200),
                                   (3000, 662, 1000), (2048, 968, 600)])
def test_materialised_output_kernels_agree_with_the_oracle(hip_ctx, orc, M, N, d):
    """Option k2_tile_shape: the bit-operand kernels (2 = two waves per SIMD, the default; 1 = one wave per
    SIMD: rows DMA'd as bits, inflated to FP4 in registers, per-class block scales; 3 / 4 = round 4's K2tb:
    the B half's FP4 images built once per workgroup in the LDS, 16x16x128 / 32x32x64 MFMAs, two workgroups
    per tile item, every block range its loop is instantiated for) and the FP4-shadow
    kernels (16, 32) write the same triangle, for every op. Shapes with interior tiles (stored through
    the LDS, 16 bytes per lane) and with none, row counts that are and are not multiples of 4 (the
    host entry point's ld = N decides whether the wide stores may be used), rows shorter than one stage,
    and ragged last row blocks of 9 / 21 / 76 / 150 / 200 rows: the default kernel multiplies 0..4 column
    blocks per wave there (every instantiation of its loop body), and 4 - wa on diagonal tiles."""
    import torch
    mat = synth.dense_matrix_c(M, N, d, seed=M + N)
    m = hip_ctx.matrix_from_host(mat)
    want = {"and": np.triu(orc.tile_counts(mat, 0, N, 0, N), k=1)}
    for code, name in ((1, "or"), (2, "xor")):
        want[name] = np.triu(orc.tile_counts_op(mat, 0, N, 0, N, code), k=1)
    try:
        for shape in shipped(hip_ctx, "k2_tile_shape", (2, 5, 3, 4, 1, 16, 32)):
            hip_ctx.set_option("k2_tile_shape", shape)
            for name in ("and", "or", "xor"):
                assert np.array_equal(m.pairw_matrix(name), want[name]), (shape, name)
            # device output with a padded, 16-byte aligned leading dimension (interior tiles take the wide
            # stores) and with an odd one (they must not)
            for ld in ((N + 3) // 4 * 4 + 8, N + 1):
                out = torch.full((N, ld), 0xABCD, dtype=torch.int32, device="cuda:0")
                m.pairw_matrix_device(out.data_ptr(), ld, "and")
                got = out.cpu().numpy().astype(np.uint32)
                assert np.array_equal(np.triu(got[:, :N], k=1), want["and"]), (shape, ld)
                # nothing outside the strict upper triangle is touched
                assert np.all(got[:, :N][np.tril_indices(N)] == 0xABCD) and np.all(got[:, N:] == 0xABCD), (shape, ld)
            # a band that starts and ends inside row blocks
            r0, nb = 130, min(N - 130, 600)
            band = torch.zeros((nb, N), dtype=torch.int32, device="cuda:0")
            m.pairw_matrix_band_device(band.data_ptr(), N, r0, nb, "xor")
            assert np.array_equal(band.cpu().numpy().astype(np.uint32), want["xor"][r0:r0 + nb]), shape
    finally:
        hip_ctx.set_option("k2_tile_shape", 0)
        m.close()


def test_rectangle_output_on_bit_operands(hip_ctx, orc):
    """storm_hip_square_matrix with the bit-operand kernels: A and B are separate allocations behind
    one virtual row space; blocks of A and of B that are full, partial and (B shorter than a block)
    nearly empty."""
    M = 20000
    mat = synth.dense_matrix_c(M, 1500, 7000, seed=77)
    for na, nbr in ((900, 600), (256, 1024), (37, 1463)):
        a, b = mat[:na], mat[na:na + nbr]
        ma, mb = hip_ctx.matrix_from_host(a), hip_ctx.matrix_from_host(b)
        want = orc.tile_counts(mat, 0, na, na, na + nbr)
        try:
            for shape in shipped(hip_ctx, "k2_tile_shape", (2, 5, 3, 4, 1, 16)):
                hip_ctx.set_option("k2_tile_shape", shape)
                assert np.array_equal(ma.square_matrix(mb, "and"), want), (na, nbr, shape)
            want_x = orc.tile_counts_op(mat, 0, na, na, na + nbr, 2)
            assert np.array_equal(ma.square_matrix(mb, "xor"), want_x), (na, nbr)
        finally:
            hip_ctx.set_option("k2_tile_shape", 0)
            ma.close()
            mb.close()


def test_strips_on_bit_operands(hip_ctx, orc):
    """Options k2_strip_operands = 1 and 2: the strips read the bit matrix itself (512-bit k-slices, rows
    inflated to FP4 in registers, no shadow; 2 = one stage stream per workgroup, one launch). Matrices created under the option (row pitch padded off
    multiples of 1 KiB) and before it (dense pitch); against the oracle where the CPU can afford it,
    against the column identity and the FP4 strips otherwise; shards; ragged rows around the waves' own
    diagonal blocks. The larger shapes put several workgroups on every CU: that is where an LDS read that
    lands in the registers of a just-issued MFMA's operand gave totals that changed from run to run."""
    try:
        for M, N, d, check_oracle in ((4096, 256, 2048, True), (1000, 131, 300, True), (65536, 513, 9000, True),
                                      (300, 65, 100, True), (20000, 1029, 7000, True), (65536, 2000, 32768, False),
                                      (70000, 777, 30000, False), (32768, 2000, 16000, False)):
            for created_under in shipped(hip_ctx, "k2_strip_operands", (1, 4)):
                hip_ctx.set_option("k2_strip_operands", created_under)
                m = hip_ctx.matrix(N, (M + 63) // 64)
                m.fill_synthetic(M, d, seed=N)
                assert (m.stride_words * 8) % 1024 != 0 or created_under == 4
                want = m.column_identity()
                if check_oracle and created_under == 1:
                    assert want == orc.wrapper_diag_blocked(m.download(), 31)
                for operands in shipped(hip_ctx, "k2_strip_operands", (1, 2, 4)):
                    hip_ctx.set_option("k2_strip_operands", operands)
                    got = [m.pairw() for _ in range(4 if operands != 4 else 1)]
                    assert got == [want] * len(got), (M, N, d, created_under, operands, got, want)
                    assert sum(m.pairw(r, 3) for r in range(3)) == want, (M, N, d, created_under, operands)
                m.close()
    finally:
        hip_ctx.set_option("k2_strip_operands", 0)
    assert hip_ctx.get_option("k2_strip_operands") == 0


def test_sparse_contiguous_containers_take_the_list_path(lib, orc):
    """A STORM_contiguous_t whose rows are ALL sparse (at most M / 16 positions: the reference's list regime,
    storm.c:1151-1162, widened to the density up to which blocks stay lists) is mirrored into a private STORM_t and
    totalled by the list-probe kernel; the first denser row ends that for good, STORM_contig_clear starts over, an in-place edit
    (STORM_contig_hip_invalidate) ends it too. Every state against the oracle's container; the timing
    line pins that the list path is the one that ran (an order of magnitude at 20 positions per row)."""
    import time
    M, N = 131072, 6000
    rows = synth.positions(M, N + 2, 20, seed=5)           # 20 draws per row, cutoff 200
    dense_row = synth.positions(M, 1, 20000, seed=6)[0]    # > M / 16 positions
    c, oc = sb.StormContig(M), orc.contig(M, ())
    for r in rows[:N]:
        c.add(r)
        oc.add(r)
    want = oc.pairw()
    assert c.pairw_intersect_cardinality() == want == c.pairw_intersect_cardinality_blocked(31)
    t_lists = 1e9     # best of 5 (a mean lets one hiccup of the box decide: 1.05 ms was measured once where 0.03 is the rule)
    for _ in range(5):
        t0 = time.perf_counter()
        assert c.pairw_intersect_cardinality() == want
        t_lists = min(t_lists, time.perf_counter() - t0)
    # a dense row: back to the dense mirror (filled in on demand: nothing was streamed while all rows were lists)
    c.add(dense_row)
    oc.add(dense_row)
    want2 = oc.pairw()
    assert c.pairw_intersect_cardinality() == want2
    c.add(rows[N])        # sparse rows after it do not bring the list path back
    oc.add(rows[N])
    want3 = oc.pairw()
    assert c.pairw_intersect_cardinality() == want3
    t_dense = 1e9
    for _ in range(5):
        t0 = time.perf_counter()
        assert c.pairw_intersect_cardinality() == want3
        t_dense = min(t_dense, time.perf_counter() - t0)
    assert t_lists * 3 < t_dense, (t_lists, t_dense)
    # clear: a fresh start
    c.clear()
    oc2 = orc.contig(M, ())
    for r in rows[:500]:
        c.add(r)
        oc2.add(r)
    assert c.pairw_intersect_cardinality() == oc2.pairw()
    c.hip_invalidate()
    assert c.pairw_intersect_cardinality() == oc2.pairw()
    assert np.array_equal(c.pairw_matrix("and"), np.triu(orc.tile_counts(oc2.dense(), 0, 500, 0, 500), k=1))
