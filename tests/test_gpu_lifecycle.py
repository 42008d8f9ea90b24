"""Container lifecycles give device and pinned memory back.

Every other GPU test checks what a call computes; these check what the library still HOLDS after "make a container, ask,
free", cycle after cycle. One helper, `held()`, reads two numbers:

  device_bytes   total - free of hipMemGetInfo (torch.cuda.mem_get_info): every hipMalloc of the process, whoever made it;
  pinned_bytes   the VmRSS line of /proc/self/status: a hipHostMalloc is resident, pinned host memory.

A loop runs WARMUP unmeasured cycles (code objects, the runtime's own pools, the first growth of the work-list buffers),
then MEASURED cycles with a reading after each and one before the first. Every cycle builds its containers from data seeded
by the cycle number — the same shapes, other bits, so a device copy that survived a free and is found again answers
wrongly —, asserts every answer against a value computed on the host, asserts which path ran (STORM_hip_last_pass) and frees
what it made. No torch tensor is made and no cache emptied between two readings: device outputs go into the one buffer of
the `dev_out` fixture, host outputs into numpy.

Pass condition, per loop and per observation: of the MEASURED increases max(0, held[i] - held[i - 1]) the two largest are
dropped (a step that is not ours: another tenant of the card, a pool that grows late) and the rest must sum to less than
half of the smallest thing a loop can lose once, which the code states and no measurement: 32 MiB of device memory (half a
64 MiB stage chunk, kChunkBlocks * kBlockBytes / kStageListChunk), 8 MiB of pinned memory (half the 16 MiB of rings of one
stage, storm_hip_stage_create). A loss per cycle costs fourteen times the whole; a loop that gives everything back costs
nothing. What this cannot see: a loss below the granularity of the allocators (a forgotten 64-byte scratch word leaves both
numbers where they were for thousands of cycles), and host memory that never becomes resident.

Host references: per-pair counts are a float32 product of 0 / 1 rows over the columns the generator can draw from (`_counts`;
sums stay below 2^24, so exact; compared once with tests/test_gpu_similarity.py's `_numpy_counts`); floats come from that
file's exact `expected` / `check` (1 ulp, NaN exactly where undefined), top-k orders from tests/test_gpu_topk.py's `rank`,
dosage values from numpy int64 products and the float64 formulas of tests/test_gpu_dosage*.py (1 ulp).

Loops 1 (matrix calls only: no totals call may have drained anything before it) and 9 (STORM_hip_shutdown destroys the
contexts every other test shares) run in a child process with a time limit of its own.

A reading that dips once and comes back counts as one increase (STORM_hip_invalidate in the reused-handle loop releases
a stage a round earlier than the other rounds do: one step of 64 MiB / 16 MiB back up, which the two dropped increases
absorb). Every cycle of a loop makes the same calls: with the call families in rotation the host references alone moved
the resident set by 5 - 8 MB every fourth cycle.

Measured on one MI355X:
  VmRSS around a stage on a context of the test's own (test_a_stage_ring_shows_in_the_pinned_observation), in KiB:
    1474512 before, 1490960 while the stage lives (+16448), 1445964 after stage and context are gone; VmLck and VmPin
    stay 0 throughout (a hipHostMalloc is an anonymous mapping the driver pins: resident, not accounted as locked)
  increases of the STORM_contiguous_t loop, which never leaked: sixteen times 0 bytes, device and pinned alike
  the matrix-only loop on the library before storm_hip_stage_create drained: 67108864 bytes of device and 16777216 of
  pinned memory in every cycle (the loop of two containers: 33554432 pinned, the reused handle: 67108864 and ~16.8 MB)
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import stormbitmaps_amd as sb
from tests.test_gpu_dosage import ordered, pack
from tests.test_gpu_dosage_complete import complete_reference, complete_sums
from tests.test_gpu_lag_matrix import to_lag
from tests.test_gpu_similarity import _numpy_counts, check, expected
from tests.test_gpu_storm_edges import _block_fns, _probe_expected, _row_ptr
from tests.test_gpu_topk import assert_topk, rank, top

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MiB = 1 << 20
WARMUP, MEASURED = 3, 16
DEVICE_BOUND, PINNED_BOUND = 32 * MiB, 8 * MiB      # half a 64 MiB chunk, half the 16 MiB of rings of one stage
STAGE_RINGS = 16 * MiB                              # 2 * kBufBlocks * kBlockBytes + 2 * kStageListBuf
BLOCK = 65536
NAN_BITS = 0x7FC00000
SENTINEL = 0x5EA1ED
RAN_DENSE_TOTALS = 1 | 2 | 4 | 8 | 16               # the kernels an all-pairs total of a dense matrix can report
RAN_FP4_STRIPS, RAN_PROBE, RAN_LISTS_MATRIX, RAN_TILES_OUT, RAN_SIMILARITY, RAN_TOPK = 4, 32, 64, 128, 512, 1024


# ------------------------------------------------------------------------------------------ the observation
def _status_kib(field):
    with open("/proc/self/status") as f:
        for line in f:
            if line.startswith(field + ":"):
                return int(line.split()[1])
    raise AssertionError(f"/proc/self/status has no {field}")


def held():
    """(device_bytes, pinned_bytes): see the module docstring"""
    import torch
    free, total = torch.cuda.mem_get_info(0)
    return total - free, _status_kib("VmRSS") * 1024


def _torch_ready():
    import torch
    torch.cuda.init()
    torch.zeros(1, device="cuda:0")
    torch.cuda.synchronize()


def assert_steady(readings, what):
    """the pass condition over MEASURED + 1 readings; the increases (device, pinned) for the record"""
    assert len(readings) == MEASURED + 1
    kinds = (("device", DEVICE_BOUND), ("pinned", PINNED_BOUND))
    all_inc = [[max(0, readings[i][k] - readings[i - 1][k]) for i in range(1, len(readings))] for k in range(len(kinds))]
    for (name, _), inc in zip(kinds, all_inc):
        print(f"{what}: {name} increases {inc}")
    for (name, bound), inc in zip(kinds, all_inc):
        assert sum(sorted(inc)[:-2]) < bound, f"{what}: {name} memory keeps growing: increases per cycle {inc} (bytes)"
    return all_inc


def run_loop(cycle, what):
    for i in range(WARMUP):
        cycle(i)
    readings = [held()]
    for i in range(WARMUP, WARMUP + MEASURED):
        cycle(i)
        readings.append(held())
    return assert_steady(readings, what)


# ------------------------------------------------------------------------------------------ data and host references
def _shape(n, columns, seed):
    """the part of a container's rows that every cycle shares: per block column (block id, span, positions per row) —
    columns: (block id, span, lo, hi): between lo and hi positions per row, drawn from the first `span` bits of the block's
    65536-bit window (4096 and more make a bitmap block, fewer a list block)"""
    rng = np.random.default_rng(seed)
    return [(b, span, rng.integers(lo, hi + 1, size=n)) for b, span, lo, hi in columns]


def _rows(shape, i, salt=0):
    """the rows of cycle i: the shape's sizes, positions seeded by (salt, i)"""
    rng = np.random.default_rng([salt, i])
    n = len(shape[0][2])
    return [np.concatenate([b * BLOCK + np.sort(rng.choice(span, size=int(sizes[r]), replace=False))
                            for b, span, sizes in shape]).astype(np.uint32) for r in range(n)]


def _cols(*shapes):
    """(column of every position the shapes can draw, -1 for every other position; the number of columns)"""
    drawn = np.unique(np.concatenate([b * BLOCK + np.arange(span) for shape in shapes for b, span, _ in shape]))
    column = np.full(int(drawn[-1]) + 1, -1, dtype=np.int64)
    column[drawn] = np.arange(drawn.size)
    return column, int(drawn.size)


_DENSE = {}


def _dense(rows, cols, slot):
    """0 / 1 float32 rows over the columns of `cols`, in a buffer kept per (slot, shape): the big host allocations of a
    cycle are the same memory every time, so that the resident set moves with the library and not with numpy"""
    column, width = cols
    key = (slot, len(rows), width)
    if key not in _DENSE:
        _DENSE[key] = np.zeros((len(rows), width), dtype=np.float32)
    m = _DENSE[key]
    m.fill(0)
    at = column[np.concatenate(rows)]
    assert (at >= 0).all()
    m[np.repeat(np.arange(len(rows)), [r.size for r in rows]), at] = 1
    assert int(m.sum()) == at.size                     # (no position twice in a row)
    return m


def _counts(rows_a, rows_b, cols):
    """|A_i & B_j| for every pair, int64 [na, nb]: a float32 product of 0 / 1 rows (every sum is an integer below 2^24)"""
    assert cols[1] < 1 << 24
    da = _dense(rows_a, cols, "a")
    db = da if rows_b is rows_a else _dense(rows_b, cols, "b")
    return np.rint(da @ db.T).astype(np.int64)


def _upper(n):
    return np.triu(np.ones((n, n), dtype=bool), 1)


def _last_pass():
    out = (C.c_uint64 * 4)()
    assert sb.load().STORM_hip_last_pass(out) == 0
    return int(out[0])


def _set(key, value):
    assert sb.load().STORM_hip_set_option(key.encode(), value) == 0, key


def _storm(rows):
    s = sb.Storm()
    for r in rows:
        assert s.add(r) == 1
    return s


def _contig(rows, M):
    c = sb.StormContig(M)
    for r in rows:
        assert c.add(r) == r.size
    return c


def _topk_counts(c_full, k, skip_self):
    """(idx, val) of the k largest counts per row of the full count matrix: value descending, then column ascending"""
    return top(rank(c_full.astype(np.uint32), "count", skip0=0 if skip_self else None), k, "count")


def _check_floats(bits, want64, nan, where, what):
    """float32 bits against float64 values: NaN (the one quiet pattern) exactly where `nan`, elsewhere within 1 ulp"""
    bits = np.ascontiguousarray(bits).view(np.uint32)
    is_nan = (bits & 0x7FFFFFFF) > 0x7F800000
    assert np.array_equal(is_nan & where, nan & where), what
    assert (bits[nan & where] == NAN_BITS).all(), what
    ok = where & ~nan
    ulps = np.abs(ordered(bits[ok]) - ordered(want64[ok].astype(np.float32).view(np.uint32)))
    assert int(ulps.max(initial=0)) <= 1, (what, int(ulps.max()))


# rows of two bitmap blocks and a list block: 600 bitmap blocks per container, so that the stage has sent its ring once
# (kBufBlocks = 512) and holds a 64 MiB chunk
MIXED = _shape(300, ((0, 8192, 4500, 6000), (1, 8192, 4500, 6000), (2, 4096, 10, 900)), seed=1)
MIXED_COLS, MIXED_BITS = _cols(MIXED), 3 * BLOCK
LAG, K = 40, 5


@pytest.fixture(scope="module", autouse=True)
def torch_ready():
    _torch_ready()


@pytest.fixture(scope="module")
def dev_out(torch_ready):
    """the one device output buffer of the file, made before any reading"""
    import torch
    t = torch.empty((320, 320), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    return t


@pytest.fixture(autouse=True)
def _restore_options():
    yield
    sb.load().STORM_hip_set_option(b"matrix_lists", -1)


def _matrix_families(s, c, a, M, rng):
    """the four matrix-shaped questions of a STORM_t, asserted against the full count matrix c and the row counts a. (All
    four in every cycle: with one family per cycle in rotation the host references of the ld_r2 cycle hold 5 - 8 MB more
    than the others', and the resident set showed that saw-tooth as four increases — measured, without the library.)"""
    n = s.n_rows
    up = _upper(n)
    assert np.array_equal(s.pairw_matrix("and").astype(np.int64), np.where(up, c, 0))
    assert _last_pass() == RAN_TILES_OUT
    want, nan = expected("ld_r2", c, a, a, M, rng)
    got = s.pairw_similarity("ld_r2", n_bits=M)
    assert _last_pass() == RAN_TILES_OUT | RAN_SIMILARITY
    assert (got.view(np.uint32)[~up] == 0).all()
    check(got.view(np.uint32), want, nan, up, "ld_r2")
    want, nan = expected("cosine", c, a, a, M, rng)
    got = s.pairw_lag_similarity(LAG, "cosine", n_bits=M)
    assert _last_pass() == RAN_TILES_OUT | RAN_SIMILARITY
    inside = to_lag(up, LAG, fill=False)
    assert got.shape == (n, LAG) and (got.view(np.uint32)[~inside] == 0).all()
    check(got.view(np.uint32), to_lag(want, LAG), to_lag(nan, LAG, fill=False), inside, "lag cosine")
    got = s.pairw_topk(K, "count")
    assert _last_pass() == RAN_TILES_OUT | RAN_TOPK
    assert_topk(got, _topk_counts(c, K, True), "topk count")


# ------------------------------------------------------------------------------------------ the observation itself
def test_host_counts_agree_with_numpy_counts():
    rows = _rows(MIXED, 0)[:40]
    assert np.array_equal(_counts(rows, rows, MIXED_COLS), _numpy_counts(rows, rows, MIXED_BITS))
    assert all(np.array_equal(r, np.unique(r)) for r in rows)


def test_a_stage_ring_shows_in_the_pinned_observation():
    """the 16 MiB of pinned rings of a stage are in VmRSS while the stage lives and gone once its context is"""
    lib = sb.load()
    ctx = sb.HipContext(0)
    try:
        assert lib.storm_hip_ctx_reserve_staging(ctx._h) == 0      # (the builder's own 24 MiB ring: not what is measured)
        before = _status_kib("VmRSS")
        stage = C.c_void_p()
        assert lib.storm_hip_stage_create(ctx._h, C.byref(stage)) == 0, lib.storm_hip_last_error()
        during = _status_kib("VmRSS")
        lib.storm_hip_stage_destroy(ctx._h, stage)
    finally:
        ctx.close()
    after = _status_kib("VmRSS")
    print(f"VmRSS around a stage: {before} {during} {after} KiB")
    assert STAGE_RINGS * 3 // 4 <= (during - before) * 1024 <= STAGE_RINGS * 5 // 4, (before, during, after)
    assert (during - after) * 1024 >= STAGE_RINGS * 3 // 4, (before, during, after)


# ------------------------------------------------------------------------------------------ 1. matrix calls only
def _loop_matrix_calls_only():
    """new STORM_t with bitmap and list blocks, the four matrix-shaped calls, free: the container's
    stage is never consumed by an arena build, and nothing on this path used to release what STORM_free put off"""
    def cycle(i):
        rng = np.random.default_rng(i)
        rows = _rows(MIXED, i)
        c = _counts(rows, rows, MIXED_COLS)
        a = np.array([r.size for r in rows], dtype=np.int64)
        s = _storm(rows)
        try:
            _matrix_families(s, c, a, MIXED_BITS, rng)
        finally:
            s.free()
    return run_loop(cycle, "STORM_t, matrix calls only")


def test_storm_matrix_calls_only_in_a_process_of_its_own():
    _run_child("matrix_calls_only")


# ------------------------------------------------------------------------------------------ 2. totals first
def test_storm_totals_first_then_a_matrix():
    probe = _probe_expected(_rows(MIXED, 0))
    assert probe

    def cycle(i):
        rng = np.random.default_rng(i)
        rows = _rows(MIXED, i, salt=2)
        c = _counts(rows, rows, MIXED_COLS)
        a = np.array([r.size for r in rows], dtype=np.int64)
        s = _storm(rows)
        try:
            assert s.pairw_intersect_cardinality() == int(c[_upper(len(rows))].sum())      # the arena takes the stage
            assert bool(_last_pass() & RAN_PROBE) == probe
            _matrix_families(s, c, a, MIXED_BITS, rng)
        finally:
            s.free()
    run_loop(cycle, "STORM_t, totals first")


# ------------------------------------------------------------------------------------------ 3. list-only through K5
LISTS = _shape(300, ((0, 16384, 300, 700),), seed=3)
LISTS_COLS = _cols(LISTS)


def test_list_only_storm_through_the_row_lists():
    def cycle(i):
        rng = np.random.default_rng(i)
        rows = _rows(LISTS, i, salt=3)
        n = len(rows)
        c = _counts(rows, rows, LISTS_COLS)
        a = np.array([r.size for r in rows], dtype=np.int64)
        up = _upper(n)
        s = _storm(rows)
        try:
            _set("matrix_lists", 1)
            assert np.array_equal(s.pairw_matrix("and").astype(np.int64), np.where(up, c, 0))
            assert _last_pass() == RAN_LISTS_MATRIX
            want, nan = expected("jaccard", c, a, a, BLOCK, rng)
            got = s.pairw_similarity("jaccard", n_bits=BLOCK)
            assert _last_pass() == RAN_LISTS_MATRIX | RAN_SIMILARITY
            check(got.view(np.uint32), want, nan, up, "jaccard from the lists")
        finally:
            s.free()
    run_loop(cycle, "STORM_t, list-only (K5)")


# ------------------------------------------------------------------------------------------ 4. two widths
SQUARE_A = _shape(140, ((0, 8192, 4500, 6000),), seed=4)                           # one block wide
SQUARE_B = _shape(75, ((0, 8192, 4500, 6000), (2, 4096, 5, 50)), seed=5)           # three blocks wide
SQUARE_COLS = _cols(SQUARE_A, SQUARE_B)


def test_two_storm_of_different_widths(dev_out):
    import torch

    def cycle(i):
        rng = np.random.default_rng(i)
        rows_a, rows_b = _rows(SQUARE_A, i, salt=4), _rows(SQUARE_B, i, salt=5)
        na, nb, M = len(rows_a), len(rows_b), 3 * BLOCK
        c = _counts(rows_a, rows_b, SQUARE_COLS)
        a = np.array([r.size for r in rows_a], dtype=np.int64)
        b = np.array([r.size for r in rows_b], dtype=np.int64)
        A, B = _storm(rows_a), _storm(rows_b)
        try:
            assert A.intersect_cardinality_square(B) == int(c.sum())
            assert _last_pass() == RAN_FP4_STRIPS
            assert np.array_equal(A.square_matrix(B, "and").astype(np.int64), c)
            assert _last_pass() == RAN_TILES_OUT
            dev_out.fill_(SENTINEL)
            torch.cuda.synchronize()
            B.square_matrix_device(A, dev_out.data_ptr(), dev_out.shape[0], dev_out.stride(0), "or")   # the widened side first
            assert _last_pass() == RAN_TILES_OUT
            full = dev_out.cpu().numpy()
            assert np.array_equal(full[:nb, :na].astype(np.int64), b[:, None] + a[None, :] - c.T)
            assert (full[nb:] == SENTINEL).all() and (full[:, na:] == SENTINEL).all()
            want, nan = expected("ld_d", c, a, b, M, rng)
            got = A.square_similarity(B, "ld_d", n_bits=M)
            assert _last_pass() == RAN_TILES_OUT | RAN_SIMILARITY
            check(got.view(np.uint32), want, nan, None, "square ld_d")
            assert_topk(A.square_topk(B, K, "count"), _topk_counts(c, K, False), "square topk")
            assert _last_pass() == RAN_TILES_OUT | RAN_TOPK
        finally:
            A.free()
            B.free()
    run_loop(cycle, "two STORM_t of different widths")


# ------------------------------------------------------------------------------------------ 5. one handle reused
def test_one_handle_filled_called_and_cleared():
    lib = sb.load()
    _block_fns(lib)
    victim, edit_round = 17, WARMUP + 6
    s = sb.Storm()

    def a_round(i):
        rng = np.random.default_rng(i)
        rows = _rows(MIXED, i, salt=5)
        for r in rows:
            assert s.add(r) == 1
        a = np.array([r.size for r in rows], dtype=np.int64)
        _matrix_families(s, _counts(rows, rows, MIXED_COLS), a, MIXED_BITS, rng)
        if i == edit_round:
            # the same block ids and the same count per block, other positions: only STORM_hip_invalidate tells the handle
            new = _rows([(b, span, sizes[victim:victim + 1]) for b, span, sizes in MIXED], 1000 + i, salt=5)[0]
            assert new.size == rows[victim].size and not np.array_equal(new, rows[victim])
            assert lib.STORM_bitmap_cont_clear(C.c_void_p(_row_ptr(s, victim))) == 1
            assert lib.STORM_bitmap_cont_add(C.c_void_p(_row_ptr(s, victim)), new.ctypes.data_as(C.c_void_p), new.size) == 1
            s.hip_invalidate()
            rows[victim] = new
            c = _counts(rows, rows, MIXED_COLS)
            assert np.array_equal(s.pairw_matrix("and").astype(np.int64), np.where(_upper(len(rows)), c, 0))
            assert _last_pass() == RAN_TILES_OUT
        assert s.clear() == 1 and s.n_rows == 0
    try:
        run_loop(a_round, "one STORM_t, filled, called and cleared")
    finally:
        s.free()


# ------------------------------------------------------------------------------------------ 6. STORM_contiguous_t
CONTIG_BITS = 8192
CONTIG = _shape(300, ((0, CONTIG_BITS, 2000, 4000),), seed=6)
CONTIG_SPARSE = _shape(300, ((0, CONTIG_BITS, 5, 30),), seed=7)        # every row below the scalar cutoff (8192 / 200 = 40)
CONTIG_COLS = _cols(CONTIG)


def _loop_contig():
    def cycle(i):
        for shape, sparse in ((CONTIG, False), (CONTIG_SPARSE, True)):
            rows = _rows(shape, i, salt=6 + sparse)
            n = len(rows)
            c = _counts(rows, rows, CONTIG_COLS)
            up = _upper(n)
            tri = np.where(up, c, 0)
            s = _contig(rows, CONTIG_BITS)
            try:
                assert s.pairw_intersect_cardinality() == int(tri.sum())
                ran = _last_pass()
                # all rows sparse: the private list mirror answers (K4); else the dense mirror on the matrix cores
                assert ran & RAN_PROBE if sparse else (ran & RAN_DENSE_TOTALS and not ran & RAN_PROBE), ran
                assert np.array_equal(s.pairw_matrix("and").astype(np.int64), tri)
                assert _last_pass() == RAN_TILES_OUT
                if not sparse:
                    assert np.array_equal(s.pairw_lag_matrix(LAG, "and").astype(np.int64), to_lag(tri, LAG))
                    assert _last_pass() == RAN_TILES_OUT
                    assert_topk(s.pairw_topk(K, "count"), _topk_counts(c, K, True), "contig topk")
                    assert _last_pass() == RAN_TILES_OUT | RAN_TOPK
            finally:
                s.free()
    return run_loop(cycle, "STORM_contiguous_t")


def test_contig_dense_and_below_the_scalar_cutoff():
    _loop_contig()


# ------------------------------------------------------------------------------------------ 7. STORM_dosage_t
def test_dosage_containers():
    n, n2, S = 200, 60, 500
    up = _upper(n)

    def cycle(i):
        rng = np.random.default_rng([7, i])
        G = rng.integers(0, 4, size=(n, S), dtype=np.uint8)
        G[5] = 1                                                  # a constant row: NaN against everybody
        G2 = rng.integers(0, 4, size=(n2, S), dtype=np.uint8)
        g, g2 = G.astype(np.int64), G2.astype(np.int64)
        P, s1, q = g @ g.T, g.sum(axis=1), (g * g).sum(axis=1)
        d, d2 = sb.StormDosage(S), sb.StormDosage(S)
        try:
            for r in G[:3]:
                d.add(r)
            d.add_packed(pack(G[3:]))
            d2.add_packed(pack(G2))
            assert np.array_equal(d.pairw_dot().astype(np.int64), np.where(up, P, 0))
            assert _last_pass() == RAN_TILES_OUT
            num, dd = S * P - s1[:, None] * s1[None, :], S * q - s1 * s1
            nan = (dd[:, None] == 0) | (dd[None, :] == 0)
            assert nan[5, 6] and int(nan[up].sum()) == n - 1
            r2 = num.astype(np.float64) ** 2 / np.where(nan, 1, dd[:, None] * dd[None, :]).astype(np.float64)
            _check_floats(d.pairw_corr("r2"), r2, nan, up, "corr r2")
            assert _last_pass() == RAN_TILES_OUT | RAN_SIMILARITY
            want, cnan, _ = complete_reference(G)
            _check_floats(d.pairw_corr_complete("r"), want[1], cnan, up, "corr_complete r")
            assert _last_pass() == RAN_TILES_OUT | RAN_SIMILARITY
            assert np.array_equal(d.pairw_nobs().astype(np.int64), np.where(up, complete_sums(G)[0], 0))
            assert _last_pass() & RAN_TILES_OUT
            assert np.array_equal(d.square_dot(d2).astype(np.int64), g @ g2.T)
            assert _last_pass() & RAN_TILES_OUT
        finally:
            d.free()
            d2.free()
    run_loop(cycle, "STORM_dosage_t")


# ------------------------------------------------------------------------------------------ 8. the C-ABI underneath
def _random_words(rng, n, n_words):
    return rng.integers(0, 1 << 63, size=(n, n_words), dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, size=(n, n_words), dtype=np.uint64)


def _bits_of(mat):
    return np.unpackbits(mat.view(np.uint8), axis=1, bitorder="little")


def _ran(ctx):
    out = (C.c_uint64 * 4)()
    assert sb.load().storm_hip_last_pass_report(ctx._h, out) == 0
    return int(out[0])


def _column_total(mat):
    """sum over the columns of C(ones, 2): the all-pairs total of a bit matrix"""
    ones = _bits_of(mat).sum(axis=0, dtype=np.int64)
    return int((ones * (ones - 1) // 2).sum())


def test_context_and_matrix_of_the_c_abi():
    """a context and a matrix per cycle; every work-list and scratch buffer of the context that a call can grow is grown,
    so closing the context is checked against the member list of storm_hip_ctx_s (storm_hip_ctx_destroy, release_mfma_state)"""
    small, big, keep, n_words = 512, 2304, 300, 16
    up = _upper(keep)

    def cycle(i):
        rng = np.random.default_rng([8, i])
        mat, panel = _random_words(rng, small, n_words), _random_words(rng, big, n_words)
        want = _column_total(mat)
        ctx = sb.HipContext(0)
        m = None
        try:
            m = ctx.matrix_from_host(mat)
            for operands, used in ((0, 5), (2, 2), (4, 4), (6, 6)):       # K2b, K2q, the FP4 shadow, the 512-row form
                ctx.set_option("k2_strip_operands", operands)
                assert m.pairw() == want and ctx.get_option("k2_operands_used") == used, (operands, used)
            ctx.set_option("k2_strip_operands", 0)
            ctx.set_option("k2_strip_rows", 128)
            assert m.pairw() == want and ctx.get_option("k2_strip_rows_used") == 128
            ctx.set_option("k2_strip_rows", 0)
            for variant, kernel in ((2, "pairw_dense_kernel"), (3, "pairw_fp4_kernel")):    # the segment table, the tile list
                ctx.set_option("variant", variant)
                assert m.pairw() == want and ctx.last_pass_report()["kernels"] == [kernel]
            ctx.set_option("variant", -1)
            m.resize(big)                                                 # beyond the allocation: the rows are kept
            assert m.pairw() == want
            assert m.pairw_upload(panel) == _column_total(panel)          # the panel lists and the copy stream
            assert ctx.last_pass_report()["kernels"] == ["strip16_bits_kernel"]
            m.resize(keep)                                                # and back: the rows given up are cleared
            bits = _bits_of(panel[:keep]).astype(np.float32)
            c = np.rint(bits @ bits.T).astype(np.int64)
            a = np.diag(c)
            assert np.array_equal(m.pairw_matrix("and").astype(np.int64), np.where(up, c, 0))
            assert _ran(ctx) == RAN_TILES_OUT
            xor = a[:, None] + a[None, :] - 2 * c
            assert np.array_equal(m.pairw_lag_matrix(LAG, "xor").astype(np.int64), to_lag(np.where(up, xor, 0), LAG))
            assert _ran(ctx) == RAN_TILES_OUT
            assert_topk(m.pairw_topk(K, "count"), _topk_counts(c, K, True), "matrix topk")
            assert _ran(ctx) == RAN_TILES_OUT | RAN_TOPK
            m.resize(big)                                                 # inside the allocation now: the rows gained are zero
            assert m.pairw() == int(c[up].sum())
        finally:
            if m is not None:
                m.close()
            ctx.close()
    run_loop(cycle, "HipContext and HipMatrix")


# ------------------------------------------------------------------------------------------ 9. STORM_hip_shutdown
def _loop_shutdown():
    """live containers across STORM_hip_shutdown: storm.h promises that the handles re-create their device copies"""
    lib = sb.load()
    rows_s, rows_c = _rows(MIXED, 9, salt=9), _rows(CONTIG, 9, salt=9)
    cs, cc = _counts(rows_s, rows_s, MIXED_COLS), _counts(rows_c, rows_c, CONTIG_COLS)
    up = _upper(300)
    tri_s, tri_c = np.where(up, cs, 0), np.where(up, cc, 0)
    s, c = _storm(rows_s), _contig(rows_c, CONTIG_BITS)

    def both(matrices):
        if matrices:
            assert np.array_equal(s.pairw_matrix("and").astype(np.int64), tri_s) and _last_pass() == RAN_TILES_OUT
            assert np.array_equal(c.pairw_matrix("and").astype(np.int64), tri_c) and _last_pass() == RAN_TILES_OUT
        else:
            assert s.pairw_intersect_cardinality() == int(tri_s.sum()) and _last_pass() & RAN_PROBE
            assert c.pairw_intersect_cardinality() == int(tri_c.sum()) and _last_pass() & RAN_DENSE_TOTALS

    def cycle(i):          # (the same calls in every cycle: what the handles hold at a reading must not alternate)
        both(True)
        both(False)
        assert lib.STORM_hip_shutdown() == 0
        both(False)
        both(True)
    try:
        return run_loop(cycle, "STORM_hip_shutdown under live containers")
    finally:
        s.free()
        c.free()


def test_shutdown_under_live_containers_in_a_process_of_its_own():
    _run_child("shutdown")


# ------------------------------------------------------------------------------------------ 10. refusals
def test_refused_calls_take_nothing():
    lib = sb.load()
    n, S, M = 120, 300, 2 * BLOCK
    shape = _shape(n, ((0, 8192, 4500, 6000), (1, 4096, 10, 900)), seed=10)
    cols = _cols(shape)
    rows = _rows(shape, 10, salt=10)
    dense_rows = [r[r < BLOCK] for r in rows]
    G = np.random.default_rng(10).integers(0, 3, size=(n, S), dtype=np.uint8)
    s, c, d = _storm(rows), _contig(dense_rows, BLOCK), sb.StormDosage(S)
    d.add_packed(pack(G))
    up = _upper(n)
    tri = np.where(up, _counts(rows, rows, cols), 0)
    tri_c = np.where(up, _counts(dense_rows, dense_rows, cols), 0)
    dot = np.where(up, G.astype(np.int64) @ G.astype(np.int64).T, 0)
    buf = np.full((n + 1, n + 1), SENTINEL, dtype=np.uint32)
    p = buf.ctypes.data_as(C.c_void_p)
    refused = [0]

    def good():
        assert np.array_equal(s.pairw_matrix("and").astype(np.int64), tri) and _last_pass() == RAN_TILES_OUT
        assert np.array_equal(c.pairw_matrix("and").astype(np.int64), tri_c) and _last_pass() == RAN_TILES_OUT
        assert np.array_equal(d.pairw_dot().astype(np.int64), dot) and _last_pass() == RAN_TILES_OUT

    def cycle(i):
        calls = []
        for h, pre in ((s._h, "STORM_"), (c._h, "STORM_contig_")):
            f = lambda name: getattr(lib, pre + name)
            calls += [(f("pairw_matrix")(h, 0, None, n, n), -2), (f("pairw_matrix")(h, 0, p, n - 1, n), -4),
                      (f("pairw_matrix")(h, 0, p, n, n - 1), -4),
                      (f("pairw_similarity")(h, 4, M, p, n, n), -3), (f("pairw_similarity")(h, 0, M, p, n, n - 1), -4),
                      (f("pairw_lag_matrix")(h, 0, 0, p, n, LAG), -3), (f("pairw_lag_matrix")(h, 0, LAG, None, n, LAG), -2),
                      (f("pairw_lag_matrix")(h, 0, LAG, p, n, LAG - 1), -4), (f("pairw_lag_similarity")(h, 4, M, LAG, p, n, LAG), -3),
                      (f("pairw_topk")(h, 0, M, 0, 0, p, p, n, 8), -3), (f("pairw_topk")(h, 0, M, K, 0, None, p, n, K), -2),
                      (f("pairw_topk")(h, 5, M, K, 0, p, p, n, K), -3), (f("pairw_topk")(h, 0, M, K, 100, p, p, n, K), -3),
                      (f("pairw_topk")(h, 0, M, K, 0, p, p, n, K - 1), -4)]
        calls += [(lib.STORM_pairw_similarity(s._h, 3, 0, p, n, n), -3),                     # a STORM_t declares no universe
                  (lib.STORM_square_matrix(s._h, s._h, 0, None, n, n), -2), (lib.STORM_square_matrix(s._h, s._h, 0, p, n - 1, n), -4),
                  (lib.STORM_dosage_pairw_dot(d._h, None, n, n), -2), (lib.STORM_dosage_pairw_dot(d._h, p, n, n - 1), -4),
                  (lib.STORM_dosage_pairw_corr(d._h, 2, p, n, n), -3), (lib.STORM_dosage_pairw_corr_complete(d._h, 0, p, n - 1, n), -4)]
        for k, (rc, want) in enumerate(calls):
            assert rc == want, (i, k, rc, want)
        assert (buf == SENTINEL).all()                                                       # nothing written by any of them
        refused[0] += len(calls)
    try:
        good()
        run_loop(cycle, "refused calls")
        assert refused[0] >= 200
        good()
    finally:
        s.free()
        c.free()
        d.free()


# ------------------------------------------------------------------------------------------ the child processes
CHILD_LOOPS = {"matrix_calls_only": _loop_matrix_calls_only, "shutdown": _loop_shutdown}


def _child(name):
    """what a child process runs: one loop, with torch's context made before the first reading"""
    _torch_ready()
    CHILD_LOOPS[name]()
    print(f"child {name}: ok")


def _run_child(name, limit=240):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + \
        ["-c", f"import tests.test_gpu_lifecycle as t; t._child({name!r})"]
    try:
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=limit)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"the child process of loop {name} hung ({e}): nothing more is started on this device", returncode=3)
    print(r.stdout[-4000:])
    if r.returncode < 0 or r.returncode in (134, 139):      # a signal: the device may be in a bad way
        pytest.exit(f"the child process of loop {name} died with {r.returncode}: {r.stderr[-2000:]}", returncode=3)
    assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert f"child {name}: ok" in r.stdout
