"""The lag layout on the device: per-pair counts and similarity statistics for the row pairs i < j with j - i <= max_lag,
pair (i, j) at out[i * ld + (j - i - 1)] of an n x L matrix, L = min(max_lag, n - 1) (storm_hip_pairw_lag_matrix*,
storm_hip_pairw_lag_similarity*, storm_hip_similarity_finish_lag_device and the storm.h forms above them).

Expected counts come from two sources that share no code with the path under test: the CPU oracle (tile_counts_op on
dense rows, OrcStorm.pair_counts on STORM_t rows) and the library's own full triangle (storm_hip_pairw_matrix /
_pairw_similarity, other kernels' epilogues and finish pass), both gathered into the lag layout in numpy (`to_lag`).
Counts must be equal; similarity floats must be bit-identical to the gathered triangle and within the 1-ulp / exact-NaN
rule of tests/test_gpu_similarity.py (its `expected` generator is imported). Device outputs are pre-filled with a
sentinel, and every entry outside the layout — the lower-right corner, the pitch columns, rows beyond the band — must
still hold it."""
import ctypes as C

import numpy as np
import pytest

import stormbitmaps_amd as sb
from stormbitmaps_amd import dist
from tests.test_gpu_similarity import MEASURES, NAN_BITS, check, expected

pytestmark = pytest.mark.gpu

OPS = ("and", "or", "xor")
RAN_LISTS_MATRIX, RAN_TILES_OUT, RAN_SIMILARITY = 64, 128, 512
SENTINEL = 0xDEADBEEF
SENTINEL_I32 = int(np.uint32(SENTINEL).view(np.int32))
ALL = (1 << 64) - 1


# ------------------------------------------------------------------------------------------ helpers
def lag_of(n, max_lag):
    return min(max_lag, max(n - 1, 0))


def lag_mask(n, L, row0=0, rows=None):
    """[rows, L] bool: entry (r, d) is the pair (row0 + r, row0 + r + 1 + d) of an n-row matrix"""
    rows = n - row0 if rows is None else rows
    return (row0 + np.arange(rows)[:, None] + 1 + np.arange(L)[None, :]) < n


def to_lag(tri, L, row0=0, rows=None, fill=0):
    """the n x n matrix `tri` (entries i < j) in the lag layout of the band [row0, row0 + rows): [rows, L], `fill` in the
    corner"""
    n = tri.shape[0]
    rows = n - row0 if rows is None else rows
    ok = lag_mask(n, L, row0, rows)
    i = np.broadcast_to(row0 + np.arange(rows)[:, None], ok.shape)
    j = i + 1 + np.arange(L)[None, :]
    out = np.full((rows, L), fill, dtype=tri.dtype)
    out[ok] = tri[i[ok], j[ok]]
    return out


def random_bits(rng, n, n_bits):
    """n rows of n_bits bits, density 0.5, as uint64 words (the bits beyond n_bits are zero)"""
    n_words = (n_bits + 63) // 64
    mat = rng.integers(0, 1 << 63, size=(n, n_words), dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, size=(n, n_words), dtype=np.uint64)
    if n_bits % 64:
        mat[:, -1] &= np.uint64((1 << (n_bits % 64)) - 1)
    return mat


def oracle_triangles(orc, mat):
    n = mat.shape[0]
    return {op: np.triu(orc.tile_counts_op(mat, 0, n, 0, n, k), 1).astype(np.uint32) for k, op in enumerate(OPS)}


def device_buffer(rows, ld, off=0):
    """a sentinel-filled int32 device tensor of `rows` x ld entries whose base is `off` words behind a 16-byte boundary"""
    import torch
    flat = torch.full((off + max(rows * ld, 1),), SENTINEL_I32, dtype=torch.int32, device="cuda:0")
    view = flat[off:]
    assert view.data_ptr() % 16 == (4 * off) % 16
    return flat, view


def read_back(view, rows, ld):
    return view.cpu().numpy().view(np.uint32)[:rows * ld].reshape(rows, ld)


def device_lag(m, max_lag, op="and", ld=None, off=0, row0=0, rows=None):
    """storm_hip_pairw_lag_matrix_device into a sentinel-filled buffer: ([rows, L] counts, corner = SENTINEL), after
    asserting that nothing outside the layout was written"""
    n = m.n_rows
    L = lag_of(n, max_lag)
    ld = L if ld is None else ld
    n_band = n - row0 if rows is None else rows
    flat, view = device_buffer(n_band + 1, ld, off)      # one row more than the band: it must stay untouched
    m.pairw_lag_matrix_device(view.data_ptr(), ld, max_lag, op, row0, rows)
    got = read_back(view, n_band + 1, ld)
    inside = np.zeros(got.shape, dtype=bool)
    inside[:n_band, :L] = lag_mask(n, L, row0, n_band)
    assert (got[~inside] == SENTINEL).all(), (n, max_lag, ld, off, row0, np.argwhere(~inside & (got != SENTINEL))[:5].tolist())
    if off:
        assert (flat[:off].cpu().numpy().view(np.uint32) == SENTINEL).all()
    return got[:n_band, :L]


def report(ctx):
    out = (C.c_uint64 * 4)()
    assert sb.load().storm_hip_last_pass_report(ctx._h, out) == 0
    return list(out)


def pairs_within(n, L, row0=0, rows=None):
    return int(lag_mask(n, L, row0, rows).sum())


@pytest.fixture(scope="module")
def hip_ctx():
    ctx = sb.HipContext(0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def orc():
    from tests._orc import Oracle
    return Oracle()


# ------------------------------------------------------------------------------------------ 1. lags at every block edge
@pytest.fixture(scope="module")
def edge300(hip_ctx, orc):
    """300 rows x 1000 bits, density 0.5: the matrix, the oracle's triangles and the library's own, computed once"""
    mat = random_bits(np.random.default_rng(300), 300, 1000)
    m = hip_ctx.matrix_from_host(mat)
    want = oracle_triangles(orc, mat)
    for op in OPS:
        assert np.array_equal(m.pairw_matrix(op), want[op]), op       # the second source says the same
    yield m, want
    m.close()


@pytest.mark.parametrize("max_lag", [1, 63, 64, 65, 127, 128, 129, 299, 1000])
def test_lags_at_the_block_and_tile_edges(edge300, max_lag):
    """lags at every 32 / 64 / 128 block edge, the ragged last tile (300 = 2 x 128 + 44), the clipped L (1000 -> 299);
    tight and padded pitch; base aligned to 16 bytes and 4 bytes off it"""
    m, want = edge300
    L = lag_of(300, max_lag)
    assert L == min(max_lag, 299)
    ref = to_lag(want["and"], L, fill=SENTINEL)
    for ld in (L, L + 3):
        for off in (0, 1):
            got = device_lag(m, max_lag, "and", ld, off)
            assert np.array_equal(got, ref), (max_lag, ld, off, np.argwhere(got != ref)[:5].tolist())
    host = m.pairw_lag_matrix(max_lag, "xor")
    assert host.shape == (300, L) and np.array_equal(host, to_lag(want["xor"], L))     # 0 in the corner


# ------------------------------------------------------------------------------------------ 2. tiles with one wanted pair
def test_tiles_that_hold_a_single_wanted_pair(hip_ctx, orc):
    """257 rows, lag 1: tiles (0, 1) and (1, 2) hold exactly one wanted pair each — (127, 128) and (255, 256) — so three
    of their four waves take the block skip and the fourth stores one element of 4096"""
    plan = dist.lag_plan(257, 16, 1)
    assert {(int(i), int(j)) for i, j in plan[:, :2]} == {(0, 0), (0, 1), (1, 1), (1, 2), (2, 2)}
    mat = random_bits(np.random.default_rng(257), 257, 1000)
    want = oracle_triangles(orc, mat)
    m = hip_ctx.matrix_from_host(mat)
    try:
        for op in OPS:
            got = device_lag(m, 1, op, ld=1)
            assert np.array_equal(got, to_lag(want[op], 1, fill=SENTINEL)), op
            got = device_lag(m, 1, op, ld=4, off=1)
            assert np.array_equal(got, to_lag(want[op], 1, fill=SENTINEL)), op
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ 3. k-parts and their tickets
def test_k_parts_meet_through_the_ticket_path(hip_ctx, orc):
    """200 rows x 65536 bits, lag 40: three tiles on a whole chip, so every tile is cut along k and its parts' sums meet
    inside the launch — through windows of 16-bit counts and, with k2_part_narrow = 0, of 32-bit counts. The second call of
    each pair finds the tickets the first one must have reset."""
    n, n_words, max_lag = 200, 1024, 40
    plan = dist.lag_plan(n, n_words, max_lag, n_cus=hip_ctx.get_option("n_cus"))
    assert {(int(i), int(j)) for i, j in plan[:, :2]} == {(0, 0), (0, 1), (1, 1)}
    assert (plan[:, 6] > 1).any(), "no tile is cut along k: the case would not reach the ticket path"
    mat = random_bits(np.random.default_rng(200), n, 65536)
    want = oracle_triangles(orc, mat)
    m = hip_ctx.matrix_from_host(mat)
    try:
        assert np.array_equal(m.pairw_matrix("and"), want["and"])
        for narrow in (1, 0):
            hip_ctx.set_option("k2_part_narrow", narrow)
            for op in ("and", "xor"):
                for rep in range(2):
                    got = device_lag(m, max_lag, op, ld=max_lag + 3)
                    ref = to_lag(want[op], max_lag, fill=SENTINEL)
                    assert np.array_equal(got, ref), (narrow, op, rep, np.argwhere(got != ref)[:5].tolist())
    finally:
        hip_ctx.set_option("k2_part_narrow", 1)
        m.close()


# ------------------------------------------------------------------------------------------ 4. row bands
def test_row_bands_concatenate_to_the_whole(hip_ctx, orc):
    """700 rows, lag 200, bands [0, 257) and [257, 700) into buffers of their own: the band edge is no multiple of 128, so
    tile row 2 is multiplied by both calls and each writes only its own rows"""
    n, max_lag = 700, 200
    mat = random_bits(np.random.default_rng(700), n, 1000)
    want = oracle_triangles(orc, mat)
    m = hip_ctx.matrix_from_host(mat)
    try:
        for op in ("and", "or"):
            whole = device_lag(m, max_lag, op, ld=max_lag)
            assert np.array_equal(whole, to_lag(want[op], max_lag, fill=SENTINEL)), op
            top = device_lag(m, max_lag, op, ld=max_lag + 1, row0=0, rows=257)
            bottom = device_lag(m, max_lag, op, ld=max_lag, off=1, row0=257, rows=443)
            assert np.array_equal(np.concatenate([top, bottom]), whole), op
        assert report(hip_ctx)[:2] == [RAN_TILES_OUT, pairs_within(n, max_lag, 257, 443) * mat.shape[1]]
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ 5. many tile rows
def test_many_tile_rows(hip_ctx, orc):
    """1500 rows x 2048 bits, lag 70: twelve tile rows of two tiles each, whole rounds of whole tiles"""
    n, max_lag = 1500, 70
    mat = random_bits(np.random.default_rng(1500), n, 2048)
    want = oracle_triangles(orc, mat)
    m = hip_ctx.matrix_from_host(mat)
    try:
        assert np.array_equal(m.pairw_matrix("and"), want["and"])
        for op in OPS:
            got = device_lag(m, max_lag, op, ld=max_lag + 2)
            ref = to_lag(want[op], max_lag, fill=SENTINEL)
            assert np.array_equal(got, ref), (op, np.argwhere(got != ref)[:5].tolist())
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ 6. similarity
@pytest.fixture(scope="module")
def sim300(hip_ctx, orc):
    """300 rows x 1000 bits with an empty row (17) and a full row (140): counts, row counts, and per measure the expected
    floats with their NaN mask over the whole triangle — computed once, gathered per case"""
    rng = np.random.default_rng(1300)
    M = 1000
    mat = random_bits(rng, 300, M)
    mat[17] = 0
    mat[140] = np.uint64((1 << 64) - 1)
    mat[140, -1] = np.uint64((1 << (M % 64)) - 1)
    c = np.triu(orc.tile_counts_op(mat, 0, 300, 0, 300, 0), 1).astype(np.int64)
    a = np.array([bin(int.from_bytes(r.tobytes(), "little")).count("1") for r in mat], dtype=np.int64)
    assert a[17] == 0 and a[140] == M
    m = hip_ctx.matrix_from_host(mat)
    assert np.array_equal(m.row_counts().astype(np.int64), a) and np.array_equal(m.pairw_matrix("and").astype(np.int64), c)
    want = {ms: expected(ms, c, a, a, M, rng) for ms in MEASURES}
    yield m, c, a, M, want
    m.close()


def _triangle_similarity_bits(hip_ctx, m, measure, M):
    """storm_hip_pairw_similarity (host form): the other finish kernel on the other count layout"""
    n = m.n_rows
    out = np.zeros((n, n), dtype=np.float32)
    rc = sb.load().storm_hip_pairw_similarity(hip_ctx._h, m._h, MEASURES.index(measure), M, out.ctypes.data_as(C.c_void_p), n)
    assert rc == 0, sb._lib.last_error()
    return out.view(np.uint32)


@pytest.mark.parametrize("measure", MEASURES)
def test_similarity_device_and_host_forms(hip_ctx, sim300, measure):
    m, c, a, M, want = sim300
    n, max_lag = 300, 129
    L = max_lag
    inside = lag_mask(n, L)
    values, nan = want[measure]
    values_lag, nan_lag = to_lag(values, L), to_lag(nan, L, fill=False)
    # the NaN pattern exactly where the measure is undefined: pairs with the empty row (cosine, r^2) or the full one (r^2)
    undefined = {"jaccard": set(), "cosine": {17}, "ld_d": set(), "ld_r2": {17, 140}}[measure]
    i = np.broadcast_to(np.arange(n)[:, None], inside.shape)
    j = i + 1 + np.arange(L)[None, :]
    assert np.array_equal(nan_lag, inside & (np.isin(i, list(undefined)) | np.isin(j, list(undefined)))), measure
    tri_bits = to_lag(_triangle_similarity_bits(hip_ctx, m, measure, M), L)
    # host form: +0.0f in the corner
    host = m.pairw_lag_similarity(max_lag, measure, M)
    assert host.dtype == np.float32 and host.shape == (n, L)
    bits = host.view(np.uint32)
    assert (bits[~inside] == 0).all()
    assert np.array_equal(bits[inside], tri_bits[inside]), measure                       # bit-identical to the triangle path
    assert (bits[nan_lag] == NAN_BITS).all()
    check(bits, values_lag, nan_lag, inside, (measure, "host"))
    assert report(hip_ctx)[0] == RAN_TILES_OUT | RAN_SIMILARITY
    # device form, padded pitch, aligned and misaligned base
    for ld, off in ((L + 3, 0), (L + 3, 1), (L + 7, 0)):
        flat, view = device_buffer(n + 1, ld, off)
        m.pairw_lag_similarity_device(view.data_ptr(), ld, max_lag, measure, M)
        got = read_back(view, n + 1, ld)
        conv = np.zeros(got.shape, dtype=bool)
        conv[:n, :L] = inside
        assert (got[~conv] == SENTINEL).all(), (measure, ld, off)
        assert np.array_equal(got[:n, :L][inside], tri_bits[inside]), (measure, ld, off)
        check(got[:n, :L], values_lag, nan_lag, inside, (measure, "device", ld, off))
        assert report(hip_ctx)[:2] == [RAN_TILES_OUT | RAN_SIMILARITY, pairs_within(n, L) * m.n_words]


@pytest.mark.parametrize("measure", MEASURES)
def test_finish_pass_alone_on_a_count_matrix_of_the_callers(hip_ctx, sim300, measure):
    """storm_hip_similarity_finish_lag_device on counts the test lays out itself: whole matrix and a band that starts and
    ends inside a 64-row tile; tight, vector-friendly and odd pitch; aligned and misaligned base"""
    import torch
    m, c, a, M, want = sim300
    n = 300
    values, nan = want[measure]
    d_counts = torch.from_numpy(a.astype(np.uint32).view(np.int32)).to("cuda:0")
    tri_bits = _triangle_similarity_bits(hip_ctx, m, measure, M)
    for max_lag, ld, off, row0, rows in ((129, 129, 0, 0, n), (129, 132, 0, 0, n), (129, 132, 1, 0, n), (260, 260, 0, 0, n),
                                         (1000, 300, 0, 0, n), (64, 64, 0, 70, 131), (300, 304, 0, 257, 43)):
        L = lag_of(n, max_lag)
        inside = lag_mask(n, L, row0, rows)
        host = np.full((rows + 1, ld), SENTINEL, dtype=np.uint32)
        host[:rows, :L] = to_lag(c.astype(np.uint32), L, row0, rows, fill=SENTINEL)
        flat, view = device_buffer(rows + 1, ld, off)
        view.copy_(torch.from_numpy(host.view(np.int32).reshape(-1)).to("cuda:0"))
        torch.cuda.synchronize()
        m.similarity_finish_lag_device(view.data_ptr(), ld, max_lag, d_counts.data_ptr(), measure, M, row0, rows)
        hip_ctx.synchronize()
        assert report(hip_ctx) == [RAN_SIMILARITY, 0, 0, 0]
        got = read_back(view, rows + 1, ld)
        conv = np.zeros(got.shape, dtype=bool)
        conv[:rows, :L] = inside
        assert (got[~conv] == SENTINEL).all(), (measure, max_lag, ld, off, row0)
        assert np.array_equal(got[:rows, :L][inside], to_lag(tri_bits, L, row0, rows)[inside]), (measure, max_lag, ld, off, row0)
        check(got[:rows, :L], to_lag(values, L, row0, rows), to_lag(nan, L, row0, rows, fill=False), inside,
              (measure, max_lag, ld, off, row0))


def test_shim_refusals_and_empty_shapes(hip_ctx, edge300):
    import torch
    lib = sb.load()
    m, _ = edge300
    t = torch.full((300 * 16,), 3, dtype=torch.int32, device="cuda:0")
    cnt = torch.full((300,), 5, dtype=torch.int32, device="cuda:0")
    p, q, h, mh = C.c_void_p(t.data_ptr()), C.c_void_p(cnt.data_ptr()), hip_ctx._h, m._h
    f = lib.storm_hip_pairw_lag_matrix_device
    for args in ((None, 0, 5, 0, ALL, p, 5), (mh, 0, 5, 0, ALL, None, 5), (mh, 3, 5, 0, ALL, p, 5), (mh, -1, 5, 0, ALL, p, 5),
                 (mh, 0, 0, 0, ALL, p, 5), (mh, 0, 5, 0, ALL, p, 4), (mh, 0, 1000, 0, ALL, p, 298), (mh, 0, 5, 301, 0, p, 5),
                 (mh, 0, 5, 200, 101, p, 5)):
        assert f(h, *args) == -1, args
        assert sb._lib.last_error()
    assert f(h, mh, 0, 5, 300, 0, p, 5) == 0 and f(h, mh, 0, 5, 10, 0, p, 5) == 0       # empty bands
    host = np.full(16, 3, dtype=np.uint32)
    hp = host.ctypes.data_as(C.c_void_p)
    assert lib.storm_hip_pairw_lag_matrix(h, mh, 0, 0, hp, 5) == -1 and lib.storm_hip_pairw_lag_matrix(h, mh, 0, 5, hp, 4) == -1
    assert lib.storm_hip_pairw_lag_matrix(h, mh, 4, 5, hp, 5) == -1
    g = lib.storm_hip_similarity_finish_lag_device
    for args in ((None, 5, 300, 0, ALL, 5, q, 0, 64), (p, 5, 300, 0, ALL, 5, None, 0, 64), (p, 5, 300, 0, ALL, 5, q, 4, 64),
                 (p, 5, 300, 0, ALL, 5, q, 0, 0), (p, 5, 300, 0, ALL, 5, q, 0, (1 << 32) + 1), (p, 4, 300, 0, ALL, 5, q, 0, 64),
                 (p, 5, 300, 0, ALL, 0, q, 0, 64), (p, 5, 300, 301, 0, 5, q, 0, 64), (p, 5, 300, 200, 101, 5, q, 0, 64)):
        assert g(h, *args) == -1, args
    for s in (lib.storm_hip_pairw_lag_similarity_device, lib.storm_hip_pairw_lag_similarity):
        buf = p if s is lib.storm_hip_pairw_lag_similarity_device else hp
        assert s(h, mh, 4, 64, 5, buf, 5) == -1 and s(h, mh, 0, 0, 5, buf, 5) == -1 and s(h, mh, 0, 64, 0, buf, 5) == -1
        assert s(h, mh, 0, 64, 5, buf, 4) == -1 and s(h, None, 0, 64, 5, buf, 5) == -1 and s(h, mh, 0, 64, 5, None, 5) == -1
    before = report(hip_ctx)
    assert g(h, p, 5, 300, 300, 0, 5, q, 0, 64) == 0 and g(h, p, 5, 1, 0, ALL, 5, q, 0, 64) == 0
    assert report(hip_ctx) == before
    one = hip_ctx.matrix_from_host(random_bits(np.random.default_rng(1), 1, 1000))
    try:
        assert f(h, one._h, 0, 5, 0, ALL, p, 0) == 0 and lib.storm_hip_pairw_lag_matrix(h, one._h, 0, 5, hp, 0) == 0
        assert lib.storm_hip_pairw_lag_similarity_device(h, one._h, 0, 64, 5, p, 0) == 0
        assert lib.storm_hip_pairw_lag_similarity(h, one._h, 0, 64, 5, hp, 0) == 0
    finally:
        one.close()
    hip_ctx.synchronize()
    assert (t.cpu().numpy() == 3).all() and (host == 3).all()


# ------------------------------------------------------------------------------------------ 7. the storm.h forms
def _last_pass():
    out = (C.c_uint64 * 4)()
    assert sb.load().STORM_hip_last_pass(out) == 0
    return int(out[0])


def _positions_of(mat):
    return [np.flatnonzero(np.unpackbits(r.view(np.uint8), bitorder="little")).astype(np.uint32) for r in mat]


def _ops_from_and(c, a):
    s = (a[:, None] + a[None, :]).astype(np.int64)
    return {"and": c, "or": np.triu(s - c, 1), "xor": np.triu(s - 2 * c, 1)}


def _check_container(s, want, a, M, rng, max_lags):
    """every lag form of a storm.h container against triangles `want` (per op) and row counts a"""
    n = s.n_rows
    exp = {measure: expected(measure, want["and"], a, a, M, rng) for measure in MEASURES}
    tris = {measure: s.pairw_similarity(measure, n_bits=M).view(np.uint32) for measure in MEASURES}   # the triangle path
    for max_lag in max_lags:
        L = lag_of(n, max_lag)
        inside = lag_mask(n, L)
        for op in OPS:
            host = s.pairw_lag_matrix(max_lag, op)
            assert host.shape == (n, L) and np.array_equal(host.astype(np.int64), to_lag(want[op], L)), (max_lag, op)
            assert _last_pass() == RAN_TILES_OUT
            flat, view = device_buffer(n + 2, L + 5)
            s.pairw_lag_matrix_device(view.data_ptr(), n + 2, L + 5, max_lag, op)
            got = read_back(view, n + 2, L + 5)
            conv = np.zeros(got.shape, dtype=bool)
            conv[:n, :L] = inside
            assert (got[~conv] == SENTINEL).all(), (max_lag, op)
            assert np.array_equal(got[:n, :L][inside].astype(np.int64), to_lag(want[op], L)[inside]), (max_lag, op)
        for measure in MEASURES:
            (values, nan), tri = exp[measure], tris[measure]
            host = s.pairw_lag_similarity(max_lag, measure, n_bits=M)
            assert _last_pass() == RAN_TILES_OUT | RAN_SIMILARITY
            bits = host.view(np.uint32)
            assert (bits[~inside] == 0).all() and np.array_equal(bits[inside], to_lag(tri, L)[inside]), (max_lag, measure)
            check(bits, to_lag(values, L), to_lag(nan, L, fill=False), inside, (max_lag, measure, "host"))
            flat, view = device_buffer(n, L + 1, 1)
            s.pairw_lag_similarity_device(view.data_ptr(), n, L + 1, max_lag, measure, n_bits=M)
            got = read_back(view, n, L + 1)
            conv = np.zeros(got.shape, dtype=bool)
            conv[:, :L] = inside
            assert (got[~conv] == SENTINEL).all(), (max_lag, measure)
            assert np.array_equal(got[:, :L][inside], to_lag(tri, L)[inside]), (max_lag, measure)


def test_contig_container(orc):
    rng = np.random.default_rng(71)
    n, M = 260, 1000
    mat = random_bits(rng, n, M)
    c = np.triu(orc.tile_counts_op(mat, 0, n, 0, n, 0), 1).astype(np.int64)
    rows = _positions_of(mat)
    a = np.array([r.size for r in rows], dtype=np.int64)
    want = _ops_from_and(c, a)
    for k, op in enumerate(OPS):
        assert np.array_equal(want[op], np.triu(orc.tile_counts_op(mat, 0, n, 0, n, k), 1))
    s = sb.StormContig(M)
    try:
        for r in rows:
            assert s.add(r) == r.size
        assert np.array_equal(s.pairw_matrix("and").astype(np.int64), c)
        _check_container(s, want, a, M, rng, (1, 130, 5000))
        # n_bits 0: the container's vector_length
        assert np.array_equal(s.pairw_lag_similarity(7, "ld_r2").view(np.uint32), s.pairw_lag_similarity(7, "ld_r2", n_bits=M).view(np.uint32))
    finally:
        s.free()


def _storm(rows):
    s = sb.Storm()
    for r in rows:
        assert s.add(np.ascontiguousarray(r, dtype=np.uint32)) == 1
    return s


def _sparse_rows(rng, n, M, lo, hi):
    return [np.sort(rng.choice(M, size=k, replace=False)).astype(np.uint32) for k in rng.integers(lo, hi + 1, size=n)]


def test_storm_with_list_and_bitmap_blocks(orc):
    """rows of a bitmap block (thousands of positions below 65536) and a list block (a few beyond it): two block columns"""
    rng = np.random.default_rng(72)
    n, M = 200, 2 * 65536
    rows = [np.concatenate([r, 65536 + q]) for r, q in zip(_sparse_rows(rng, n, 65536, 4500, 20000),
                                                           _sparse_rows(rng, n, 65536, 10, 900))]
    c = orc.storm(rows).pair_counts().astype(np.int64)
    a = np.array([r.size for r in rows], dtype=np.int64)
    s = _storm(rows)
    try:
        assert np.array_equal(s.pairw_matrix("and").astype(np.int64), c)
        _check_container(s, _ops_from_and(c, a), a, M, rng, (3, 150))
    finally:
        s.free()


def test_list_only_storm_runs_on_its_dense_replica(orc):
    """a list-only container that STORM_pairw_matrix joins from its row lists (K5): the lag forms build the dense replica
    and still give the right matrix; the triangle calls between them keep running from the lists"""
    rng = np.random.default_rng(73)
    n, M = 300, 65536
    rows = _sparse_rows(rng, n, M, 300, 700)
    c = orc.storm(rows).pair_counts().astype(np.int64)
    a = np.array([r.size for r in rows], dtype=np.int64)
    s = _storm(rows)
    try:
        assert sb.load().STORM_hip_set_option(b"matrix_lists", 1) == 0
        assert np.array_equal(s.pairw_matrix("and").astype(np.int64), c) and _last_pass() == RAN_LISTS_MATRIX
        _check_container(s, _ops_from_and(c, a), a, M, rng, (129,))
        assert np.array_equal(s.pairw_matrix("and").astype(np.int64), c) and _last_pass() == RAN_LISTS_MATRIX
    finally:
        sb.load().STORM_hip_set_option(b"matrix_lists", -1)
        s.free()


def test_container_return_codes_and_empty_containers():
    lib = sb.load()
    rng = np.random.default_rng(74)
    n, M = 40, 1000
    rows = _positions_of(random_bits(rng, n, M))
    c, s = sb.StormContig(M), _storm(rows)
    e_c, e_s, one_c, one_s = sb.StormContig(M), sb.Storm(), sb.StormContig(M), _storm(rows[:1])
    try:
        for r in rows:
            assert c.add(r) == r.size
        assert one_c.add(rows[0]) == rows[0].size
        buf = np.full((n + 1, 16), SENTINEL, dtype=np.uint32)
        p = buf.ctypes.data_as(C.c_void_p)
        L = 10
        for cont, mat_f, sim_f in ((c, lib.STORM_contig_pairw_lag_matrix, lib.STORM_contig_pairw_lag_similarity),
                                   (c, lib.STORM_contig_pairw_lag_matrix_device, lib.STORM_contig_pairw_lag_similarity_device),
                                   (s, lib.STORM_pairw_lag_matrix, lib.STORM_pairw_lag_similarity),
                                   (s, lib.STORM_pairw_lag_matrix_device, lib.STORM_pairw_lag_similarity_device)):
            h = cont._h
            assert mat_f(None, 0, L, p, n, L) == -1 and sim_f(None, 0, M, L, p, n, L) == -1
            assert mat_f(h, 0, L, None, n, L) == -2 and sim_f(h, 0, M, L, None, n, L) == -2
            assert mat_f(h, 0, L, p, n, L - 1) == -4 and sim_f(h, 0, M, L, p, n, L - 1) == -4
            assert mat_f(h, 0, L, p, n - 1, L) == -4 and mat_f(h, 0, 1000, p, n, n - 2) == -4
            assert mat_f(h, 0, 0, p, n, L) == -3 and sim_f(h, 0, M, 0, p, n, L) == -3             # max_lag 0
            assert lib.STORM_hip_error()
            assert mat_f(h, 3, L, p, n, L) == -3 and mat_f(h, -1, L, p, n, L) == -3               # bad op
            assert sim_f(h, 4, M, L, p, n, L) == -3 and sim_f(h, -1, M, L, p, n, L) == -3         # bad measure
            assert sim_f(h, 3, (1 << 32) + 1, L, p, n, L) == -3
            if cont is s:
                assert sim_f(h, 3, 0, L, p, n, L) == -3 and sim_f(h, 2, 0, L, p, n, L) == -3      # a STORM_t declares no universe
        assert (buf == SENTINEL).all()
        for h, mat_f, sim_f in ((e_c._h, lib.STORM_contig_pairw_lag_matrix, lib.STORM_contig_pairw_lag_similarity),
                                (one_c._h, lib.STORM_contig_pairw_lag_matrix, lib.STORM_contig_pairw_lag_similarity),
                                (e_s._h, lib.STORM_pairw_lag_matrix, lib.STORM_pairw_lag_similarity),
                                (one_s._h, lib.STORM_pairw_lag_matrix, lib.STORM_pairw_lag_similarity)):
            assert mat_f(h, 0, 5, p, 1, 0) == 0 and sim_f(h, 0, M, 5, p, 1, 0) == 0
        assert (buf == SENTINEL).all()
        assert one_c.pairw_lag_matrix(5).shape == (1, 0) and e_s.pairw_lag_similarity(5, "jaccard").shape == (0, 0)
    finally:
        for x in (c, s, e_c, e_s, one_c, one_s):
            x.free()


# ------------------------------------------------------------------------------------------ 8. the last-pass report
def test_last_pass_report(hip_ctx, edge300):
    m, _ = edge300
    for max_lag, row0, rows in ((1, 0, None), (129, 0, None), (1000, 0, None), (64, 100, 150), (64, 280, 20)):
        L = lag_of(300, max_lag)
        device_lag(m, max_lag, "or", L, 0, row0, rows)
        assert hip_ctx.get_option("k2_tile_shape_used") == 6
        assert report(hip_ctx) == [RAN_TILES_OUT, pairs_within(300, L, row0, rows) * m.n_words, 0, 0], (max_lag, row0)
    assert pairs_within(300, 299) == 300 * 299 // 2
