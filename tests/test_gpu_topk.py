"""Per-row top-k neighbours selected on the device (storm_hip_topk_rows_device, storm_hip_pairw_topk*,
storm_hip_cross_dense_topk* and the storm.h forms above them): for each row the k best columns, value descending, then
column index ascending; NaN entries are no candidates; short rows are padded.

Expected values come from paths that share no code with topk_rows_kernel: counts from the CPU oracle (tile_counts_op on
dense rows, OrcStorm.pair_counts on STORM_t rows), float bits from the library's existing similarity calls
(storm_hip_pairw_similarity with the triangle mirrored in numpy, storm_hip_cross_dense_similarity, the storm.h
similarity forms, and storm_hip_similarity_finish_device for a caller's count matrix). numpy ranks them by the rule above
(`rank`); idx and val must be EQUAL to that, bit for bit, no tolerance. Device outputs are pre-filled with a sentinel:
columns [k, ld_k) and one row beyond the output must still hold it."""
import ctypes as C

import numpy as np
import pytest

import stormbitmaps_amd as sb
from tests.test_gpu_lag_matrix import (SENTINEL, _positions_of, _sparse_rows, _storm, device_buffer, random_bits, read_back,
                                       report)
from tests.test_gpu_similarity import MEASURES, NAN_BITS

pytestmark = pytest.mark.gpu

SCORES = MEASURES + ("count",)                      # 0 .. 3 the measures, 4 = STORM_HIP_TOPK_COUNT
RAN_TILES_OUT, RAN_TOPK = 128, 1024
NO_INDEX = 0xFFFFFFFF
ALL = (1 << 64) - 1
TOPK_MAX = 128
STAGING = 1920                                      # keys topk_rows_kernel stages between two sorts (kTopkStaging)


# ------------------------------------------------------------------------------------------ helpers
def rank(bits, score, skip0=None):
    """The whole order of every row of the value matrix `bits` (uint32: float bits, or counts for score "count"):
    (idx [n, m] uint32, val [n, m] uint32, candidates [n]) — value descending, then column ascending (a stable sort of
    the negated values), the non-candidates (NaN pattern; column skip0 + r of row r) replaced by padding at the end."""
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    n, m = bits.shape
    cand = np.ones((n, m), dtype=bool)
    if score != "count":
        cand &= bits != NAN_BITS
    if skip0 is not None:
        r = np.arange(n)
        j = skip0 + r
        cand[r[j < m], j[j < m]] = False
    value = bits.astype(np.float64) if score == "count" else bits.view(np.float32).astype(np.float64)
    assert np.isfinite(value[cand]).all()
    order = np.argsort(np.where(cand, -value, np.inf), axis=1, kind="stable")
    idx, val = order.astype(np.uint32), np.take_along_axis(bits, order, axis=1)
    n_cand = cand.sum(axis=1)
    pad = np.arange(m)[None, :] >= n_cand[:, None]
    idx[pad] = NO_INDEX
    val[pad] = 0 if score == "count" else NAN_BITS
    return idx, val, n_cand


def top(ranked, k, score):
    """columns [0, k) of a `rank` result, padded where the matrix has fewer than k columns"""
    idx, val, _ = ranked
    n, m = idx.shape
    if m < k:
        idx = np.concatenate([idx, np.full((n, k - m), NO_INDEX, dtype=np.uint32)], axis=1)
        val = np.concatenate([val, np.full((n, k - m), 0 if score == "count" else NAN_BITS, dtype=np.uint32)], axis=1)
    return idx[:, :k], val[:, :k]


def ties_across(ranked, k):
    """rows whose k-th and (k + 1)-th candidate have the same value: only the column index decides which is listed"""
    idx, val, n_cand = ranked
    if idx.shape[1] <= k:
        return 0
    return int(((n_cand > k) & (val[:, k - 1] == val[:, k])).sum())


def into_device(call, n, k, ld_k):
    """call(d_idx, d_val) into two sentinel-filled device buffers of n + 1 rows x ld_k: (idx, val) [n, k] after asserting
    that columns [k, ld_k) and the row beyond the output still hold the sentinel"""
    _, vi = device_buffer(n + 1, ld_k)
    _, vv = device_buffer(n + 1, ld_k)
    call(vi.data_ptr(), vv.data_ptr())
    gi, gv = read_back(vi, n + 1, ld_k), read_back(vv, n + 1, ld_k)
    for g in (gi, gv):
        assert (g[n:] == SENTINEL).all() and (g[:, k:] == SENTINEL).all()
    return gi[:n, :k].copy(), gv[:n, :k].copy()


def assert_topk(got, want, what):
    (gi, gv), (wi, wv) = got, want
    gv = np.ascontiguousarray(gv).view(np.uint32)
    bad = np.argwhere((gi != wi) | (gv != wv))
    assert bad.size == 0, (what, bad[:5].tolist(), gi[tuple(bad[0])], wi[tuple(bad[0])], hex(gv[tuple(bad[0])]), hex(wv[tuple(bad[0])]))


def triangle_bits(hip_ctx, m, measure, M):
    """storm_hip_pairw_similarity (host form) mirrored: the n x n float bits, 0 on the diagonal"""
    n = m.n_rows
    out = np.zeros((n, n), dtype=np.float32)
    assert sb.load().storm_hip_pairw_similarity(hip_ctx._h, m._h, MEASURES.index(measure), M, out.ctypes.data_as(C.c_void_p), n) == 0
    tri = np.triu(out.view(np.uint32), 1)
    return tri + tri.T


def cross_bits(hip_ctx, a, b, measure, M):
    out = np.zeros((a.n_rows, b.n_rows), dtype=np.float32)
    assert sb.load().storm_hip_cross_dense_similarity(hip_ctx._h, a._h, b._h, MEASURES.index(measure), M,
                                                      out.ctypes.data_as(C.c_void_p), b.n_rows) == 0
    return out.view(np.uint32)


def pairw_values(hip_ctx, orc, mat, m, M):
    """per score the n x n value matrix of one matrix's rows among themselves (the diagonal is never a candidate)"""
    n = mat.shape[0]
    values = {"count": orc.tile_counts_op(mat, 0, n, 0, n, 0)}
    for measure in MEASURES:
        values[measure] = triangle_bits(hip_ctx, m, measure, M)
    return values


def last_pass():
    out = (C.c_uint64 * 4)()
    assert sb.load().STORM_hip_last_pass(out) == 0
    return int(out[0])


# ------------------------------------------------------------------------------------------ 1. block edges and ties
@pytest.fixture(scope="module")
def edge300(hip_ctx, orc):
    """300 rows x 1000 bits, density 0.5 (two 128-row tiles and 44 rows; one sweep step of 300 columns): per score the
    whole expected order, computed once"""
    M = 1000
    mat = random_bits(np.random.default_rng(300), 300, M)
    m = hip_ctx.matrix_from_host(mat)
    values = pairw_values(hip_ctx, orc, mat, m, M)
    ranked = {score: rank(values[score], score, skip0=0) for score in SCORES}
    yield m, M, values, ranked
    m.close()


@pytest.mark.parametrize("k", [1, 8, 64, 128])
@pytest.mark.parametrize("score", SCORES)
def test_block_edges_and_ties(edge300, score, k):
    m, M, _, ranked = edge300
    if score in ("count", "jaccard"):
        # with this generator 36 / 138 / 263 / 274 rows (count) and 1 / 7 / 35 / 39 rows (Jaccard) tie across the boundary
        assert ties_across(ranked[score], k) >= 1, (score, k)
    want = top(ranked[score], k, score)
    assert (want[0] != NO_INDEX).all() and (want[0] != np.arange(300)[:, None]).all()
    for ld_k in (k, k + 3):
        got = into_device(lambda di, dv: m.pairw_topk_device(di, dv, ld_k, k, score, n_bits=M), 300, k, ld_k)
        assert_topk(got, want, (score, k, ld_k))
    idx, val = m.pairw_topk(k, score, n_bits=M)
    assert val.dtype == (np.uint32 if score == "count" else np.float32) and idx.shape == val.shape == (300, k)
    assert_topk((idx, val), want, (score, k, "host"))


# ------------------------------------------------------------------------------------------ 2. undefined entries
def test_undefined_entries_are_no_candidates(hip_ctx, orc):
    """the sim300 matrix of tests/test_gpu_lag_matrix.py: row 17 empty, row 140 full"""
    rng = np.random.default_rng(1300)
    M, n, k = 1000, 300, 8
    mat = random_bits(rng, n, M)
    mat[17] = 0
    mat[140] = np.uint64((1 << 64) - 1)
    mat[140, -1] = np.uint64((1 << (M % 64)) - 1)
    m = hip_ctx.matrix_from_host(mat)
    try:
        values = pairw_values(hip_ctx, orc, mat, m, M)
        others = np.setdiff1d(np.arange(n), [17, 140])
        for score in SCORES:
            want = top(rank(values[score], score, skip0=0), k, score)
            got = into_device(lambda di, dv: m.pairw_topk_device(di, dv, k + 1, k, score, n_bits=M), n, k, k + 1)
            assert_topk(got, want, score)
            idx, val = got
            undefined = {"jaccard": [], "cosine": [17], "ld_d": [], "ld_r2": [17, 140], "count": []}[score]
            for r in undefined:                                   # all padding, and listed nowhere
                assert (idx[r] == NO_INDEX).all() and (val[r] == NAN_BITS).all(), (score, r)
                assert not (idx == r).any(), (score, r)
            for r in set((17, 140)) - set(undefined):              # listed normally: k real neighbours
                assert (idx[r] != NO_INDEX).all() and (val[r] != NAN_BITS).all(), (score, r)
            assert (idx[others] != NO_INDEX).all() and (val[others] != NAN_BITS).all(), score
        # the full row is every other row's superset: under the count it is a best neighbour of every non-empty row
        idx, _ = into_device(lambda di, dv: m.pairw_topk_device(di, dv, k, k, "count"), n, k, k)
        assert (idx[others] == 140).any(axis=1).all()
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ 3. fewer candidates than k
def test_fewer_candidates_than_k(hip_ctx, orc):
    M, k = 1000, 8
    mat = random_bits(np.random.default_rng(5), 5, M)
    five, one, none = hip_ctx.matrix_from_host(mat), hip_ctx.matrix_from_host(mat[:1]), hip_ctx.matrix(0, mat.shape[1])
    try:
        values = pairw_values(hip_ctx, orc, mat, five, M)
        for score in SCORES:
            pad = 0 if score == "count" else NAN_BITS
            want = top(rank(values[score], score, skip0=0), k, score)
            assert (want[0][:, :4] != NO_INDEX).all() and (want[0][:, 4:] == NO_INDEX).all() and (want[1][:, 4:] == pad).all()
            assert_topk(into_device(lambda di, dv: five.pairw_topk_device(di, dv, k + 2, k, score, n_bits=M), 5, k, k + 2), want, score)
            assert_topk(five.pairw_topk(k, score, n_bits=M), want, (score, "host"))
            # one row: k paddings
            idx, val = into_device(lambda di, dv: one.pairw_topk_device(di, dv, k, k, score, n_bits=M), 1, k, k)
            assert (idx == NO_INDEX).all() and (val == pad).all(), score
            idx, val = one.pairw_topk(k, score, n_bits=M)
            assert (idx == NO_INDEX).all() and (val.view(np.uint32) == pad).all(), score
            # an empty B: every row of A is k paddings
            idx, val = five.cross_topk(none, k, score, n_bits=M)
            assert idx.shape == (5, k) and (idx == NO_INDEX).all() and (val.view(np.uint32) == pad).all(), score
            # no rows: OK, nothing written
            _, vi = device_buffer(2, k)
            _, vv = device_buffer(2, k)
            none.pairw_topk_device(vi.data_ptr(), vv.data_ptr(), k, k, score, n_bits=M)
            hip_ctx.synchronize()
            assert (read_back(vi, 2, k) == SENTINEL).all() and (read_back(vv, 2, k) == SENTINEL).all()
            assert none.pairw_topk(k, score, n_bits=M)[0].shape == (0, k)
            assert none.cross_topk(five, k, score, n_bits=M)[0].shape == (0, k)
    finally:
        for x in (five, one, none):
            x.close()


# ------------------------------------------------------------------------------------------ 4. panels
def test_panels(hip_ctx, orc):
    """700 rows, panel_rows 256: three panels, the last of 188 rows, each against all 700 columns"""
    lib = sb.load()
    M, n, k = 1000, 700, 16
    mat = random_bits(np.random.default_rng(700), n, M)
    m = hip_ctx.matrix_from_host(mat)
    try:
        values = pairw_values(hip_ctx, orc, mat, m, M)
        for score in ("count", "jaccard", "ld_r2"):
            want = top(rank(values[score], score, skip0=0), k, score)
            paneled = into_device(lambda di, dv: m.pairw_topk_device(di, dv, k, k, score, n_bits=M, panel_rows=256), n, k, k)
            whole = into_device(lambda di, dv: m.pairw_topk_device(di, dv, k, k, score, n_bits=M, panel_rows=0), n, k, k)
            assert_topk(paneled, want, (score, 256))
            assert_topk(whole, want, (score, 0))
            assert_topk(m.pairw_topk(k, score, n_bits=M, panel_rows=512), want, (score, 512, "host"))
        # the cross form in panels: rows 300 .. 699 against rows 0 .. 299
        a, b = hip_ctx.matrix_from_host(mat[300:]), hip_ctx.matrix_from_host(mat[:300])
        try:
            want = top(rank(orc.tile_counts_op(mat, 300, n, 0, 300, 0), "count"), k, "count")
            assert_topk(a.cross_topk(b, k, "count", panel_rows=256), want, "cross, 256")
            want = top(rank(cross_bits(hip_ctx, a, b, "cosine", M), "cosine"), k, "cosine")
            assert_topk(a.cross_topk(b, k, "cosine", panel_rows=256), want, "cross cosine, 256")
        finally:
            a.close()
            b.close()
        host = np.full((n, k), SENTINEL, dtype=np.uint32)
        p = host.ctypes.data_as(C.c_void_p)
        for panel_rows in (100, 255, 257):
            assert lib.storm_hip_pairw_topk(hip_ctx._h, m._h, 4, 1, k, panel_rows, p, p, k) == -1 and sb._lib.last_error()
            assert lib.storm_hip_cross_dense_topk(hip_ctx._h, m._h, m._h, 4, 1, k, panel_rows, p, p, k) == -1
        assert (host == SENTINEL).all()
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ 5. the flush path
def test_flush_path_under_the_worst_arrival_order(hip_ctx, orc):
    """B's rows are nested prefixes of growing length, so that against A's rows (half of them all ones, half random)
    every score ascends with the column: every entry of a sweep step beats the threshold of the last sort, the staging
    area fills at every step, and the workgroup sorts as often as it can. Then B reversed: only the first step stages
    anything. Rows of 8192 columns are more than 4 x the staging capacity."""
    M, na, nb = 512, 64, 8192
    assert nb >= 4 * STAGING and STAGING <= 2048
    rng = np.random.default_rng(55)
    a_mat = random_bits(rng, na, M)
    a_mat[:32] = np.uint64((1 << 64) - 1)
    lengths = 1 + np.arange(nb) // 20                                  # 1 .. 410 in runs of 20 equal rows (the last of 12):
    assert lengths.max() <= M                                          # ranks 1 | 2 and 128 | 129 fall inside a run: ties by index
    dense = (np.arange(M)[None, :] < lengths[:, None]).astype(np.uint8)
    b_mat = np.packbits(dense, axis=1, bitorder="little").view(np.uint64)
    assert b_mat.shape == (nb, M // 64)
    a = hip_ctx.matrix_from_host(a_mat)
    try:
        for order in ("ascending", "descending"):
            bm = np.ascontiguousarray(b_mat if order == "ascending" else b_mat[::-1])
            b = hip_ctx.matrix_from_host(bm)
            try:
                counts = orc.tile_counts_op(np.concatenate([a_mat, bm]), 0, na, na, na + nb, 0)
                step = np.diff(counts.astype(np.int64), axis=1)
                assert (step >= 0).all() if order == "ascending" else (step <= 0).all()
                values = {"count": counts, "jaccard": cross_bits(hip_ctx, a, b, "jaccard", M)}
                jac = values["jaccard"][:32].view(np.float32)
                assert (np.diff(jac, axis=1) >= 0).all() if order == "ascending" else (np.diff(jac, axis=1) <= 0).all()
                for score in ("count", "jaccard"):
                    ranked = rank(values[score], score)
                    for k in (1, 128):
                        assert ties_across(ranked, k) >= 32
                        want = top(ranked, k, score)
                        def call(di, dv):
                            rc = sb.load().storm_hip_cross_dense_topk_device(hip_ctx._h, a._h, b._h, SCORES.index(score), M, k, 0,
                                                                             C.c_void_p(di), C.c_void_p(dv), k)
                            assert rc == 0, sb._lib.last_error()
                        got = into_device(call, na, k, k)
                        assert_topk(got, want, (order, score, k))
            finally:
                b.close()
    finally:
        a.close()


# ------------------------------------------------------------------------------------------ 6. the primitive alone
@pytest.mark.parametrize("ld,off", [(304, 0), (303, 1)])
def test_primitive_on_a_count_matrix_of_the_callers(hip_ctx, edge300, ld, off):
    """a count matrix with its diagonal (|A_i|) at a base 16-byte aligned with ld % 4 == 0 (128-bit loads), and 4 bytes off
    a 16-byte boundary with an odd ld (entry by entry); skip0 none, 0 (the diagonal) and one beyond the row"""
    import torch
    lib = sb.load()
    m, M, values, _ = edge300
    n, k = 300, 8
    counts = values["count"].copy()
    a = np.diag(counts).copy()
    assert np.array_equal(a, m.row_counts())
    pitched = np.full((n, ld), 0xABCDEF01, dtype=np.uint32)             # the pitch columns are never read
    pitched[:, :n] = counts
    flat, view = device_buffer(n, ld, off)
    view[:n * ld] = torch.from_numpy(pitched.reshape(-1).view(np.int32)).to("cuda:0")
    d_a = torch.from_numpy(a.astype(np.uint32).view(np.int32)).to("cuda:0")
    # float bits of the whole square, the diagonal included: the finish pass over a copy of the counts
    bits = {"count": counts}
    for measure in MEASURES:
        t = torch.from_numpy(counts.view(np.int32)).to("cuda:0")
        torch.cuda.synchronize()
        assert lib.storm_hip_similarity_finish_device(hip_ctx._h, C.c_void_p(t.data_ptr()), n, n, n, C.c_void_p(d_a.data_ptr()),
                                                      C.c_void_p(d_a.data_ptr()), 0, MEASURES.index(measure), M) == 0
        hip_ctx.synchronize()
        bits[measure] = t.cpu().numpy().view(np.uint32)
    assert (bits["jaccard"].view(np.float32).diagonal() == 1).all()
    torch.cuda.synchronize()
    for score in SCORES:
        for skip0 in (None, 0, 1000):
            want = top(rank(bits[score], score, skip0=skip0), k, score)
            if skip0 is None and score in ("count", "jaccard"):
                assert (want[0][:, 0] == np.arange(n)).all()           # a row is its own best neighbour
            got = into_device(lambda di, dv: (m.topk_rows_device(view.data_ptr(), ld, n, n, d_a.data_ptr(), d_a.data_ptr(), di, dv,
                                                                 k + 1, k, score, n_bits=M, skip0=skip0), hip_ctx.synchronize()),
                              n, k, k + 1)
            assert report(hip_ctx) == [RAN_TOPK, 0, 0, 0]
            assert_topk(got, want, (score, skip0, ld, off))
    # a window of the same matrix: rows 100 .. 149 against columns 0 .. 199, the row's own column skipped
    want = top(rank(counts[100:150, :200], "count", skip0=100), k, "count")
    got = into_device(lambda di, dv: (m.topk_rows_device(view.data_ptr() + 4 * 100 * ld, ld, 50, 200, d_a.data_ptr() + 400,
                                                         d_a.data_ptr(), di, dv, k, k, "count", skip0=100), hip_ctx.synchronize()),
                      50, k, k)
    assert_topk(got, want, "window")
    assert np.array_equal(read_back(view, n, ld), pitched)                 # the count matrix is unchanged
    if off:
        assert (flat[:off].cpu().numpy().view(np.uint32) == SENTINEL).all()


def test_primitive_refusals_and_empty_shapes(hip_ctx):
    import torch
    lib = sb.load()
    t = torch.full((64 * 16,), 3, dtype=torch.int32, device="cuda:0")
    out = torch.full((64 * 8,), 5, dtype=torch.int32, device="cuda:0")
    p, o, o2, h = C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(out.data_ptr() + 4 * 256), hip_ctx._h
    f = lib.storm_hip_topk_rows_device
    good = [p, 16, 8, 16, p, p, ALL, 0, 64, 4, o, o2, 4]      # matrix, ld, rows, columns, counts, counts, skip0, score, n_bits, k, idx, val, ld_k
    assert f(h, *good) == 0
    hip_ctx.synchronize()
    out.fill_(5)
    torch.cuda.synchronize()
    for at, bad in ((0, None), (4, None), (5, None), (10, None), (11, None), (7, 5), (7, -1), (8, 0), (8, (1 << 32) + 1),
                    (9, 0), (9, TOPK_MAX + 1), (12, 3), (1, 15)):
        args = list(good)
        args[at] = bad
        assert f(h, *args) == -1 and sb._lib.last_error(), (at, bad)
    assert f(None, *good) == -1
    before = report(hip_ctx)
    args = list(good)
    args[2] = 0                                                          # no rows: nothing launched
    assert f(h, *args) == 0 and report(hip_ctx) == before
    hip_ctx.synchronize()
    assert (out.cpu().numpy() == 5).all()
    args = list(good)
    args[3] = 0                                                          # no columns: every row is k paddings
    assert f(h, *args) == 0
    hip_ctx.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert (got[:32] == NO_INDEX).all() and (got[256:288] == NAN_BITS).all() and (got[32:256] == 5).all() and (got[288:] == 5).all()
    # the similarity entry points keep refusing 4
    assert lib.storm_hip_similarity_finish_device(h, p, 16, 8, 16, p, p, 0, 4, 64) == -1


# ------------------------------------------------------------------------------------------ 7. the storm.h forms
def _check_container(s, values, M, ks, square_of=None):
    """the host and device forms of a container against per-score value matrices (s against itself, or against square_of)"""
    n = s.n_rows
    for score in SCORES:
        ranked = rank(values[score], score, skip0=None if square_of is not None else 0)
        for k in ks:
            want = top(ranked, k, score)
            if square_of is None:
                host = s.pairw_topk(k, score, n_bits=M)
                call = lambda di, dv: s.pairw_topk_device(di, dv, n + 1, k + 2, k, score, n_bits=M, panel_rows=256)
            else:
                host = s.square_topk(square_of, k, score, n_bits=M)
                call = lambda di, dv: s.square_topk_device(square_of, di, dv, n + 1, k + 2, k, score, n_bits=M, panel_rows=256)
            assert last_pass() == RAN_TILES_OUT | RAN_TOPK
            assert host[1].dtype == (np.uint32 if score == "count" else np.float32)
            assert_topk(host, want, (score, k, "host"))
            assert_topk(into_device(call, n, k, k + 2), want, (score, k, "device"))
            assert last_pass() == RAN_TILES_OUT | RAN_TOPK


def _mirror(tri):
    tri = np.triu(tri, 1)
    return tri + tri.T


def test_contig_container(orc):
    rng = np.random.default_rng(81)
    n, M = 260, 1000
    mat = random_bits(rng, n, M)
    s = sb.StormContig(M)
    try:
        for r in _positions_of(mat):
            assert s.add(r) == r.size
        values = {"count": orc.tile_counts_op(mat, 0, n, 0, n, 0)}
        for measure in MEASURES:
            values[measure] = _mirror(s.pairw_similarity(measure, n_bits=M).view(np.uint32))
        _check_container(s, values, M, (1, 20))
        # n_bits 0: the container's vector_length
        for score in ("ld_d", "ld_r2"):
            assert_topk(s.pairw_topk(5, score), top(rank(values[score], score, skip0=0), 5, score), (score, "n_bits 0"))
    finally:
        s.free()


def test_storm_with_list_and_bitmap_blocks(orc):
    """rows of a bitmap block (thousands of positions below 65536) and a list block (a few beyond it): two block columns,
    the construction of tests/test_gpu_lag_matrix.py"""
    rng = np.random.default_rng(82)
    n, M = 200, 2 * 65536
    rows = [np.concatenate([r, 65536 + q]) for r, q in zip(_sparse_rows(rng, n, 65536, 4500, 20000),
                                                           _sparse_rows(rng, n, 65536, 10, 900))]
    s = _storm(rows)
    try:
        values = {"count": _mirror(orc.storm(rows).pair_counts()).astype(np.uint32)}
        for measure in MEASURES:
            values[measure] = _mirror(s.pairw_similarity(measure, n_bits=M).view(np.uint32))
        _check_container(s, values, M, (10,))
    finally:
        s.free()


def test_square_of_two_storm_of_different_widths(orc):
    rng = np.random.default_rng(83)
    M = 3 * 65536
    rows_a = _sparse_rows(rng, 140, 65536, 3000, 20000)                                # one block wide
    rows_b = [np.concatenate([r, 2 * 65536 + q]) for r, q in zip(_sparse_rows(rng, 75, 65536, 3000, 20000),
                                                                 _sparse_rows(rng, 75, 65536, 5, 50))]   # three blocks
    A, B, E = _storm(rows_a), _storm(rows_b), sb.Storm()
    try:
        for x, y, rx, ry in ((A, B, rows_a, rows_b), (B, A, rows_b, rows_a)):
            nx = len(rx)
            values = {"count": orc.storm(list(rx) + list(ry)).pair_counts(0, nx)[:, nx:].astype(np.uint32)}
            for measure in MEASURES:
                values[measure] = x.square_similarity(y, measure, n_bits=M).view(np.uint32)
            _check_container(x, values, M, (7,), square_of=y)
        # an empty second container: every row is k paddings; an empty first one: nothing
        idx, val = A.square_topk(E, 3, "jaccard")
        assert idx.shape == (140, 3) and (idx == NO_INDEX).all() and (val.view(np.uint32) == NAN_BITS).all()
        idx, val = A.square_topk(E, 3, "count")
        assert (idx == NO_INDEX).all() and (val == 0).all()
        assert E.square_topk(A, 3, "count")[0].shape == (0, 3)
    finally:
        for x in (A, B, E):
            x.free()


def test_container_return_codes_and_empty_containers():
    lib = sb.load()
    rng = np.random.default_rng(84)
    n, M, k = 40, 1000, 6
    rows = _positions_of(random_bits(rng, n, M))
    c, s, e_c, e_s = sb.StormContig(M), _storm(rows), sb.StormContig(M), sb.Storm()
    try:
        for r in rows:
            assert c.add(r) == r.size
        idx = np.full((n + 1, 8), SENTINEL, dtype=np.uint32)
        val = np.full((n + 1, 8), SENTINEL, dtype=np.uint32)
        p, q = idx.ctypes.data_as(C.c_void_p), val.ctypes.data_as(C.c_void_p)
        pair = lambda f, h: (lambda *a: f(h, *a))
        square = lambda f: (lambda *a: f(s._h, s._h, *a))
        forms = [(pair(lib.STORM_contig_pairw_topk, c._h), c), (pair(lib.STORM_contig_pairw_topk_device, c._h), c),
                 (pair(lib.STORM_pairw_topk, s._h), s), (pair(lib.STORM_pairw_topk_device, s._h), s),
                 (square(lib.STORM_square_topk), s), (square(lib.STORM_square_topk_device), s)]
        for f, cont in forms:
            assert f(0, M, k, 0, None, q, n, k) == -2 and f(0, M, k, 0, p, None, n, k) == -2
            assert f(0, M, k, 0, p, q, n - 1, k) == -4 and f(0, M, k, 0, p, q, n, k - 1) == -4
            assert f(5, M, k, 0, p, q, n, k) == -3 and f(-1, M, k, 0, p, q, n, k) == -3               # bad score
            assert lib.STORM_hip_error()
            assert f(0, M, 0, 0, p, q, n, 8) == -3                                                      # k 0
            assert f(0, M, TOPK_MAX + 1, 0, p, q, n, TOPK_MAX + 1) == -3                                 # k above the maximum
            assert f(0, M, k, 100, p, q, n, k) == -3                                                    # bad panel_rows
            assert f(3, (1 << 32) + 1, k, 0, p, q, n, k) == -3
            if cont is s:
                assert f(3, 0, k, 0, p, q, n, k) == -3 and f(2, 0, k, 0, p, q, n, k) == -3            # a STORM_t declares no universe
        for f in (lib.STORM_contig_pairw_topk, lib.STORM_contig_pairw_topk_device, lib.STORM_pairw_topk, lib.STORM_pairw_topk_device):
            assert f(None, 0, M, k, 0, p, q, n, k) == -1
        for f in (lib.STORM_square_topk, lib.STORM_square_topk_device):
            assert f(None, s._h, 0, M, k, 0, p, q, n, k) == -1 and f(s._h, None, 0, M, k, 0, p, q, n, k) == -1
        assert (idx == SENTINEL).all() and (val == SENTINEL).all()                                      # untouched on every refusal
        # no rows: 0, nothing written
        assert lib.STORM_contig_pairw_topk(e_c._h, 0, M, k, 0, p, q, 0, k) == 0 and lib.STORM_pairw_topk(e_s._h, 0, M, k, 0, p, q, 0, k) == 0
        assert lib.STORM_square_topk(e_s._h, s._h, 0, M, k, 0, p, q, 0, k) == 0
        assert (idx == SENTINEL).all() and (val == SENTINEL).all()
        # n_bits 0 where the score does not read it, and for a contig container's LD scores
        assert lib.STORM_pairw_topk(s._h, 0, 0, k, 0, p, q, n, 8) == 0 and lib.STORM_pairw_topk(s._h, 4, 0, k, 0, p, q, n, 8) == 0
        assert lib.STORM_contig_pairw_topk(c._h, 3, 0, k, 0, p, q, n, 8) == 0
        assert (idx[:n, :k] != SENTINEL).all() and (idx[:n, k:] == SENTINEL).all() and (idx[n:] == SENTINEL).all()
        assert (val[:n, k:] == SENTINEL).all() and (val[n:] == SENTINEL).all()
        assert e_c.pairw_topk(3)[0].shape == (0, 3) and e_s.pairw_topk(3, "count")[1].shape == (0, 3)
    finally:
        for x in (c, s, e_c, e_s):
            x.free()


# ------------------------------------------------------------------------------------------ 8. the last-pass report
def test_last_pass_report(hip_ctx, edge300):
    m, M, _, _ = edge300
    m.pairw_topk(4, "count")
    assert report(hip_ctx) == [RAN_TILES_OUT | RAN_TOPK, 300 * 300 * m.n_words, 0, 0]
    m.pairw_topk(4, "ld_r2", n_bits=M, panel_rows=256)
    assert report(hip_ctx) == [RAN_TILES_OUT | RAN_TOPK, 300 * 300 * m.n_words, 0, 0]
    b = hip_ctx.matrix_from_host(random_bits(np.random.default_rng(9), 70, M))
    try:
        b.cross_topk(m, 4, "jaccard")
        assert report(hip_ctx) == [RAN_TILES_OUT | RAN_TOPK, 70 * 300 * m.n_words, 0, 0]
        m.cross_topk(b, 4, "count", panel_rows=256)
        assert report(hip_ctx) == [RAN_TILES_OUT | RAN_TOPK, 300 * 70 * m.n_words, 0, 0]
    finally:
        b.close()
    # through storm.h: STORM_hip_last_pass
    s = sb.StormContig(M)
    try:
        for r in _positions_of(random_bits(np.random.default_rng(10), 30, M)):
            assert s.add(r) == r.size
        s.pairw_topk(3, "count")
        assert last_pass() == RAN_TILES_OUT | RAN_TOPK
    finally:
        s.free()
