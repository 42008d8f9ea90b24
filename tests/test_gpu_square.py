"""The rectangle of two STORM_t on the device: STORM_intersect_cardinality_square, STORM_square_matrix and
STORM_square_matrix_device, on the list join (K5x, lists_square_kernel) and on the dense replicas at a common width.

Every case is checked against two references: the CPU oracle, unchanged — the union container of A's rows then B's rows,
whose per-pair counts (storm.c:790-814) hold the rectangle in rows [0, N_A) x columns [N_A, N_A + N_B) — and a numpy
count that shares no code with it (the total as the sum over distinct positions of cA[p] x cB[p], the pairs from dense
boolean rows). Every case also asserts which path ran (STORM_hip_last_pass), so that a change of dispatch cannot make a
case hollow.
"""
import ctypes as C

import numpy as np
import pytest

import stormbitmaps_amd as sb
from stormbitmaps_amd import synth
from tests.test_gpu_storm_edges import _block_fns, _row_ptr, _same_headers, _seq

pytestmark = pytest.mark.gpu

RAN_POPCOUNT, RAN_FP4_STRIPS, RAN_TILES, RAN_SQUARE = 1, 4, 128, 256
OPS = ("and", "or", "xor")
SENTINEL = -7
WIN = 8191


def _u32(values):
    return np.ascontiguousarray(values, dtype=np.uint32)


def _last_pass():
    out = (C.c_uint64 * 4)()
    assert sb.load().STORM_hip_last_pass(out) == 0
    return [int(x) for x in out]


def _set(key, value):
    assert sb.load().STORM_hip_set_option(key.encode(), value) == 0, key


@pytest.fixture(autouse=True)
def _restore_options():
    yield
    for key, value in (("matrix_lists", -1), ("matrix_lists_kernel", 0)):
        sb.load().STORM_hip_set_option(key.encode(), value)


def _storm(rows):
    s = sb.Storm()
    for r in rows:
        assert s.add(_u32(r)) == 1
    return s


def _oracle_rect(orc, rows_a, rows_b):
    na = len(rows_a)
    return orc.storm(list(rows_a) + list(rows_b)).pair_counts(0, na)[:, na:].astype(np.int64)


def _numpy_rect(rows_a, rows_b):
    allpos = np.unique(np.concatenate([_u32(r) for r in list(rows_a) + list(rows_b)] + [np.zeros(0, np.uint32)]))
    def dense(rows):
        m = np.zeros((len(rows), max(1, allpos.size)), dtype=np.float32)
        for i, r in enumerate(rows):
            m[i, np.searchsorted(allpos, np.unique(_u32(r)))] = 1
        return m
    return np.rint(dense(rows_a) @ dense(rows_b).T).astype(np.int64)


def _numpy_total(rows_a, rows_b):
    def counts(rows):
        flat = np.concatenate([np.unique(_u32(r)) for r in rows] + [np.zeros(0, np.uint32)])
        return dict(zip(*np.unique(flat, return_counts=True)))
    ca, cb = counts(rows_a), counts(rows_b)
    return sum(int(c) * int(cb.get(p, 0)) for p, c in ca.items())


def _lists_eligible(rows):
    for r in rows:
        _, cnt = np.unique(_u32(r) // 65536, return_counts=True)
        if (cnt >= 4096).any() or len(np.unique(_u32(r))) > 65535:
            return False
    return any(len(r) for r in rows)


def _refs(want, rows_a, rows_b):
    la = np.array([len(np.unique(_u32(r))) for r in rows_a], dtype=np.int64)
    lb = np.array([len(np.unique(_u32(r))) for r in rows_b], dtype=np.int64)
    both = la[:, None] + lb[None, :]
    return {"and": want, "or": both - want, "xor": both - 2 * want}


def check_pair(orc, rows_a, rows_b, lists_modes=(1, 0), ops=OPS, A=None, B=None, want=None):
    """total, host matrix and device matrix for every op, with matrix_lists forced to each of `lists_modes`"""
    import torch
    if want is None:
        want = _oracle_rect(orc, rows_a, rows_b)
        assert np.array_equal(want, _numpy_rect(rows_a, rows_b))
    total = _numpy_total(rows_a, rows_b)
    assert total == int(want.sum())
    own_a, own_b = A is None, B is None
    A = _storm(rows_a) if own_a else A
    B = _storm(rows_b) if own_b else B
    na, nb = len(rows_a), len(rows_b)
    refs = _refs(want, rows_a, rows_b)
    lists_ok = _lists_eligible(rows_a) and _lists_eligible(rows_b)
    dev = torch.full((na + 1, nb + 3), SENTINEL, dtype=torch.int32, device="cuda:0")
    try:
        for lists in lists_modes:
            _set("matrix_lists", lists)
            square = lists == 1 and lists_ok
            assert A.intersect_cardinality_square(B) == total, (na, nb, lists)
            ran = _last_pass()
            assert ran[0] == (RAN_SQUARE if square else RAN_FP4_STRIPS), (na, nb, lists, ran)
            if square:
                assert ran[3] == 64
            for op in ops:
                dev.fill_(SENTINEL)
                A.square_matrix_device(B, dev.data_ptr(), na + 1, nb + 3, op)
                full = dev.cpu().numpy()
                assert _last_pass()[0] == (RAN_SQUARE if square else RAN_TILES), (na, nb, lists, op)
                got = full[:na, :nb].astype(np.int64)
                assert np.array_equal(got, refs[op]), (na, nb, lists, op, np.argwhere(got != refs[op])[:5])
                assert (full[na:] == SENTINEL).all() and (full[:, nb:] == SENTINEL).all(), (na, nb, lists, op)
                host = A.square_matrix(B, op).astype(np.int64)
                assert np.array_equal(host, refs[op]), (na, nb, lists, op)
    finally:
        if own_a:
            A.free()
        if own_b:
            B.free()
    return total


def _rows(rng, n, n_pos, hi_block=2, lo=0):
    return [np.unique(rng.integers(lo, hi_block * 65536, size=n_pos, dtype=np.uint64)).astype(np.uint32) for _ in range(n)]


# ------------------------------------------------------------------------------------------ 1. list-only pairs
@pytest.mark.parametrize("n_pos", [3, 40, 400, 3000])
def test_list_only_pairs_at_several_densities(orc, n_pos):
    rng = np.random.default_rng(n_pos)
    rows_a, rows_b = _rows(rng, 150, n_pos), _rows(rng, 90, n_pos)
    rows_a[7] = np.zeros(0, np.uint32)       # an empty row on either side
    rows_b[0] = np.zeros(0, np.uint32)
    check_pair(orc, rows_a, rows_b)


# ------------------------------------------------------------------------------------------ 2. bitmap blocks: dense
def test_bitmap_blocks_take_the_dense_rectangle(orc):
    rng = np.random.default_rng(2)
    bitmap_rows = [np.unique(np.concatenate([rng.choice(65536, 5000, replace=False),
                                             65536 + rng.choice(65536, 300, replace=False)])).astype(np.uint32)
                   for _ in range(40)]
    list_rows = _rows(rng, 70, 500)
    check_pair(orc, bitmap_rows, _rows(rng, 30, 6000, hi_block=1))      # both with bitmap blocks
    check_pair(orc, list_rows, bitmap_rows)                             # list-only against bitmaps, both ways
    check_pair(orc, bitmap_rows, list_rows, lists_modes=(1,))


# ------------------------------------------------------------------------------------------ 3. ragged shapes
def test_ragged_shapes(orc):
    rng = np.random.default_rng(3)
    pool = _rows(rng, 769 * 2, 12, hi_block=3)
    for i in range(0, len(pool), 9):
        pool[i] = np.zeros(0, np.uint32)
    union = orc.storm(pool).pair_counts().astype(np.int64)     # one oracle pass: any A prefix x B prefix is a block of it
    assert np.array_equal(union[:769, 769:], _numpy_rect(pool[:769], pool[769:]))
    for na, nb in ((1, 769), (63, 64), (64, 65), (65, 767), (767, 768), (768, 769), (769, 1), (769, 63), (1, 1),
                   (65, 64), (768, 767), (769, 768)):
        check_pair(orc, pool[:na], pool[769:769 + nb], want=union[:na, 769:769 + nb], ops=("and", "xor"))


# ------------------------------------------------------------------------------------------ 4. different universes
def test_different_universes_and_window_edges(orc):
    rng = np.random.default_rng(4)
    edges = np.array([w * WIN + k for w in range(0, 2 * 65536 // WIN) for k in (0, WIN - 1)], dtype=np.uint64)
    narrow = []    # largest block id 1
    for i in range(100):
        r = rng.integers(0, 2 * 65536, size=60, dtype=np.uint64)
        if i % 3 == 0:
            r = np.concatenate([r, rng.choice(edges, 8)])
        narrow.append(np.unique(r).astype(np.uint32))
    wide = []      # largest block id 7; some rows only beyond the narrow side's universe
    for i in range(80):
        r = rng.integers(0 if i % 4 else 2 * 65536, 8 * 65536, size=200, dtype=np.uint64)
        if i % 3 == 0:
            r = np.concatenate([r, rng.choice(edges, 8), np.array([8 * 65536 - 1], np.uint64)])
        wide.append(np.unique(r).astype(np.uint32))
    assert max(int(r.max()) for r in narrow) // 65536 == 1 and max(int(r.max()) for r in wide) // 65536 == 7
    check_pair(orc, narrow, wide)
    check_pair(orc, wide, narrow)


# ------------------------------------------------------------------------------------------ 5. counter range
def test_counter_range_65535_beside_0(orc):
    full = _seq(0, 65535)
    other = _seq(1, 65535)
    rows_a = [full, other[:10]]
    rows_b = [full, other, other[:3]]           # columns 0 and 1 share one 32-bit counter word
    want = np.array([[65535, 0, 0], [0, 10, 3]], dtype=np.int64)
    assert np.array_equal(_oracle_rect(orc, rows_a, rows_b), want)
    check_pair(orc, rows_a, rows_b, want=want)


# ------------------------------------------------------------------------------------------ 6. a == b
def test_a_container_against_itself(orc):
    rng = np.random.default_rng(6)
    rows = _rows(rng, 130, 300)
    s = _storm(rows)
    try:
        lens = np.array([len(r) for r in rows], dtype=np.int64)
        pairw = orc.storm(rows).pairw()
        want = _numpy_rect(rows, rows)
        assert np.array_equal(np.diag(want), lens) and np.array_equal(want, want.T)
        assert int(want.sum()) == 2 * pairw + int(lens.sum())
        check_pair(orc, rows, rows, A=s, B=s, want=want)
        for lists in (1, 0):
            _set("matrix_lists", lists)
            assert s.intersect_cardinality_square(s) == 2 * s.pairw_intersect_cardinality() + int(lens.sum())
            m = s.square_matrix(s, "xor")
            assert np.array_equal(m, m.T) and (np.diag(m) == 0).all()
    finally:
        s.free()


# ------------------------------------------------------------------------------------------ 7. empty, -4
def test_empty_containers_and_short_outputs():
    import torch
    lib = sb.load()
    rng = np.random.default_rng(7)
    e, a, b = sb.Storm(), _storm(_rows(rng, 5, 20)), _storm(_rows(rng, 4, 20))
    try:
        assert e.intersect_cardinality_square(a) == 0 and a.intersect_cardinality_square(e) == 0
        assert e.intersect_cardinality_square(e) == 0
        assert a.square_matrix(e).shape == (5, 0) and e.square_matrix(a).shape == (0, 5)
        host = np.full((5, 4), 9, dtype=np.uint32)
        dev = torch.full((5, 4), SENTINEL, dtype=torch.int32, device="cuda:0")
        p = host.ctypes.data_as(C.c_void_p)
        for lists in (1, 0):
            _set("matrix_lists", lists)
            assert lib.STORM_square_matrix(a._h, b._h, 0, p, 4, 4) == -4
            assert lib.STORM_square_matrix(a._h, b._h, 0, p, 5, 3) == -4
            assert (host == 9).all()
            assert lib.STORM_square_matrix_device(a._h, b._h, 0, C.c_void_p(dev.data_ptr()), 4, 4) == -4
            assert lib.STORM_square_matrix_device(a._h, b._h, 0, C.c_void_p(dev.data_ptr()), 5, 3) == -4
            assert (dev.cpu().numpy() == SENTINEL).all()
            assert lib.STORM_square_matrix_device(a._h, b._h, 0, C.c_void_p(dev.data_ptr()), 5, 4) == 0
            assert (dev.cpu().numpy() != SENTINEL).all()
            dev.fill_(SENTINEL)
    finally:
        for s in (e, a, b):
            s.free()


# ------------------------------------------------------------------------------------------ 8. caching and edits
def test_cached_copies_follow_edits_and_keep_the_triangle(orc):
    import torch
    lib = sb.load()
    _block_fns(lib)
    rng = np.random.default_rng(8)
    rows_a = _rows(rng, 120, 400, hi_block=2)
    rows_b = _rows(rng, 100, 400, hi_block=6)
    A, B = _storm(rows_a), _storm(rows_b)
    try:
        for lists in (1, 0):
            _set("matrix_lists", lists)
            tri = A.pairw_matrix()
            dev = torch.zeros((120, 120), dtype=torch.int32, device="cuda:0")
            first = A.intersect_cardinality_square(B)
            assert first == A.intersect_cardinality_square(B) == _numpy_total(rows_a, rows_b)
            # the triangle of A is what it was (A's dense replica may now be B's width)
            assert np.array_equal(A.pairw_matrix(), tri)
            A.pairw_matrix_device(dev.data_ptr(), 120, 120)
            assert np.array_equal(np.triu(dev.cpu().numpy().astype(np.int64), 1), tri.astype(np.int64))
        # B cleared and filled again: same block headers, other positions
        new_b = [_same_headers(rng, r, r) if len(r) else r for r in rows_b]
        assert B.clear() == 1
        for r in new_b:
            assert B.add(r) == 1
        rows_b = new_b
        check_pair(orc, rows_a, rows_b, A=A, B=B, ops=("and",))
        # one row of B edited behind STORM_add's back, headers unchanged
        victim = 11
        new = _same_headers(rng, rows_b[victim], rows_b[victim])
        assert lib.STORM_bitmap_cont_clear(C.c_void_p(_row_ptr(B, victim))) == 1
        assert lib.STORM_bitmap_cont_add(C.c_void_p(_row_ptr(B, victim)), new.ctypes.data_as(C.c_void_p), new.size) == 1
        rows_b[victim] = new
        check_pair(orc, rows_a, rows_b, A=A, B=B, ops=("and",))
    finally:
        A.free()
        B.free()


# ------------------------------------------------------------------------------------------ 9. c4 size
def test_halves_of_the_readme_shape_against_the_union_triangle():
    import torch
    M, N, draws, seed = 524288, 5000, 524, 42
    A, B, U = sb.Storm(), sb.Storm(), sb.Storm()
    A.add_synthetic(M, N, draws, seed=seed, row0=0)
    B.add_synthetic(M, N, draws, seed=seed, row0=N)
    U.add_synthetic(M, 2 * N, draws, seed=seed, row0=0)

    def counts(row0):
        pos = np.sort(synth.draws_for_rows(M, row0, N, draws, seed).astype(np.int64), axis=1)
        keep = np.ones_like(pos, dtype=bool)
        keep[:, 1:] = pos[:, 1:] != pos[:, :-1]
        return np.bincount(pos[keep], minlength=M)

    total = int((counts(0) * counts(N)).sum())
    try:
        tri = torch.zeros((2 * N, 2 * N), dtype=torch.int32, device="cuda:0")
        U.pairw_matrix_device(tri.data_ptr(), 2 * N, 2 * N)
        block = tri[:N, N:].clone()
        del tri
        rect = torch.full((N, N), SENTINEL, dtype=torch.int32, device="cuda:0")
        for lists in (-1, 1, 0):
            _set("matrix_lists", lists)
            assert A.intersect_cardinality_square(B) == total, lists
            rect.fill_(SENTINEL)
            A.square_matrix_device(B, rect.data_ptr(), N, N)
            assert torch.equal(rect, block), lists
            assert int(rect.to(torch.int64).sum()) == total
    finally:
        for s in (A, B, U):
            s.free()


# ------------------------------------------------------------------------------------------ 10. shards refused
def test_shard_world_of_two_is_refused():
    lib = sb.load()
    rng = np.random.default_rng(10)
    a, b = _storm(_rows(rng, 10, 30)), _storm(_rows(rng, 10, 30))
    out = np.full((10, 10), 9, dtype=np.uint32)
    try:
        assert lib.STORM_hip_set_shard(0, 2) == 0
        try:
            assert lib.STORM_intersect_cardinality_square(a._h, b._h) == (1 << 64) - 1
            assert b"ONE" in lib.STORM_hip_error()
            assert lib.STORM_square_matrix(a._h, b._h, 0, out.ctypes.data_as(C.c_void_p), 10, 10) == -3
            assert (out == 9).all()
        finally:
            assert lib.STORM_hip_set_shard(0, 1) == 0
        assert a.intersect_cardinality_square(b) == _numpy_total(_rows(np.random.default_rng(10), 10, 30),
                                                                 _rows(np.random.default_rng(10), 20, 30)[10:])
    finally:
        a.free()
        b.free()
