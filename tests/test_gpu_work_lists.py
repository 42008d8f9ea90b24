"""The cached device work lists of the matrix-core launchers and of K1 (WorkList, storm_hip_internal.h): every list is hit
by an identical request, evicted by every other list that shares its buffer, and asked for again; every result is held
against numpy (popcounts of the bit rows, integer dot products of the unpacked 2-bit values). A stale key returns wrong
numbers without a fault, so the call ORDER is what these tests are about.

One HipContext of the file's own: its cache history is what the tests below make it. Two shapes that straddle the 128-,
256- and 512-row tiles with ragged last tiles, and a second matrix of the first shape with other rows: the same key, other
content — a hit must still read the rows it is given."""
import ctypes as C
import itertools

import numpy as np
import pytest

import stormbitmaps_amd as sb
from tests.conftest import shipped

pytestmark = pytest.mark.gpu

SHAPES = {"a": (300, 8), "b": (700, 16), "a2": (300, 8)}   # rows x 64-bit words; a2: a's key, other rows
LAG = 150


def _unpack(rows, bits):
    """[n, words] uint64 -> [n, words * 64 / bits] float32 values of `bits` bits each, lowest first (exact in float32:
    every product sum below stays under 2^24)."""
    b = np.unpackbits(rows.view(np.uint8), axis=1, bitorder="little").astype(np.float32)
    return b if bits == 1 else b[:, 0::2] + 2.0 * b[:, 1::2]


def _lag_layout(full, lag):
    n = full.shape[0]
    w = min(lag, n - 1)
    out = np.zeros((n, w), dtype=np.uint32)
    for d in range(w):
        out[:n - 1 - d, d] = np.diagonal(full, d + 1)
    return out


class _Ref:
    """The numpy answers of one matrix, computed once."""

    def __init__(self, rows):
        self.rows = rows
        self.bits = _unpack(rows, 1)
        self.vals = _unpack(rows, 2)
        self.and_ = (self.bits @ self.bits.T).astype(np.int64)
        self.dot = (self.vals @ self.vals.T).astype(np.int64)
        self.total = int(np.triu(self.and_, 1).sum())
        self.tri = np.triu(self.and_, 1).astype(np.uint32)
        self.lag = _lag_layout(self.and_, LAG)
        self.dot_tri = np.triu(self.dot, 1).astype(np.uint32)
        self.dot_lag = _lag_layout(self.dot, LAG)


@pytest.fixture(scope="module")
def env():
    rng = np.random.default_rng(20261020)
    ctx = sb.HipContext(0)
    refs = {k: _Ref(rng.integers(0, 1 << 64, size=s, dtype=np.uint64)) for k, s in SHAPES.items()}
    mats = {k: ctx.matrix_from_host(r.rows) for k, r in refs.items()}
    yield ctx, mats, refs
    for m in mats.values():
        m.close()
    ctx.close()


DEFAULTS = {"variant": -1, "k2_tile_shape": 0, "k2_matrix_parts": 0, "k2_strip_operands": 0, "k2_strip_rows": 0, "k2_max_run": 0,
            "k2_part_min_chunks": 8, "seg_rows": 256}


def _set(ctx, **options):
    for key, value in {**DEFAULTS, **options}.items():
        ctx.set_option(key, value)


def _host(m, name, shape, *args):
    """A host-form C call `name`(ctx, matrix, *args, out, ld) into a zeroed uint32 array of `shape`."""
    out = np.zeros(shape, dtype=np.uint32)
    rc = getattr(m._lib, name)(m.ctx._h, m._h, *args, out.ctypes.data_as(C.c_void_p), shape[1])
    assert rc == 0, (name, m._lib.storm_hip_last_error())
    return out


def _item_calls(ctx, mats, refs):
    """name -> call(key): runs one call that plans a list in the tile kernels' item buffer on matrix `key` and holds the
    result against numpy."""
    def total3(k):
        _set(ctx, variant=3)
        assert mats[k].pairw() == refs[k].total

    def tiles(shape, parts):
        def call(k):
            _set(ctx, k2_tile_shape=shape, k2_matrix_parts=parts)
            assert np.array_equal(mats[k].pairw_matrix(), refs[k].tri)
        return call

    def lag(k):
        _set(ctx)
        assert np.array_equal(mats[k].pairw_lag_matrix(LAG), refs[k].lag)

    def lag_dosage(k):
        _set(ctx)
        assert np.array_equal(mats[k].pairw_lag_dosage_matrix(LAG), refs[k].dot_lag)

    def dosage_triangle(k):
        _set(ctx)
        n = mats[k].n_rows
        assert np.array_equal(_host(mats[k], "storm_hip_pairw_dosage_matrix", (n, n)), refs[k].dot_tri)

    def dosage_rectangle(k):   # against the matrix of the other shape's row count where the words agree: a x a2
        _set(ctx)
        other = "a2" if k == "a" else "a" if k == "a2" else k
        want = (refs[k].vals @ refs[other].vals.T).astype(np.uint32)
        got = _host(mats[k], "storm_hip_square_dosage_matrix", want.shape, mats[other]._h)
        assert np.array_equal(got, want)

    calls = {"sum-mode tiles": total3, "K2h": tiles(0, 0), "lag": lag, "lag dosage": lag_dosage,
             "dosage triangle": dosage_triangle, "dosage rectangle": dosage_rectangle}
    for shape in shipped(ctx, "k2_tile_shape", (5, 2, 3, 1)):
        for parts in ((0, 1) if shape == 2 else (0,)):
            calls[f"tiles {shape} parts {parts}"] = tiles(shape, parts)
    return calls


def test_every_list_of_the_item_buffer_survives_every_other_one(env):
    """d_items holds one list at a time — sum-mode tiles (variant 3), the 256 x 256 output tiles (k2_tile_shape 5, and 2 with
    the parts added by atomics or by reduce_parts_kernel), K2h at the default, in the lag layout, on 2-bit values (lag,
    triangle, rectangle): A B A over every ordered pair and both shapes, then A on other rows under A's key."""
    ctx, mats, refs = env
    calls = _item_calls(ctx, mats, refs)
    for (name_a, a), (name_b, b) in itertools.permutations(calls.items(), 2):
        for k in ("a", "b"):
            try:
                a(k), b(k), a(k)
                if k == "a":
                    a("a2"), a("a")
            except AssertionError as e:
                raise AssertionError(f"{name_a} / {name_b} / {name_a} on {SHAPES[k]}: {e}") from None


def test_k2h_list_is_keyed_by_its_options(env):
    """k2_part_min_chunks is part of the K2h request: two otherwise equal calls on either side of a change are both right."""
    ctx, mats, refs = env
    for k in ("a", "b"):
        for chunks in (8, 1, 2, 8):
            _set(ctx, k2_part_min_chunks=chunks)
            assert np.array_equal(mats[k].pairw_matrix(), refs[k].tri), (k, chunks)
            assert ctx.get_option("k2_tile_shape_used") == 6
            assert np.array_equal(mats[k].pairw_lag_matrix(LAG), refs[k].lag), (k, chunks)


def _strip_calls(ctx, mats, refs):
    def total(**options):
        def call(k):
            _set(ctx, **options)
            assert mats[k].pairw() == refs[k].total
        return call

    def square(k):   # launch_square_mfma: overwrites the strip list without a key
        _set(ctx)
        other = "a2" if k == "a" else "a" if k == "a2" else k
        assert mats[k].square(mats[other]) == int((refs[k].bits @ refs[other].bits.T).astype(np.int64).sum())

    def shards(k):
        _set(ctx, k2_strip_operands=5, k2_strip_rows=64)
        assert mats[k].pairw(0, 2) + mats[k].pairw(1, 2) == refs[k].total

    def rows128(k):   # 128 A rows per wave where the allocation has the zero rows up to a multiple of 512 (300 rows: yes; 700: no)
        total(k2_strip_operands=5, k2_strip_rows=128)(k)
        assert ctx.get_option("k2_strip_rows_used") == (128 if mats[k].n_rows <= 512 else 64)

    calls = {"K2b 64": total(k2_strip_operands=5, k2_strip_rows=64), "K2b 128": rows128, "square": square, "shards": shards}
    for operands in shipped(ctx, "k2_strip_operands", (4, 6, 1)):
        calls[f"operands {operands}"] = total(k2_strip_operands=operands)
    return calls


def test_every_strip_list_survives_every_other_one(env):
    """The strip list: K2b with 64 and 128 rows per wave, the FP4 strips (4), the 512-row tiles (6), the rectangle's keyless
    list, the two shards of a pass: A B A over every ordered pair and both shapes, then A on other rows under A's key."""
    ctx, mats, refs = env
    calls = _strip_calls(ctx, mats, refs)
    for (name_a, a), (name_b, b) in itertools.permutations(calls.items(), 2):
        for k in ("a", "b"):
            try:
                a(k), b(k), a(k)
                if k == "a":
                    a("a2"), a("a")
            except AssertionError as e:
                raise AssertionError(f"{name_a} / {name_b} / {name_a} on {SHAPES[k]}: {e}") from None


def test_strip_list_is_keyed_by_its_options(env):
    """k2_max_run shapes the strip list: two otherwise equal calls on either side of a change are both right."""
    ctx, mats, refs = env
    for k in ("a", "b"):
        for operands in (5, 4):
            for run in (0, 1, 3, 0):
                _set(ctx, k2_strip_operands=operands, k2_strip_rows=64, k2_max_run=run)
                assert mats[k].pairw() == refs[k].total, (k, operands, run)


def test_stream_lists_around_a_strip_list(env):
    """K2q (k2_strip_operands 2; in the tools build K2w, 3, which keeps its words in the same buffer under another key)
    before and after a strip-list call and each other, at both shapes and on other rows under the same key."""
    ctx, mats, refs = env
    forms = shipped(ctx, "k2_strip_operands", (2, 3))
    for k in ("a", "b", "a2", "a"):
        for operands in forms + (5,) + forms + forms[::-1]:
            _set(ctx, k2_strip_operands=operands)
            assert mats[k].pairw() == refs[k].total, (k, operands)
            assert mats[k].pairw(1, 2) + mats[k].pairw(0, 2) == refs[k].total, (k, operands)


def test_panel_lists_of_the_uploading_pass(env):
    """storm_hip_pairw_dense_upload keeps one list per row panel: 700 rows, then 300, then 700, then 300 with other rows."""
    ctx, mats, refs = env
    _set(ctx)
    for k in ("b", "a", "b", "a2", "a"):
        assert mats[k].pairw_upload(refs[k].rows) == refs[k].total, k


def _k1_rounds(ctx, total_of, want):
    for variant in (0, 1, 2):
        for seg_rows in (256, 100, 256):
            _set(ctx, variant=variant, seg_rows=seg_rows)
            assert total_of(0, 1) == want, (variant, seg_rows)
        assert total_of(0, 2) + total_of(1, 2) == want, variant
        assert total_of(0, 1) == want, variant


def test_k1_segment_tables_of_the_context(env):
    """The popcount kernels' segment table: seg_rows 256, 100, 256, then the two shards, at both shapes and on other rows."""
    ctx, mats, refs = env
    for k in ("a", "b", "a2", "a"):
        _k1_rounds(ctx, mats[k].pairw, refs[k].total)


def test_k1_segment_tables_of_a_sparse_container(env):
    """The same on sparse containers, whose handles keep their own table: two containers with the rows of the two shapes,
    on the one context, in turn."""
    ctx, _, refs = env
    lib = sb.load()
    handles = {}
    try:
        for k in ("a", "b"):
            s = sb.Storm()
            for row in refs[k].bits:
                s.add(np.flatnonzero(row).astype(np.uint32))
            data = s.serialize()
            s.free()
            handles[k] = C.c_void_p()
            assert lib.storm_hip_sparse_create_serialized(ctx._h, data.ctypes.data_as(C.c_void_p), data.size, C.byref(handles[k])) == 0

        def total_of(k):
            def call(rank, count):
                out = C.c_uint64()
                assert lib.storm_hip_pairw_sparse(ctx._h, handles[k], rank, count, C.byref(out)) == 0, lib.storm_hip_last_error()
                return out.value
            return call
        for k in ("a", "b", "a"):
            _k1_rounds(ctx, total_of(k), refs[k].total)
    finally:
        for h in handles.values():
            lib.storm_hip_sparse_destroy(ctx._h, h)
        _set(ctx)
