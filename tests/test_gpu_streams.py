"""The C-ABI on a caller's stream and across storm_hip_ctx_set_stream (the stream contract of include/storm_hip.h).

Every other GPU test runs on contexts of the NULL stream. Here the streams are torch.cuda.Stream() objects (non-blocking
streams, as torch's pool streams are), device buffers are torch tensors, and the file makes and closes its own contexts.

References. Totals: the CPU oracle (tests/_orc.py: truth_naive, truth_columns). Per-pair counts: numpy, 0/1 rows multiplied
in float32 (sums <= 8256: exact). Similarities: the exact generator and the 1-ulp check of tests/test_gpu_similarity.py.
Dosage correlations: float64 numpy as in tests/test_gpu_dosage.py / test_gpu_dosage_complete.py, NaN where a denominator is
0, elsewhere at most 1 float32 ulp. Integer outputs must be EQUAL. No result of the library is ever the reference.

Reading a `_device` output: the tensor is filled with a sentinel ON the context's stream (so the fill needs no host wait
before the call), and right after the call returns it is copied to the host under a third stream, with no synchronise of
the context's stream in between: a `_device` form that returned before its kernels had finished would hand back sentinels.

The backlog of part (c): passes of storm_hip_pairw_dense_launch over a 4096 x 65536-bit synthetic matrix into a scratch word,
enqueued on s1 through a context of their own (so that they do not evict the work lists the context under test has cached:
a call that has to plan and upload a list waits for its stream, and would drain the backlog before the scenario starts).
It is only a delay in front of what the context under test enqueues on s1. Measured once on one MI355X (HIP events around
the backlog on s1, perf_counter around the host calls that follow it, work lists and band buffers warm as in the tests):
  one pass runs 0.13 - 0.15 ms on the device and takes 6 us of host time to enqueue; BACKLOG_PASSES = 64 passes run
  8.3 - 8.9 ms and are enqueued in 0.37 ms;
  matrix create / fill_synthetic, set_stream, upload of 513 x 129 words, pairw: 0.06 - 0.10 ms of host time;
  begin, set_stream: 0.008 ms.
64 passes outlast the longest host sequence 80 times over (4 times is the least that is wanted; the host side varies with the
load of the machine), and the 2 ms that the result mailbox polls before it synchronises the context's stream 4 times.

No test asserts anything about time or about which stream finished first; only answers are asserted. Every test synchronises
the device before it releases anything."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import stormbitmaps_amd as sb
from tests.test_gpu_dosage import NAN_BITS, ordered
from tests.test_gpu_similarity import check as similarity_check, expected as similarity_expected
from tests.test_gpu_stage_edges import NONE, Desc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((300, 192), (513, 8256))      # rows x bits: the ragged shapes of tests/test_gpu_dense_edges.py
SENTINEL = -7                           # int32 / int64 fill of every device output
SENTINEL_U32 = int(np.int32(SENTINEL).view(np.uint32))
SENTINEL_F = -7.5
SENTINEL_F_BITS = int(np.float32(SENTINEL_F).view(np.uint32))

# passes of the backlog (the module's docstring has the measurement behind the number)
BACKLOG_PASSES = 64


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ------------------------------------------------------------------------------------------ inputs and references, once
class Case:
    """rows [n, words] uint64 and what the host says about them"""

    def __init__(self, orc, n, bits, seed):
        self.n, self.bits, self.words = n, bits, bits // 64
        self.mat = np.random.default_rng(seed).integers(0, 2 ** 64, size=(n, self.words), dtype=np.uint64)
        self.total = orc.truth_naive(self.mat)
        self._orc = orc

    @property
    def dense(self):
        """[n, bits] 0/1, bit v of a row from word v / 64, bit v % 64"""
        return np.unpackbits(np.ascontiguousarray(self.mat).view(np.uint8), axis=1, bitorder="little")

    @property
    def counts(self):
        """[n, n] int64, popcount(row_i & row_j), the diagonal included"""
        if not hasattr(self, "_counts"):
            d = self.dense.astype(np.float32)
            self._counts = np.rint(d @ d.T).astype(np.int64)
            assert int(np.triu(self._counts, 1).sum()) == self.total        # numpy and the oracle agree
        return self._counts

    @property
    def upper(self):
        return np.triu(np.ones((self.n, self.n), dtype=bool), 1)

    @property
    def values(self):
        """the same words read as rows of 2-bit values: [n, bits / 2]"""
        shifts = np.arange(32, dtype=np.uint64) * np.uint64(2)
        return ((self.mat[:, :, None] >> shifts) & np.uint64(3)).reshape(self.n, -1).astype(np.int64)


@pytest.fixture(scope="module")
def cases(orc):
    return {shape: Case(orc, shape[0], shape[1], 100 + i) for i, shape in enumerate(SHAPES)}


@pytest.fixture(scope="module")
def twin(orc):
    """a second matrix of the larger shape (same shape: one cached work list serves both), with another total"""
    t = Case(orc, 513, 8256, 333)
    return t


# ------------------------------------------------------------------------------------------ streams and contexts
class Streams:
    def __init__(self):
        import torch
        self.torch = torch
        self.s1, self.s2, self.reader = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
        assert self.s1.cuda_stream and self.s2.cuda_stream and self.s1.cuda_stream != self.s2.cuda_stream

    def full(self, stream, shape, value=SENTINEL, dtype=None):
        """a tensor filled on `stream`, no host wait"""
        torch = self.torch
        with torch.cuda.stream(stream):
            return torch.full(shape, value, dtype=dtype or torch.int32, device="cuda:0")

    def read(self, t):
        """the tensor on the host, copied under the reader stream (which nothing orders against the contexts' streams)"""
        with self.torch.cuda.stream(self.reader):
            return t.cpu().numpy()

    def drain(self):
        self.torch.cuda.synchronize()


@pytest.fixture(scope="module")
def st():
    s = Streams()
    yield s
    s.drain()


@pytest.fixture(scope="module")
def born(st):
    """(a), (b): a context that has never seen another stream than the caller's"""
    ctx = sb.HipContext(0, st.s1.cuda_stream)
    yield ctx
    st.drain()
    ctx.close()


class Held:
    """matrices (and other handles) of one test: everything is released after the device has gone idle"""

    def __init__(self, st):
        self.st, self.items = st, []

    def __call__(self, m):
        self.items.append(m)
        return m

    def matrix(self, ctx, mat):
        return self(ctx.matrix_from_host(mat))

    def release(self):
        self.st.drain()
        for m in reversed(self.items):
            m.close()
        self.items = []


@pytest.fixture()
def held(st):
    h = Held(st)
    yield h
    h.release()


# ------------------------------------------------------------------------------------------ (a) born on a caller's stream
@pytest.mark.parametrize("shape", SHAPES)
def test_totals_on_a_callers_stream(born, held, cases, shape):
    """default kernel, the popcount kernel (variant 2), and the three shards of 3 (which partition the pairs)"""
    c = cases[shape]
    m = held.matrix(born, c.mat)
    assert m.pairw() == c.total
    born.set_option("variant", 2)
    try:
        assert m.pairw() == c.total
        assert born.get_option("variant_used") == 2
    finally:
        born.set_option("variant", -1)
    parts = [m.pairw(r, 3) for r in range(3)]
    assert sum(parts) == c.total, parts


@pytest.mark.parametrize("n,bits", [(2048, 8256), (300, 192)])
def test_pairw_upload_on_a_callers_stream(born, held, orc, n, bits):
    """2048 rows: the panels travel on the context's second stream while the caller's stream multiplies; 300: copy, then pass"""
    mat = np.random.default_rng(n).integers(0, 2 ** 64, size=(n, bits // 64), dtype=np.uint64)
    want = orc.truth_columns(mat)
    m = held(born.matrix(n, bits // 64))            # (its zero fill is still queued when the copies start)
    assert m.pairw_upload(mat) == want
    assert m.pairw_upload(mat) == want               # work lists cached, matrix already resident
    assert np.array_equal(m.download(), mat)


def _check_triangle(got, want, upper, n):
    """got [rows, ld] as int64: want where upper, the sentinel everywhere else"""
    inside = np.zeros(got.shape, dtype=bool)
    inside[:n, :n] = upper
    assert (got[~inside] == SENTINEL).all(), np.argwhere(~inside & (got != SENTINEL))[:5].tolist()
    bad = np.argwhere((got[:n, :n] != want) & upper)
    assert len(bad) == 0, (len(bad), [(int(i), int(j), int(got[i, j]), int(want[i, j])) for i, j in bad[:5]])


@pytest.mark.parametrize("shape", SHAPES)
def test_count_matrices_are_complete_on_return(born, held, st, cases, shape):
    """pairw_matrix_device, pairw_matrix_band_device and square_matrix_device, each read under another stream at once"""
    c = cases[shape]
    n, ld = c.n, c.n + 3
    m = held.matrix(born, c.mat)
    out = st.full(st.s1, (n, ld))
    m.pairw_matrix_device(out.data_ptr(), ld)
    _check_triangle(st.read(out).astype(np.int64), c.counts, c.upper, n)

    row0, nb = n // 3 + 1, n // 2
    band = st.full(st.s1, (nb, ld))
    m.pairw_matrix_band_device(band.data_ptr(), ld, row0, nb)
    got = st.read(band).astype(np.int64)
    written = np.zeros(got.shape, dtype=bool)
    written[:, :n] = c.upper[row0:row0 + nb]
    assert (got[~written] == SENTINEL).all()
    assert np.array_equal(got[:, :n][written[:, :n]], c.counts[row0:row0 + nb][written[:, :n]])

    nb_rows = 130                                                       # B: the last 130 rows, last row first
    b = held.matrix(born, c.mat[::-1][:nb_rows])
    ldb = nb_rows + 5
    rect = st.full(st.s1, (n, ldb))
    check = sb._lib.check
    check(born._lib.storm_hip_square_matrix_device(born._h, m._h, b._h, 0, C.c_void_p(rect.data_ptr()), ldb),
          "storm_hip_square_matrix_device")
    got = st.read(rect).astype(np.int64)
    assert (got[:, nb_rows:] == SENTINEL).all()
    assert np.array_equal(got[:, :nb_rows], c.counts[:, ::-1][:, :nb_rows])


@pytest.mark.parametrize("measure", ["jaccard", "ld_r2"])
@pytest.mark.parametrize("shape", SHAPES)
def test_similarity_is_complete_on_return(born, held, st, cases, shape, measure):
    c = cases[shape]
    n, ld = c.n, c.n + 1
    a = np.diag(c.counts)
    want, nan = similarity_expected(measure, c.counts, a, a, c.bits, np.random.default_rng(5))
    m = held.matrix(born, c.mat)
    out = st.full(st.s1, (n, ld), SENTINEL_F, st.torch.float32)
    sb._lib.check(born._lib.storm_hip_pairw_similarity_device(born._h, m._h, sb.api.MEASURES[measure], c.bits,
                                                              C.c_void_p(out.data_ptr()), ld), "storm_hip_pairw_similarity_device")
    got = st.read(out).view(np.uint32)
    assert (got[:, n:] == SENTINEL_F_BITS).all()
    similarity_check(got[:, :n], want, nan, c.upper, (measure, shape))


@pytest.mark.parametrize("shape", SHAPES)
def test_lag_matrix_is_complete_on_return(born, held, st, cases, shape):
    c = cases[shape]
    n, lag = c.n, 70
    ld = lag + 2
    m = held.matrix(born, c.mat)
    out = st.full(st.s1, (n, ld))
    m.pairw_lag_matrix_device(out.data_ptr(), ld, lag)
    got = st.read(out).astype(np.int64)
    want = np.full((n, ld), SENTINEL, dtype=np.int64)
    for d in range(lag):
        i = np.arange(n - 1 - d)
        want[i, d] = c.counts[i, i + 1 + d]
    assert np.array_equal(got, want), np.argwhere(got != want)[:5].tolist()


@pytest.mark.parametrize("shape", SHAPES)
def test_topk_is_complete_on_return(born, held, st, cases, shape):
    """score "count": integers, order value descending then column ascending, a row never lists itself"""
    c = cases[shape]
    n, k, ld_k = c.n, 5, 7
    key = (int(c.counts.max()) - c.counts) * n + np.arange(n)[None, :]
    key[np.arange(n), np.arange(n)] = np.iinfo(np.int64).max
    want_idx = np.argsort(key, axis=1, kind="stable")[:, :k]
    want_val = np.take_along_axis(c.counts, want_idx, axis=1)
    m = held.matrix(born, c.mat)
    idx, val = st.full(st.s1, (n, ld_k)), st.full(st.s1, (n, ld_k))
    m.pairw_topk_device(idx.data_ptr(), val.data_ptr(), ld_k, k, score="count")
    got_idx, got_val = st.read(idx).astype(np.int64), st.read(val).astype(np.int64)
    assert (got_idx[:, k:] == SENTINEL).all() and (got_val[:, k:] == SENTINEL).all()
    assert np.array_equal(got_val[:, :k], want_val)
    assert np.array_equal(got_idx[:, :k], want_idx)


def _products(a, b):
    """a @ b.T of small non-negative integers, through float64 (sums far below 2^53: exact) for the speed of BLAS"""
    return np.rint(a.astype(np.float64) @ b.astype(np.float64).T).astype(np.int64)


def _complete_reference(x):
    """complete_reference of tests/test_gpu_dosage_complete.py (float64 r^2 and r over the samples both rows have, and where
    a denominator is 0), the six sums through _products"""
    g, m = np.where(x == 3, 0, x), (x != 3).astype(np.int64)
    N, P, Sx, Qx = _products(m, m), _products(g, g), _products(g, m), _products(g * g, m)
    Sy, Qy = Sx.T, Qx.T
    num, dx, dy = N * P - Sx * Sy, N * Qx - Sx * Sx, N * Qy - Sy * Sy
    assert (dx >= 0).all() and (dy >= 0).all()
    nan = (dx == 0) | (dy == 0)
    den = np.where(nan, 1, dx * dy).astype(np.float64)
    return {0: num.astype(np.float64) ** 2 / den, 1: num.astype(np.float64) / np.sqrt(den)}, nan


def _check_correlation(bits, want, nan, upper, what):
    """NaN (the one quiet pattern) exactly where `nan`, elsewhere at most 1 float32 ulp from the float64 value"""
    is_nan = (bits & 0x7FFFFFFF) > 0x7F800000
    assert np.array_equal(is_nan & upper, nan & upper), (what, np.argwhere((is_nan != nan) & upper)[:5].tolist())
    assert (bits[nan & upper] == NAN_BITS).all(), what
    ok = upper & ~nan
    assert ok.sum() >= 0.9 * upper.sum(), what
    ulps = np.abs(ordered(bits[ok]) - ordered(want[ok].astype(np.float32).view(np.uint32)))
    assert int(ulps.max()) <= 1, (what, int(ulps.max()), np.argwhere(ok)[np.argmax(ulps)].tolist())


@pytest.mark.parametrize("shape", SHAPES)
def test_dosage_correlations_are_complete_on_return(born, held, st, cases, shape):
    """the same words as rows of 2-bit values: pairw_dosage_corr (3 an ordinary value) and pairw_dosage_corr_complete
    (3 = missing: a quarter of every row), r^2 and r"""
    c = cases[shape]
    n, S, ld = c.n, c.bits // 2, c.n + 3
    x = c.values
    P, s, q = _products(x, x), x.sum(axis=1), (x * x).sum(axis=1)
    num, dd = S * P - s[:, None] * s[None, :], S * q - s * s
    nan = (dd[:, None] == 0) | (dd[None, :] == 0)
    den = np.where(nan, 1, dd[:, None] * dd[None, :]).astype(np.float64)
    plain = {0: num.astype(np.float64) ** 2 / den, 1: num.astype(np.float64) / np.sqrt(den)}
    complete, nan_complete = _complete_reference(x)
    m = held.matrix(born, c.mat)
    lib = born._lib
    for name, fn, want, want_nan in (("corr", lib.storm_hip_pairw_dosage_corr_device, plain, nan),
                                     ("corr_complete", lib.storm_hip_pairw_dosage_corr_complete_device, complete, nan_complete)):
        for measure in (0, 1):
            out = st.full(st.s1, (n, ld))
            sb._lib.check(fn(born._h, m._h, measure, S, C.c_void_p(out.data_ptr()), ld), name)
            got = st.read(out).view(np.uint32)
            assert (got[:, n:] == SENTINEL_U32).all() and (got[:, :n][~c.upper] == SENTINEL_U32).all(), (name, measure)
            _check_correlation(got[:, :n], want[measure], want_nan, c.upper, (name, measure, shape))


def _list_blocks(case):
    """the rows as one list block each (block 0: both widths lie below 65536 bits)"""
    d = Desc()
    for row in case.dense:
        d.block(0, 0, np.flatnonzero(row).astype(np.uint16), NONE)
        d.end_row()
    return d


@pytest.mark.parametrize("shape", SHAPES)
def test_sparse_arena_and_row_lists_on_a_callers_stream(born, st, cases, shape):
    c = cases[shape]
    lib = born._lib
    d = _list_blocks(c)
    n_rows, n_blocks, off, ids, kinds, lens, ptrs, _ = d.arrays()
    arena, lists = C.c_void_p(), C.c_void_p()
    try:
        sb._lib.check(lib.storm_hip_sparse_create_blocks(born._h, n_rows, n_blocks, _p(off), _p(ids), _p(kinds), _p(lens),
                                                         _p(ptrs), C.byref(arena)), "storm_hip_sparse_create_blocks")
        total = C.c_uint64()
        sb._lib.check(lib.storm_hip_pairw_sparse(born._h, arena, 0, 1, C.byref(total)), "storm_hip_pairw_sparse")
        assert total.value == c.total
        parts = []
        for r in range(3):
            sb._lib.check(lib.storm_hip_pairw_sparse(born._h, arena, r, 3, C.byref(total)), "storm_hip_pairw_sparse")
            parts.append(int(total.value))
        assert sum(parts) == c.total, parts

        sb._lib.check(lib.storm_hip_rowlists_create_blocks(born._h, n_rows, n_blocks, _p(off), _p(ids), _p(kinds), _p(lens),
                                                           _p(ptrs), C.byref(lists)), "storm_hip_rowlists_create_blocks")
        assert lists.value, "a list-only container is eligible for the row lists"
        ld = c.n + 3
        out = st.full(st.s1, (c.n, ld))
        sb._lib.check(lib.storm_hip_rowlists_pairw_matrix_device(born._h, lists, 0, C.c_void_p(out.data_ptr()), ld),
                      "storm_hip_rowlists_pairw_matrix_device")
        _check_triangle(st.read(out).astype(np.int64), c.counts, c.upper, c.n)
    finally:
        st.drain()
        if lists.value:
            lib.storm_hip_rowlists_destroy(born._h, lists)
        if arena.value:
            lib.storm_hip_sparse_destroy(born._h, arena)


# ------------------------------------------------------------------------------------------ (b) the asynchronous chain
def _produced_on(st, stream, mat):
    """the rows as a device tensor that a kernel on `stream` has just written (x ^ y, the operands resident beforehand)"""
    torch = st.torch
    y = np.random.default_rng(1).integers(0, 2 ** 63, size=mat.shape, dtype=np.int64)
    dx, dy = torch.from_numpy(mat.view(np.int64) ^ y).to("cuda:0"), torch.from_numpy(y).to("cuda:0")
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        return torch.bitwise_xor(dx, dy)


@pytest.mark.parametrize("shape", SHAPES)
def test_import_launch_consume_without_a_host_wait(born, held, st, cases, shape):
    """create (zero fill), import from a tensor the stream has just produced, import again out of the first matrix's own
    rows (device_ptr / stride_words), launch into a sentinel word, a torch copy of the word: five things on one stream and
    one synchronise at the end"""
    c = cases[shape]
    torch = st.torch
    src = _produced_on(st, st.s1, c.mat)
    word = st.full(st.s1, (1,), dtype=torch.int64)
    m = held(born.matrix(c.n, c.words))
    m.import_device(src.data_ptr(), c.n, c.words)
    assert m.device_ptr and m.stride_words >= c.words and m.stride_words % 64 == 0
    m2 = held(born.matrix(c.n, c.words))
    m2.import_device(m.device_ptr, c.n, m.stride_words)
    m2.pairw_launch(word.data_ptr())
    with torch.cuda.stream(st.s1):
        copy = word.clone()
    st.s1.synchronize()
    assert int(copy.item()) == c.total and int(word.item()) == c.total
    assert np.array_equal(m2.download(), c.mat)


@pytest.mark.parametrize("shape", SHAPES)
def test_launches_back_to_back_share_the_slots_in_stream_order(born, held, st, cases, shape):
    """two shards into two words, then three whole passes into three words: each pass zeroes the partial-sum slots for the
    next one on the stream, no host wait anywhere"""
    c = cases[shape]
    torch = st.torch
    m = held.matrix(born, c.mat)
    words = st.full(st.s1, (5,), dtype=torch.int64)
    base = words.data_ptr()
    m.pairw_launch(base, 0, 2)
    m.pairw_launch(base + 8, 1, 2)
    for i in range(2, 5):
        m.pairw_launch(base + 8 * i)
    with torch.cuda.stream(st.s1):
        copy = words.clone()
    st.s1.synchronize()
    got = copy.cpu().numpy().tolist()
    assert SENTINEL not in got[:2] and got[0] + got[1] == c.total, got
    assert got[2:] == [c.total] * 3, got


# ------------------------------------------------------------------------------------------ (c) across set_stream
class Switching:
    """the context under test (born on s1) and the backlog, which a context of its own enqueues on s1"""

    def __init__(self, st):
        self.st = st
        self.ctx = sb.HipContext(0, st.s1.cuda_stream)
        self.delay = sb.HipContext(0, st.s1.cuda_stream)
        self.big = self.delay.matrix(4096, 1024)
        self.big.fill_synthetic(65536, 2048, seed=7)
        self.scratch = st.full(st.s1, (1,), dtype=st.torch.int64)
        self.big.pairw_launch(self.scratch.data_ptr())      # plans and uploads the backlog's work list
        st.drain()

    def backlog(self):
        for _ in range(BACKLOG_PASSES):
            self.big.pairw_launch(self.scratch.data_ptr())

    def gate(self):
        """s2 held back by the caller until the backlog on s1 has run: both streams become free at the same moment, so work
        the library puts on them without an order of its own runs at the same time"""
        self.st.s2.wait_event(self.st.s1.record_event())

    def home(self):
        self.st.drain()
        self.ctx.set_stream(self.st.s1.cuda_stream)
        self.ctx.set_option("result_mailbox", 1)
        self.ctx.set_option("k2_fold_inline", -1)

    def fold_behind(self):
        """The total folded by a launch of its own behind the pass (k2_fold_inline 0), for the two tests whose passes would run
        AT THE SAME TIME if set_stream ordered nothing. The default for short launches folds inside the pass: the workgroup
        dispatched last polls the slots until the arrivals equal its own grid's waves, and with a second pass of the same
        context adding its arrivals to the same slots that poll never ends: the library of before the ordering hung there.
        With the fold behind the pass the same mistake is a wrong total."""
        self.ctx.set_option("k2_fold_inline", 0)

    def close(self):
        self.st.drain()
        self.big.close()
        self.delay.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def sw_module(st):
    s = Switching(st)
    yield s
    s.close()


@pytest.fixture()
def sw(sw_module, held):
    """(the matrices of a test are released, after a device-wide wait, before the context goes back to s1)"""
    yield sw_module
    held.release()
    sw_module.home()


@pytest.mark.parametrize("kind", ["create", "clear", "fill_synthetic", "shrink"])
def test_a_zero_fill_queued_on_the_old_stream_does_not_wipe_a_later_upload(sw, held, st, cases, kind):
    """the asynchronous call waits behind the backlog on s1; after set_stream(s2) the rows are uploaded (synchronous, on s2)
    and multiplied. The total must be exact, and once both streams have drained the matrix must still hold the rows"""
    c = cases[(513, 8256)]
    ctx, n = sw.ctx, c.n
    held.matrix(ctx, c.mat).pairw()                        # the work list of this shape: planned and uploaded now
    cut = n - 100
    if kind != "create":
        m = held.matrix(ctx, ~c.mat)                       # rows that a late zero fill would be seen to wipe
        st.drain()
    sw.backlog()
    if kind == "create":
        m = held(ctx.matrix(n, c.words))
    elif kind == "clear":
        m.clear()
    elif kind == "fill_synthetic":
        m.fill_synthetic(c.bits, 100, seed=3)
    else:
        m.resize(cut)                                      # zeroes rows [cut, n) on s1
    ctx.set_stream(st.s2.cuda_stream)
    if kind == "shrink":
        m.resize(n)                                        # inside the allocation: nothing is enqueued
        m.upload(c.mat[cut:], row0=cut)
        m.upload(c.mat[:cut])
    else:
        m.upload(c.mat)
    got = m.pairw()
    st.drain()
    rows = m.download()
    assert got == c.total
    wiped = np.flatnonzero((rows != c.mat).any(axis=1))
    assert len(wiped) == 0, (len(wiped), wiped[:5].tolist())


def test_create_on_the_old_stream_small_shape(sw, held, st, cases):
    c = cases[(300, 192)]
    held.matrix(sw.ctx, c.mat).pairw()
    sw.backlog()
    m = held(sw.ctx.matrix(c.n, c.words))
    sw.ctx.set_stream(st.s2.cuda_stream)
    m.upload(c.mat)
    got = m.pairw()
    st.drain()
    assert got == c.total
    assert np.array_equal(m.download(), c.mat)


def test_a_pass_on_each_side_of_set_stream(sw, held, st, cases, twin):
    """A on s1, set_stream(s2), B: the two passes share the slots, the cached work list and nothing else"""
    a, b = cases[(513, 8256)], twin
    sw.fold_behind()
    ma, mb = held.matrix(sw.ctx, a.mat), held.matrix(sw.ctx, b.mat)
    assert ma.pairw() == a.total and mb.pairw() == b.total and a.total != b.total
    words = st.full(st.s1, (2,), dtype=st.torch.int64)
    st.drain()
    sw.backlog()
    sw.gate()
    ma.pairw_launch(words.data_ptr())
    sw.ctx.set_stream(st.s2.cuda_stream)
    mb.pairw_launch(words.data_ptr() + 8)
    st.drain()
    assert words.cpu().numpy().tolist() == [a.total, b.total]


def test_twenty_launches_alternating_between_two_streams(sw, held, st, cases, twin):
    a, b = cases[(513, 8256)], twin
    sw.fold_behind()
    ma, mb = held.matrix(sw.ctx, a.mat), held.matrix(sw.ctx, b.mat)
    assert ma.pairw() == a.total and mb.pairw() == b.total
    words = st.full(st.s1, (20,), dtype=st.torch.int64)
    st.drain()
    sw.backlog()
    sw.gate()
    for i in range(20):
        sw.ctx.set_stream((st.s2 if i % 2 else st.s1).cuda_stream)
        (mb if i % 2 else ma).pairw_launch(words.data_ptr() + 8 * i)
    st.drain()
    assert words.cpu().numpy().tolist() == [a.total, b.total] * 10


def _arena(ctx, case):
    d = _list_blocks(case)
    n_rows, n_blocks, off, ids, kinds, lens, ptrs, _ = d.arrays()
    h = C.c_void_p()
    sb._lib.check(ctx._lib.storm_hip_sparse_create_blocks(ctx._h, n_rows, n_blocks, _p(off), _p(ids), _p(kinds), _p(lens),
                                                          _p(ptrs), C.byref(h)), "storm_hip_sparse_create_blocks")
    return h


class _Arena:
    def __init__(self, ctx, case):
        self.ctx, self._h = ctx, _arena(ctx, case)

    def close(self):
        if self._h:
            self.ctx._lib.storm_hip_sparse_destroy(self.ctx._h, self._h)
            self._h = None


def _dense_begin_end(ctx, m):
    lib = ctx._lib
    return (lambda: sb._lib.check(lib.storm_hip_pairw_dense_begin(ctx._h, m._h, 0, 1), "storm_hip_pairw_dense_begin"),
            lambda out: sb._lib.check(lib.storm_hip_pairw_dense_end(ctx._h, C.byref(out)), "storm_hip_pairw_dense_end"))


def _sparse_begin_end(ctx, s):
    lib = ctx._lib
    return (lambda: sb._lib.check(lib.storm_hip_pairw_sparse_begin(ctx._h, s._h, 0, 1), "storm_hip_pairw_sparse_begin"),
            lambda out: sb._lib.check(lib.storm_hip_pairw_sparse_end(ctx._h, C.byref(out)), "storm_hip_pairw_sparse_end"))


def _total_of(begin_end):
    begin, end = begin_end
    out = C.c_uint64()
    begin()
    end(out)
    return int(out.value)


@pytest.mark.parametrize("mailbox", [0, 1])
@pytest.mark.parametrize("family", ["dense", "sparse"])
def test_begin_on_one_stream_end_on_the_other(sw, held, st, cases, twin, family, mailbox):
    """begin waits behind the backlog on s1; set_stream(s2); end must wait for that pass — through the mailbox (which gives up
    polling after 2 ms and synchronises the context's stream) and through the copy of the result word alike. The result word
    holds ANOTHER matrix's total when the pass is begun, so a copy taken too early is seen"""
    a, b = cases[(513, 8256)], twin
    ctx = sw.ctx
    ctx.set_option("result_mailbox", mailbox)
    if family == "dense":
        of_a, of_b = _dense_begin_end(ctx, held.matrix(ctx, a.mat)), _dense_begin_end(ctx, held.matrix(ctx, b.mat))
    else:
        of_a, of_b = _sparse_begin_end(ctx, held(_Arena(ctx, a))), _sparse_begin_end(ctx, held(_Arena(ctx, b)))
    assert _total_of(of_a) == a.total                    # work lists planned and uploaded
    assert _total_of(of_b) == b.total                    # ... and the result word now holds B's total
    st.drain()
    sw.backlog()
    of_a[0]()
    ctx.set_stream(st.s2.cuda_stream)
    out = C.c_uint64(0)
    of_a[1](out)
    st.drain()
    assert out.value == a.total, (out.value, a.total, b.total)


@pytest.mark.parametrize("mailbox", [0, 1])
def test_band_begin_on_one_stream_end_on_the_other(sw, held, st, cases, mailbox):
    """the band form copies into HOST memory (pinned here, so that the copy is as asynchronous as the kernels): after end
    the band must be there"""
    c = cases[(513, 8256)]
    ctx, lib, torch = sw.ctx, sw.ctx._lib, st.torch
    ctx.set_option("result_mailbox", mailbox)
    m = held.matrix(ctx, c.mat)
    n, ld, row0, nb = c.n, c.n + 3, 129, 300
    host = torch.full((nb, ld), SENTINEL, dtype=torch.int32).pin_memory()

    def begin():
        sb._lib.check(lib.storm_hip_pairw_matrix_band_begin(ctx._h, m._h, 0, row0, nb, C.c_void_p(host.data_ptr()), ld),
                      "storm_hip_pairw_matrix_band_begin")

    def end():
        sb._lib.check(lib.storm_hip_pairw_matrix_band_end(ctx._h), "storm_hip_pairw_matrix_band_end")

    want = np.full((nb, ld), SENTINEL, dtype=np.int64)
    want[:, :n] = np.where(c.upper[row0:row0 + nb], c.counts[row0:row0 + nb], 0)
    begin()
    end()
    assert np.array_equal(host.numpy().astype(np.int64), want)       # (and the band buffer and the work list exist now)
    host.fill_(SENTINEL)
    st.drain()
    sw.backlog()
    begin()
    ctx.set_stream(st.s2.cuda_stream)
    end()
    got = host.numpy().astype(np.int64).copy()
    st.drain()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (len(bad), [(int(i), int(j), int(got[i, j]), int(want[i, j])) for i, j in bad[:5]])


def test_back_to_the_first_stream_and_to_the_null_stream(sw, held, st, cases, twin):
    a, b = cases[(513, 8256)], twin
    ctx = sw.ctx
    ma, mb = held.matrix(ctx, a.mat), held.matrix(ctx, b.mat)
    assert ma.pairw() == a.total
    word = st.full(st.s1, (3,), dtype=st.torch.int64)
    st.drain()
    sw.backlog()
    ma.pairw_launch(word.data_ptr())
    ctx.set_stream(st.s2.cuda_stream)
    assert mb.pairw() == b.total
    mb.pairw_launch(word.data_ptr() + 8)
    ctx.set_stream(st.s1.cuda_stream)
    assert ma.pairw() == a.total
    ma.pairw_launch(word.data_ptr() + 16)
    ctx.set_stream(0)
    assert mb.pairw() == b.total
    m = held(ctx.matrix(a.n, a.words))                    # zero fill on the NULL stream, then back to s1
    ctx.set_stream(st.s1.cuda_stream)
    m.upload(a.mat)
    assert m.pairw() == a.total
    st.drain()
    assert word.cpu().numpy().tolist() == [a.total, b.total, a.total]
    assert np.array_equal(m.download(), a.mat)


# ------------------------------------------------------------------------------------------ (d) two contexts, one thread
@pytest.fixture(scope="module")
def pair_module(st):
    a, b = sb.HipContext(0, st.s1.cuda_stream), sb.HipContext(0, st.s2.cuda_stream)
    yield a, b
    st.drain()
    a.close()
    b.close()


@pytest.fixture()
def pair(pair_module, held):
    yield pair_module
    held.release()
    for ctx in pair_module:
        ctx.set_option("result_mailbox", 1)


@pytest.mark.parametrize("mailbox", [0, 1])
def test_two_contexts_dense_begin_a_begin_b_end_b_end_a(pair, held, cases, twin, mailbox):
    a, b = cases[(513, 8256)], twin
    ca, cb = pair
    for ctx in pair:
        ctx.set_option("result_mailbox", mailbox)
    of_a, of_b = _dense_begin_end(ca, held.matrix(ca, a.mat)), _dense_begin_end(cb, held.matrix(cb, b.mat))
    for _ in range(3):
        ta, tb = C.c_uint64(0), C.c_uint64(0)
        of_a[0]()
        of_b[0]()
        of_b[1](tb)
        of_a[1](ta)
        assert (ta.value, tb.value) == (a.total, b.total)


@pytest.mark.parametrize("mailbox", [0, 1])
def test_two_contexts_band_begin_a_begin_b_end_b_end_a(pair, held, st, cases, twin, mailbox):
    a, b = cases[(513, 8256)], twin
    torch = st.torch
    n, ld, row0, nb = a.n, a.n, 200, 313
    calls = []
    for ctx, case in zip(pair, (a, b)):
        ctx.set_option("result_mailbox", mailbox)
        m = held.matrix(ctx, case.mat)
        host = torch.full((nb, ld), SENTINEL, dtype=torch.int32).pin_memory()
        want = np.where(case.upper[row0:row0 + nb], case.counts[row0:row0 + nb], 0)
        calls.append((ctx, m, host, want))
    for ctx, m, host, _ in calls:
        sb._lib.check(ctx._lib.storm_hip_pairw_matrix_band_begin(ctx._h, m._h, 0, row0, nb, C.c_void_p(host.data_ptr()), ld),
                      "storm_hip_pairw_matrix_band_begin")
    for ctx, m, host, want in reversed(calls):
        sb._lib.check(ctx._lib.storm_hip_pairw_matrix_band_end(ctx._h), "storm_hip_pairw_matrix_band_end")
        assert np.array_equal(host.numpy().astype(np.int64), want)


def test_two_contexts_interleaved_launch_chains(pair, held, st, cases, twin):
    a, b = cases[(513, 8256)], twin
    ca, cb = pair
    ma, mb = held.matrix(ca, a.mat), held.matrix(cb, b.mat)
    wa, wb = st.full(st.s1, (6,), dtype=st.torch.int64), st.full(st.s2, (6,), dtype=st.torch.int64)
    for i in range(6):
        ma.pairw_launch(wa.data_ptr() + 8 * i)
        mb.pairw_launch(wb.data_ptr() + 8 * i)
    st.drain()
    assert wa.cpu().numpy().tolist() == [a.total] * 6 and wb.cpu().numpy().tolist() == [b.total] * 6


# ------------------------------------------------------------------------------------------ (e) no warm-up at creation
CHILD = """
import numpy as np, torch
import stormbitmaps_amd as sb
mat = np.random.default_rng(77).integers(0, 2 ** 64, size=(513, 129), dtype=np.uint64)
stream = torch.cuda.Stream()
ctx = sb.HipContext(0, stream.cuda_stream)
m = ctx.matrix_from_host(mat)
first = m.pairw()
parts = [m.pairw(r, 3) for r in range(3)]
torch.cuda.synchronize()
m.close()
ctx.close()
print(first, sum(parts))
"""


def test_a_context_made_without_warm_up_on_a_non_blocking_stream(orc):
    """STORM_HIP_NO_WARM: storm_hip_ctx_create launches and waits for nothing, so only stream order stands between the zeroing
    of the workspace and the first pass. A fresh process, its own time limit, its exit status checked"""
    want = orc.truth_naive(np.random.default_rng(77).integers(0, 2 ** 64, size=(513, 129), dtype=np.uint64))
    env = dict(os.environ, STORM_HIP_NO_WARM="1")
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    first, parts = (int(v) for v in r.stdout.strip().splitlines()[-1].split())
    assert (first, parts) == (want, want)
