"""Per-pair similarity matrices on the device: finish_tiles_kernel<SimilarityStat> alone on count matrices of the test's own, and
behind every matrix-output path (STORM_contig_pairw_similarity, STORM_pairw_similarity, STORM_square_similarity and their
_device forms).

Expected values are built from exact integers. The counts come from the CPU oracle (pair_counts, storm.c:790-814) and a
second time from a numpy count that shares no code with it (dense 0/1 rows multiplied in float32 panels, exact below
2^24); the rows' own counts from their unique positions. A value is then the rational of the measure's formula rounded
to float32 — for cosine c over the square root of a b, decided with integer square roots. The rounding is done with
fractions.Fraction (`_rn32`); so that two million entries per case do not each go through Python integers, entries whose
float64 evaluation lies further than 2^-44 (relative) from every float32 rounding boundary take that float64 rounded to
float32 — the float64 formulas below carry at most 3 roundings of 2^-53, so there both roundings are the same number —
and the Fraction path decides the rest, plus a random sample of every case, which must agree with the fast path.

Pass condition per entry: NaN (bits 0x7FC00000, nothing else) exactly where the measure is undefined, elsewhere at most
1 float32 ulp from the expected value. The tolerance is derived: the kernel evaluates in float64 (1e-15 relative) and
rounds once, which lands on the correctly rounded float or on its neighbour.

Wall time of the file on one MI355X: not measured yet ("Similarity finish", takes the figure). The host
side of it — oracle, numpy counts and the exact generator, everything but the calls under test — is about 14 s, of
which the 2049 x 65536 case is about 6 s.
"""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import stormbitmaps_amd as sb

pytestmark = pytest.mark.gpu

MEASURES = ("jaccard", "cosine", "ld_d", "ld_r2")
NAN_BITS = 0x7FC00000
RAN_LISTS_MATRIX, RAN_TILES_OUT, RAN_LISTS_SQUARE, RAN_SIMILARITY = 64, 128, 256, 512
SENTINEL = -7.5
SENTINEL_BITS = int(np.float32(SENTINEL).view(np.uint32))


# ------------------------------------------------------------------------------------------ exact expected values
def _rn32(q, root=False):
    """float32 nearest (ties to even) to the rational q >= 0, or to sqrt(q) — exact, normal range only"""
    if q == 0:
        return np.float32(0.0)
    n, d = q.numerator, q.denominator
    e = n.bit_length() - d.bit_length()
    if root:
        e //= 2
    e -= 24

    def scaled_floor(e):    # floor(x / 2^e), x = q or sqrt(q)
        if root:
            num, den = (n, d << (2 * e)) if e >= 0 else (n << (-2 * e), d)
            return math.isqrt(num // den)
        num, den = (n, d << e) if e >= 0 else (n << -e, d)
        return num // den

    m = scaled_floor(e)
    while m >= 1 << 24:
        e += 1
        m = scaled_floor(e)
    while m < 1 << 23:
        e -= 1
        m = scaled_floor(e)
    # x / 2^e against m + 1/2
    two = Fraction(2 * m + 1, 2) * Fraction(2) ** e
    x_cmp = (q > two * two) - (q < two * two) if root else (q > two) - (q < two)
    if x_cmp > 0 or (x_cmp == 0 and m & 1):
        m += 1
    assert -126 <= e + 23 and e + 24 <= 127
    return np.float32(math.ldexp(m, e))


def _exact(measure, c, a, b, M):
    """the measure of one entry as float32 from Python integers; None = undefined (NaN)"""
    c, a, b, M = int(c), int(a), int(b), int(M)
    if measure == "jaccard":
        return None if a + b - c == 0 else _rn32(Fraction(c, a + b - c))
    if measure == "cosine":
        return None if a * b == 0 else _rn32(Fraction(c * c, a * b), root=True)
    num = M * c - a * b
    if measure == "ld_d":
        v = _rn32(Fraction(abs(num), M * M))
        return np.float32(-v) if num < 0 else v
    if not (0 < a < M and 0 < b < M):
        return None
    return _rn32(Fraction(num * num, a * (M - a) * b * (M - b)))


def expected(measure, c, a, b, M, rng):
    """(float32 values, NaN mask) for a count matrix c [na, nb], row counts a [na], column counts b [nb], universe M"""
    c = np.asarray(c, dtype=np.int64)
    A = np.broadcast_to(np.asarray(a, dtype=np.int64)[:, None], c.shape)
    B = np.broadcast_to(np.asarray(b, dtype=np.int64)[None, :], c.shape)
    if measure == "jaccard":
        nan = A + B - c == 0
    elif measure == "cosine":
        nan = (A == 0) | (B == 0)
    elif measure == "ld_d":
        nan = np.zeros(c.shape, dtype=bool)
    else:
        nan = ~((A > 0) & (A < M) & (B > 0) & (B < M))
    out = np.zeros(c.shape, dtype=np.float32)
    slow = ~nan
    if M * int(max(1, c.max(initial=0))) < 1 << 52 and int(A.max(initial=0)) * int(B.max(initial=0)) < 1 << 52:
        with np.errstate(divide="ignore", invalid="ignore"):
            cf, af, bf, Mf = c.astype(np.float64), A.astype(np.float64), B.astype(np.float64), float(M)
            if measure == "jaccard":
                v = cf / (af + bf - cf)
            elif measure == "cosine":
                v = cf / np.sqrt(af * bf)
            else:
                num = (M * c - A * B).astype(np.float64)      # exact: both products below 2^52
                v = num / (Mf * Mf) if measure == "ld_d" else (num / (af * (Mf - af))) * (num / (bf * (Mf - bf)))
        v = np.where(nan, 0.0, v)
        out = v.astype(np.float32)
        # distance of v from the float32 rounding boundaries around it: half a spacing (a quarter below a power of two)
        r = np.abs(v - out.astype(np.float64))
        s = np.spacing(np.abs(out)).astype(np.float64)
        tol = np.abs(v) * 2.0 ** -44
        slow = ~nan & ((np.abs(r - s / 2) <= tol) | (np.abs(r - s / 4) <= tol))
        if measure == "ld_d" and M & (M - 1) == 0:
            # v is exact here (an exact integer below 2^52 divided by a power of two), so numpy's rounding of it, ties
            # to even included, is the correctly rounded value: only the sample goes through Fraction. (Otherwise
            # every other numerator of 25 bits is a tie, and a case of 2049 rows spends ten seconds on them.)
            slow[:] = False
        sample = rng.integers(0, c.size, size=min(c.size, 1500))
        fast = out.copy()
        slow.flat[sample] = ~nan.flat[sample]
    else:
        fast = None
    for i, j in np.argwhere(slow):
        out[i, j] = _exact(measure, c[i, j], A[i, j], B[i, j], M)
        if fast is not None and abs(r[i, j] - s[i, j] / 2) > tol[i, j] and abs(r[i, j] - s[i, j] / 4) > tol[i, j]:
            assert out[i, j] == fast[i, j], (measure, c[i, j], A[i, j], B[i, j], M)    # the sample: both paths agree
    return out, nan


def _ordered(bits):
    """float32 bit patterns as integers in the order of the values they stand for"""
    i = bits.astype(np.int64)
    return np.where(i & 0x80000000, -(i & 0x7FFFFFFF), i)


def check(got_bits, want, nan, where=None, what=""):
    """NaN exactly where `nan` (the one quiet pattern), elsewhere within 1 ulp; only over `where` (default: everywhere)"""
    got_bits = np.asarray(got_bits, dtype=np.uint32)
    where = np.ones(nan.shape, dtype=bool) if where is None else where
    is_nan = (got_bits & 0x7FFFFFFF) > 0x7F800000
    assert np.array_equal(is_nan & where, nan & where), (what, np.argwhere((is_nan != nan) & where)[:5])
    assert (got_bits[nan & where] == NAN_BITS).all(), what
    ok = where & ~nan
    ulps = np.abs(_ordered(got_bits[ok]) - _ordered(want.view(np.uint32)[ok]))
    worst = int(ulps.max(initial=0))
    assert worst <= 1, (what, worst, np.argwhere(ok)[np.argmax(ulps)])
    return worst


def _upper(n):
    return np.triu(np.ones((n, n), dtype=bool), 1)


def _numpy_counts(rows_a, rows_b, M):
    """|A_i & B_j| from dense 0/1 rows, float32 products in panels of columns (exact: a panel's sums stay below 2^24)"""
    def dense(rows):
        m = np.zeros((len(rows), M), dtype=np.uint8)
        for i, r in enumerate(rows):
            m[i, np.asarray(r, dtype=np.int64)] = 1
        return m
    da = dense(rows_a)
    db = da if rows_b is rows_a else dense(rows_b)
    out = np.zeros((len(rows_a), len(rows_b)), dtype=np.int64)
    for k in range(0, M, 16384):
        out += np.rint(da[:, k:k + 16384].astype(np.float32) @ db[:, k:k + 16384].astype(np.float32).T).astype(np.int64)
    return out


def _last_pass():
    out = (C.c_uint64 * 4)()
    assert sb.load().STORM_hip_last_pass(out) == 0
    return int(out[0])


def _set(key, value):
    assert sb.load().STORM_hip_set_option(key.encode(), value) == 0, key


@pytest.fixture(autouse=True)
def _restore_options():
    yield
    sb.load().STORM_hip_set_option(b"matrix_lists", -1)


def _random_rows(rng, n, M, lo, hi):
    """n rows over [0, M): between lo and hi positions each, never empty, never full"""
    assert 0 < lo <= hi < M
    sizes = rng.integers(lo, hi + 1, size=n)
    return [np.sort(rng.choice(M, size=k, replace=False)).astype(np.uint32) for k in sizes]


def _assert_not_hollow(c, nans, where):
    assert int(nans.sum()) == 0
    assert int((c[where] > 0).sum()) * 2 > int(where.sum()), "more than half of the pairs must intersect"


# ------------------------------------------------------------------------------------------ 1. the primitive alone
def _finish(ctx, t, ld, n_rows, n_cols, ca, cb, triangle, measure, M):
    import torch
    torch.cuda.synchronize()
    rc = sb.load().storm_hip_similarity_finish_device(ctx._h, C.c_void_p(t.data_ptr()), ld, n_rows, n_cols,
                                                      C.c_void_p(ca.data_ptr()), C.c_void_p(cb.data_ptr()), triangle,
                                                      MEASURES.index(measure), M)
    assert rc == 0, sb._lib.last_error()
    ctx.synchronize()


def _device_u32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to("cuda:0")


def _consistent_counts(rng, na, nb, M, near_independence=False):
    """row counts, column counts and a count matrix a pair of sets could have: max(0, a + b - M) <= c <= min(a, b)"""
    a = rng.integers(1, M, size=na, dtype=np.int64)
    b = rng.integers(1, M, size=nb, dtype=np.int64)
    lo = np.maximum(0, a[:, None] + b[None, :] - M)
    hi = np.minimum(a[:, None], b[None, :])
    if near_independence:     # M c ~ a b: the numerator of D and r^2 is a small difference of two 64-bit products
        mid = np.array([[int(x) * int(y) // M for y in b] for x in a], dtype=np.int64)
        c = np.clip(mid + rng.integers(-2, 3, size=mid.shape), lo, hi)
    else:
        c = lo + (rng.random((na, nb)) * (hi - lo + 1)).astype(np.int64)
        c = np.clip(c, lo, hi)
    return a, b, c


@pytest.mark.parametrize("measure", MEASURES)
def test_primitive_on_a_count_matrix_of_the_callers(hip_ctx, measure):
    import torch
    rng = np.random.default_rng(MEASURES.index(measure))
    worst = 0
    # (rows, columns, ld, triangle, element offset of the base, universe, counts near independence)
    for na, nb, ld, triangle, off, M, indep in ((130, 300, 304, 0, 0, 100000, False),      # rectangle, ragged tiles, pitch
                                                (333, 333, 340, 1, 0, 65536, False),       # triangle through the vector path
                                                (333, 333, 335, 1, 0, 65536, False),       # ld not a multiple of 4: entry by entry
                                                (70, 261, 264, 0, 1, 4096, False),         # misaligned base: entry by entry
                                                (65, 65, 68, 1, 3, 4096, False),
                                                (70, 90, 92, 0, 0, 1 << 32, True),         # 2^32 with M c ~ a b
                                                (1, 1, 1, 0, 0, 50, False)):
        a, b, c = _consistent_counts(rng, na, nb, M, indep)
        if triangle:
            b = a
            c = np.triu(np.minimum(c, c.T), 1)
            c = np.clip(c, np.maximum(0, a[:, None] + a[None, :] - M), np.minimum(a[:, None], a[None, :]))
        want, nan = expected(measure, c, a, b, M, rng)
        assert not nan.any()
        host = np.full((na, ld), SENTINEL_BITS, dtype=np.uint32)
        host[:, :nb] = c.astype(np.uint32)
        converted = np.zeros((na, ld), dtype=bool)
        converted[:, :nb] = _upper(na) if triangle else True
        host[~converted] = SENTINEL_BITS                    # the pitch and, for a triangle, every entry i >= j
        flat = torch.full((off + na * ld,), 0, dtype=torch.int32, device="cuda:0")
        view = flat[off:]
        view.copy_(_device_u32(host).reshape(-1))
        assert view.data_ptr() % 16 == (4 * off) % 16
        _finish(hip_ctx, view, ld, na, nb, _device_u32(a), _device_u32(b), triangle, measure, M)
        got = view.cpu().numpy().view(np.uint32).reshape(na, ld)
        assert (got[~converted] == SENTINEL_BITS).all(), (na, nb, ld, off)
        worst = max(worst, check(got[:, :nb], want, nan, converted[:, :nb], (measure, na, nb, ld, off)))
    print(f"primitive {measure}: worst error {worst} ulp")


def test_primitive_refuses_bad_arguments_and_ignores_empty_shapes(hip_ctx):
    import torch
    lib = sb.load()
    t = torch.full((4, 4), 3, dtype=torch.int32, device="cuda:0")
    cnt = _device_u32(np.full(4, 5))
    p, q = C.c_void_p(t.data_ptr()), C.c_void_p(cnt.data_ptr())
    f = lib.storm_hip_similarity_finish_device
    for args in ((None, 4, 4, 4, q, q, 0, 0, 64), (p, 4, 4, 4, None, q, 0, 0, 64), (p, 4, 4, 4, q, None, 0, 0, 64),
                 (p, 4, 4, 4, q, q, 0, 4, 64), (p, 4, 4, 4, q, q, 0, -1, 64), (p, 4, 4, 4, q, q, 0, 0, 0),
                 (p, 4, 4, 4, q, q, 0, 0, (1 << 32) + 1), (p, 3, 4, 4, q, q, 0, 0, 64), (p, 4, 3, 4, q, q, 1, 0, 64)):
        assert f(hip_ctx._h, *args) == -1, args
        assert sb._lib.last_error()
    assert f(hip_ctx._h, p, 4, 0, 4, q, q, 0, 0, 64) == 0 and f(hip_ctx._h, p, 4, 4, 0, q, q, 0, 0, 64) == 0
    hip_ctx.synchronize()
    assert (t.cpu().numpy() == 3).all()


# ------------------------------------------------------------------------------------------ 2. StormContig
@pytest.mark.parametrize("n,M,lo,hi", [(300, 4096, 200, 3000), (1100, 8192, 4200, 6000), (2049, 65536, 5000, 30000)])
def test_contig_host_and_device(orc, n, M, lo, hi):
    import torch
    rng = np.random.default_rng(n)
    rows = _random_rows(rng, n, M, lo, hi)
    c = orc.storm(rows).pair_counts().astype(np.int64)
    assert np.array_equal(c, np.triu(_numpy_counts(rows, rows, M), 1))
    a = np.array([len(np.unique(r)) for r in rows], dtype=np.int64)
    up = _upper(n)
    s = sb.StormContig(M)
    ld = n + 5
    dev = torch.empty((n + 1, ld), dtype=torch.float32, device="cuda:0")
    try:
        for r in rows:
            assert s.add(r) == r.size
        counts = s.pairw_matrix().astype(np.int64)
        assert np.array_equal(counts, c)
        for measure in MEASURES:
            want, nan = expected(measure, c, a, a, M, rng)
            _assert_not_hollow(c, nan[up], up)
            host = s.pairw_similarity(measure)                      # n_bits 0: the container's vector_length
            assert host.dtype == np.float32 and (host.view(np.uint32)[~up] == 0).all()
            w_host = check(host.view(np.uint32), want, nan, up, (measure, n, "host"))
            assert _last_pass() & RAN_SIMILARITY and _last_pass() & RAN_TILES_OUT
            dev.fill_(SENTINEL)
            s.pairw_similarity_device(dev.data_ptr(), n + 1, ld, measure, n_bits=M)
            full = dev.cpu().numpy()
            assert (full[n:] == SENTINEL).all() and (full[:, n:] == SENTINEL).all(), (measure, n)
            w_dev = check(full[:n, :n].view(np.uint32), want, nan, up, (measure, n, "device"))
            # entries i >= j are as the count kernel left them: zero counts inside the tiles it touched, or untouched
            low = full[:n, :n].view(np.uint32)[~up]
            assert ((low == 0) | (low == SENTINEL_BITS)).all(), (measure, n)
            print(f"contig {n} x {M} {measure}: worst error host {w_host} ulp, device {w_dev} ulp")
            if measure == "jaccard":    # the count matrix and the similarity matrix of one handle tell the same story
                union = a[:, None] + a[None, :] - counts
                assert np.array_equal(np.rint(host.astype(np.float64) * union)[up].astype(np.int64), counts[up])
    finally:
        s.free()


# ------------------------------------------------------------------------------------------ 3. / 4. Storm
def _storm(rows):
    s = sb.Storm()
    for r in rows:
        assert s.add(np.ascontiguousarray(r, dtype=np.uint32)) == 1
    return s


def _check_storm_triangle(orc, rows, M, lists, ran, rng):
    import torch
    n = len(rows)
    c = orc.storm(rows).pair_counts().astype(np.int64)
    assert np.array_equal(c, np.triu(_numpy_counts(rows, rows, M), 1))
    a = np.array([len(np.unique(r)) for r in rows], dtype=np.int64)
    up = _upper(n)
    ld = n + 3
    dev = torch.empty((n, ld), dtype=torch.float32, device="cuda:0")
    s = _storm(rows)
    try:
        _set("matrix_lists", lists)
        counts = s.pairw_matrix().astype(np.int64)
        assert np.array_equal(counts, c)
        for measure in MEASURES:
            want, nan = expected(measure, c, a, a, M, rng)
            _assert_not_hollow(c, nan[up], up)
            host = s.pairw_similarity(measure, n_bits=M)
            assert _last_pass() == ran | RAN_SIMILARITY, (_last_pass(), measure)
            assert (host.view(np.uint32)[~up] == 0).all()
            check(host.view(np.uint32), want, nan, up, (measure, "host"))
            dev.fill_(SENTINEL)
            s.pairw_similarity_device(dev.data_ptr(), n, ld, measure, n_bits=M)
            assert _last_pass() == ran | RAN_SIMILARITY, (_last_pass(), measure)
            full = dev.cpu().numpy()
            assert (full[:, n:] == SENTINEL).all()
            check(full[:, :n].view(np.uint32), want, nan, up, (measure, "device"))
            if measure == "jaccard":
                union = a[:, None] + a[None, :] - counts
                assert np.array_equal(np.rint(host.astype(np.float64) * union)[up].astype(np.int64), counts[up])
    finally:
        s.free()


def test_storm_list_only_rows_run_from_the_lists(orc):
    rng = np.random.default_rng(3)
    _check_storm_triangle(orc, _random_rows(rng, 700, 65536, 300, 700), 65536, 1, RAN_LISTS_MATRIX, rng)


def test_storm_with_bitmap_blocks_runs_on_the_dense_replica(orc):
    rng = np.random.default_rng(4)
    rows = [np.concatenate([r, 65536 + q]) for r, q in zip(_random_rows(rng, 260, 65536, 4500, 20000),
                                                           _random_rows(rng, 260, 65536, 10, 900))]
    _check_storm_triangle(orc, rows, 2 * 65536, -1, RAN_TILES_OUT, rng)


# ------------------------------------------------------------------------------------------ 5. the rectangle
def _check_square(orc, rows_a, rows_b, M, lists, ran, rng, same=False):
    import torch
    na, nb = len(rows_a), len(rows_b)
    c = _numpy_counts(rows_a, rows_a if same else rows_b, M)
    if same:
        tri = orc.storm(rows_a).pair_counts().astype(np.int64)
        assert np.array_equal(np.triu(c, 1), tri) and np.array_equal(c, c.T)
    else:
        assert np.array_equal(c, orc.storm(list(rows_a) + list(rows_b)).pair_counts(0, na)[:, na:].astype(np.int64))
    a = np.array([len(np.unique(r)) for r in rows_a], dtype=np.int64)
    b = a if same else np.array([len(np.unique(r)) for r in rows_b], dtype=np.int64)
    everywhere = np.ones((na, nb), dtype=bool)
    A = _storm(rows_a)
    B = A if same else _storm(rows_b)
    dev = torch.empty((na + 1, nb + 3), dtype=torch.float32, device="cuda:0")
    try:
        _set("matrix_lists", lists)
        for measure in MEASURES:
            want, nan = expected(measure, c, a, b, M, rng)
            _assert_not_hollow(c, nan, everywhere)
            host = A.square_similarity(B, measure, n_bits=M)
            assert _last_pass() == ran | RAN_SIMILARITY, (_last_pass(), measure)
            check(host.view(np.uint32), want, nan, None, (measure, "host"))
            dev.fill_(SENTINEL)
            A.square_similarity_device(B, dev.data_ptr(), na + 1, nb + 3, measure, n_bits=M)
            assert _last_pass() == ran | RAN_SIMILARITY, (_last_pass(), measure)
            full = dev.cpu().numpy()
            assert (full[na:] == SENTINEL).all() and (full[:, nb:] == SENTINEL).all()
            check(full[:na, :nb].view(np.uint32), want, nan, None, (measure, "device"))
            if same and measure in ("jaccard", "cosine"):
                assert (np.diag(host) == 1).all()
    finally:
        A.free()
        if not same:
            B.free()


def test_square_from_the_lists(orc):
    rng = np.random.default_rng(5)
    rows_a, rows_b = _random_rows(rng, 150, 65536, 300, 700), _random_rows(rng, 90, 65536, 300, 700)
    _check_square(orc, rows_a, rows_b, 65536, 1, RAN_LISTS_SQUARE, rng)
    _check_square(orc, rows_a, rows_a, 65536, 1, RAN_LISTS_SQUARE, rng, same=True)


def test_square_on_dense_replicas_of_unequal_width(orc):
    rng = np.random.default_rng(6)
    rows_a = _random_rows(rng, 140, 65536, 3000, 20000)                              # one block wide
    rows_b = [np.concatenate([r, 2 * 65536 + q]) for r, q in zip(_random_rows(rng, 75, 65536, 3000, 20000),
                                                                 _random_rows(rng, 75, 65536, 5, 50))]   # three blocks
    _check_square(orc, rows_a, rows_b, 3 * 65536, 0, RAN_TILES_OUT, rng)
    _check_square(orc, rows_b, rows_a, 3 * 65536, 0, RAN_TILES_OUT, rng)
    _check_square(orc, rows_b, rows_b, 3 * 65536, 0, RAN_TILES_OUT, rng, same=True)


# ------------------------------------------------------------------------------------------ the host forms' own pitch
def _into_host_window(call, na, nb):
    """a host form into a sentinel-filled buffer with more rows and a longer pitch than the matrix: the na x nb window
    as bits, after asserting that nothing outside it was written"""
    buf = np.full((na + 2, nb + 7), SENTINEL, dtype=np.float32)
    rc = call(buf.ctypes.data_as(C.c_void_p), na + 2, nb + 7)
    assert rc == 0, (rc, sb.load().STORM_hip_error())
    bits = buf.view(np.uint32)
    outside = np.ones(buf.shape, dtype=bool)
    outside[:na, :nb] = False
    assert (bits[outside] == SENTINEL_BITS).all(), np.argwhere(outside & (bits != SENTINEL_BITS))[:5]
    return bits[:na, :nb]


@pytest.mark.parametrize("kind", ["contig", "lists", "dense"])
def test_host_triangles_into_a_pitched_buffer(orc, kind):
    lib = sb.load()
    rng = np.random.default_rng(70 + len(kind))
    n, M = 203, 65536
    rows = _random_rows(rng, n, M, 300, 700) if kind == "lists" else _random_rows(rng, n, M, 3000, 20000)
    c = orc.storm(rows).pair_counts().astype(np.int64)
    assert np.array_equal(c, np.triu(_numpy_counts(rows, rows, M), 1))
    a = np.array([len(np.unique(r)) for r in rows], dtype=np.int64)
    up = _upper(n)
    if kind == "contig":
        s = sb.StormContig(M)
        for r in rows:
            assert s.add(r) == r.size
        f, ran = lib.STORM_contig_pairw_similarity, RAN_TILES_OUT
    else:
        s = _storm(rows)
        f, ran = lib.STORM_pairw_similarity, RAN_LISTS_MATRIX if kind == "lists" else RAN_TILES_OUT
    try:
        if kind != "contig":
            _set("matrix_lists", 1 if kind == "lists" else 0)
        for measure in MEASURES:
            want, nan = expected(measure, c, a, a, M, rng)
            _assert_not_hollow(c, nan[up], up)
            bits = _into_host_window(lambda p, r, ld: f(s._h, MEASURES.index(measure), M, p, r, ld), n, n)
            assert _last_pass() == ran | RAN_SIMILARITY, (_last_pass(), measure)
            assert (bits[~up] == 0).all(), (kind, measure)            # +0.0f at i >= j
            check(bits, want, nan, up, (kind, measure, "host, pitched"))
    finally:
        s.free()


@pytest.mark.parametrize("kind", ["lists", "dense"])
def test_host_rectangle_into_a_pitched_buffer(orc, kind):
    lib = sb.load()
    rng = np.random.default_rng(80 + len(kind))
    na, nb = 131, 77
    if kind == "lists":
        M = 65536
        rows_a, rows_b = _random_rows(rng, na, M, 300, 700), _random_rows(rng, nb, M, 300, 700)
    else:                                                                 # replicas of unequal width: one block, two
        M = 2 * 65536
        rows_a = _random_rows(rng, na, 65536, 3000, 20000)
        rows_b = [np.concatenate([r, 65536 + q]) for r, q in zip(_random_rows(rng, nb, 65536, 3000, 20000),
                                                                 _random_rows(rng, nb, 65536, 5, 50))]
    c = _numpy_counts(rows_a, rows_b, M)
    assert np.array_equal(c, orc.storm(list(rows_a) + list(rows_b)).pair_counts(0, na)[:, na:].astype(np.int64))
    a = np.array([len(np.unique(r)) for r in rows_a], dtype=np.int64)
    b = np.array([len(np.unique(r)) for r in rows_b], dtype=np.int64)
    A, B = _storm(rows_a), _storm(rows_b)
    ran = RAN_LISTS_SQUARE if kind == "lists" else RAN_TILES_OUT
    try:
        _set("matrix_lists", 1 if kind == "lists" else 0)
        for measure in MEASURES:
            want, nan = expected(measure, c, a, b, M, rng)
            _assert_not_hollow(c, nan, np.ones((na, nb), dtype=bool))
            bits = _into_host_window(lambda p, r, ld: lib.STORM_square_similarity(A._h, B._h, MEASURES.index(measure), M,
                                                                                   p, r, ld), na, nb)
            assert _last_pass() == ran | RAN_SIMILARITY, (_last_pass(), measure)
            check(bits, want, nan, None, (kind, measure, "host, pitched"))
    finally:
        A.free()
        B.free()


def test_primitive_alone_reports_itself_only(hip_ctx):
    import torch
    def report():
        out = (C.c_uint64 * 4)()
        assert sb.load().storm_hip_last_pass_report(hip_ctx._h, out) == 0
        return list(out)

    m = hip_ctx.matrix_from_host(np.random.default_rng(9).integers(0, 1 << 63, size=(64, 8), dtype=np.uint64))
    try:
        m.pairw()                                  # an earlier call on the same context leaves its own report behind
    finally:
        m.close()
    before = report()
    assert before[0] != 0 and not before[0] & RAN_SIMILARITY
    t = torch.full((8, 8), 3, dtype=torch.int32, device="cuda:0")
    cnt = _device_u32(np.full(8, 5))
    f = sb.load().storm_hip_similarity_finish_device
    assert f(hip_ctx._h, C.c_void_p(t.data_ptr()), 8, 0, 8, C.c_void_p(cnt.data_ptr()), C.c_void_p(cnt.data_ptr()), 0, 0, 64) == 0
    assert report() == before                      # an empty shape touches nothing, the report included
    _finish(hip_ctx, t, 8, 8, 8, cnt, cnt, 0, "jaccard", 64)
    assert report() == [RAN_SIMILARITY, 0, 0, 0]


# ------------------------------------------------------------------------------------------ 6. degenerate rows, by hand
@pytest.mark.parametrize("lists", [1, 0])
def test_degenerate_rows_with_the_nan_positions_enumerated(lists):
    M = 64
    rows = [np.zeros(0, np.uint32),            # 0: empty
            np.arange(64, dtype=np.uint32),    # 1: full (a = M)
            np.arange(32, dtype=np.uint32),    # 2
            np.arange(32, dtype=np.uint32),    # 3: identical to 2
            np.arange(32, 64, dtype=np.uint32),  # 4: the complement of 2
            np.array([0, 1, 40], np.uint32)]   # 5
    n = len(rows)
    nan_of = {
        "jaccard": {(0, 0)},                                                                 # both rows empty
        "cosine": {(i, j) for i in range(n) for j in range(n) if i == 0 or j == 0},        # either row empty
        "ld_d": set(),
        "ld_r2": {(i, j) for i in range(n) for j in range(n) if i in (0, 1) or j in (0, 1)},   # a row empty or full
    }
    c = _numpy_counts(rows, rows, M)
    a = np.array([len(r) for r in rows], dtype=np.int64)
    rng = np.random.default_rng(60 + lists)
    s = _storm(rows)
    try:
        _set("matrix_lists", lists)
        for measure in MEASURES:
            want, nan = expected(measure, c, a, a, M, rng)
            assert {(int(i), int(j)) for i, j in np.argwhere(nan)} == nan_of[measure], measure   # the generator, by hand
            sq = s.square_similarity(s, measure, n_bits=M)
            tri = s.pairw_similarity(measure, n_bits=M)
            bits = sq.view(np.uint32)
            check(bits, want, nan, None, (measure, lists))
            tb = tri.view(np.uint32)
            assert np.array_equal(tb, np.where(_upper(n), bits, 0)), (measure, lists)
            # identical rows (2, 3), complementary rows (2, 4), a row with itself; values a float holds exactly
            if measure in ("jaccard", "cosine"):
                assert sq[2, 3] == 1 and sq[2, 4] == 0 and all(sq[i, i] == 1 for i in range(1, n))
            if measure == "jaccard":
                assert sq[0, 2] == 0 and sq[1, 2] == 0.5
            if measure == "ld_r2":
                assert sq[2, 3] == 1 and sq[2, 4] == 1       # complete LD either way
            if measure == "ld_d":
                assert sq[2, 4] == -0.25 and sq[2, 3] == 0.25 and sq[0, 3] == 0 and sq[1, 2] == 0
                assert sq[2, 5] == (64 * 2 - 32 * 3) / 64 ** 2
        # a universe smaller than a row's count: r^2 is undefined for that row, D still a number
        small = 16
        defined = {5}                                         # the only row with 0 < a < 16
        want, nan = expected("ld_r2", c, a, a, small, rng)
        assert {(int(i), int(j)) for i, j in np.argwhere(~nan)} == {(5, 5)} and defined == {5}
        check(s.square_similarity(s, "ld_r2", n_bits=small).view(np.uint32), want, nan, None, ("ld_r2", small))
        d = s.square_similarity(s, "ld_d", n_bits=small)
        want, nan = expected("ld_d", c, a, a, small, rng)
        assert not nan.any()
        check(d.view(np.uint32), want, nan, None, ("ld_d", small))
        assert d[2, 3] == (16 * 32 - 32 * 32) / 16 ** 2 and d[2, 5] == (16 * 2 - 32 * 3) / 16 ** 2
    finally:
        s.free()
