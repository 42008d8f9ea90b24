"""Dosage rows with missing genotypes, and the rectangle of two dosage containers, on the device (storm.h:
STORM_dosage_square_dot, _row_missing, _pairw_nobs, _pairw_corr_complete). The rectangle is K2h in its dosage form over
n_a x n_b (tile128_kernel<false, 2> with a column base and count); the pairwise-complete correlation splits the rows into G
(3 -> 0), H (1 where 2) and M (1 where present) on the device, multiplies the triangles of G and M and the rectangle
[G ; H] x M, and finishes in place. Everything goes through the C-ABI, in the host and the _device forms, which must be
bit-identical.

The reference is numpy in this file: `A.astype(int64) @ B.T` for the rectangle (EQUAL), and for the correlation the sums
over the samples both rows have, in int64, divided in float64: NaN (0x7FC00000) exactly where dx or dy is 0, elsewhere at
most 1 float32 ulp (tests/test_dosage_complete_math.py derives the bound on the CPU). Device outputs are pre-filled with a
sentinel and have ld > n: nothing outside the window, and nothing at i >= j of a triangle, may change."""
import ctypes as C

import numpy as np
import pytest

import stormbitmaps_amd as sb
from stormbitmaps_amd import dist
from tests.test_gpu_dosage import NAN_BITS, SENTINEL, SENTINEL_I32, WEIGHT, Dosage, genotypes, ordered, pack  # noqa: F401

pytestmark = pytest.mark.gpu

HOST_FILL = -7.5
HOST_FILL_BITS = int(np.float32(HOST_FILL).view(np.uint32))


# ------------------------------------------------------------------------------------------ helpers
class Complete(Dosage):
    """tests/test_gpu_dosage.py's container with the calls of this file"""

    def nobs_host(self):
        n = self.n
        out = np.full((n + 1, n + 3), SENTINEL, dtype=np.uint32)
        self.ok(self.lib.STORM_dosage_pairw_nobs(self.h, out.ctypes.data, n + 1, n + 3), "STORM_dosage_pairw_nobs")
        return out

    def nobs_device(self):
        return self._device(lambda p, rows, ld: self.lib.STORM_dosage_pairw_nobs_device(self.h, C.c_void_p(p), rows, ld))

    def complete_host(self, measure):
        n = self.n
        out = np.full((n + 1, n + 3), HOST_FILL, dtype=np.float32)
        self.ok(self.lib.STORM_dosage_pairw_corr_complete(self.h, measure, out.ctypes.data, n + 1, n + 3),
                "STORM_dosage_pairw_corr_complete")
        return out.view(np.uint32)

    def complete_device(self, measure):
        return self._device(lambda p, rows, ld: self.lib.STORM_dosage_pairw_corr_complete_device(self.h, measure, C.c_void_p(p),
                                                                                                 rows, ld))

    def missing(self):
        miss = np.full(self.n + 1, SENTINEL, dtype=np.uint32)
        self.ok(self.lib.STORM_dosage_row_missing(self.h, miss.ctypes.data), "STORM_dosage_row_missing")
        assert miss[self.n] == SENTINEL
        return miss[:self.n]


def square_host(a, b):
    out = np.full((a.n + 1, b.n + 3), SENTINEL, dtype=np.uint32)
    a.ok(a.lib.STORM_dosage_square_dot(a.h, b.h, out.ctypes.data, a.n + 1, b.n + 3), "STORM_dosage_square_dot")
    return out


def square_device(a, b):
    import torch
    ld = b.n + 5
    buf = torch.full(((a.n + 1) * ld,), SENTINEL_I32, dtype=torch.int32, device="cuda:0")
    a.ok(a.lib.STORM_dosage_square_dot_device(a.h, b.h, C.c_void_p(buf.data_ptr()), a.n + 1, ld), "STORM_dosage_square_dot_device")
    return buf.cpu().numpy().view(np.uint32).reshape(a.n + 1, ld)


def check_square(a, b, want):
    """host and _device forms of the rectangle against `want` [n_a, n_b] (int64): exact everywhere inside the window, both
    forms alike, everything outside the window untouched"""
    host, dev = square_host(a, b), square_device(a, b)
    for got, name in ((host, "host"), (dev, "device")):
        inside = np.zeros(got.shape, dtype=bool)
        inside[:a.n, :b.n] = True
        assert (got[~inside] == SENTINEL).all(), (name, a.n, b.n, a.S, np.argwhere(~inside & (got != SENTINEL))[:5].tolist())
        win = got[:a.n, :b.n].astype(np.int64)
        bad = np.argwhere(win != want)
        assert bad.size == 0, (name, a.n, b.n, a.S, bad[:5].tolist(), [(int(win[i, j]), int(want[i, j])) for i, j in bad[:5]])
    assert np.array_equal(host[:a.n, :b.n], dev[:a.n, :b.n])


def check_triangle(host, dev, n, want, host_below=0):
    """a uint32 triangle in both forms against `want` [n, n]: equal at i < j; host `host_below` at i >= j; the device's i >= j
    and everything outside the n x n window of either output untouched (host fill: SENTINEL)"""
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    for got, name in ((host, "host"), (dev, "device")):
        inside = np.zeros(got.shape, dtype=bool)
        if n >= 2:
            inside[:n, :n] = True
        assert (got[~inside] == SENTINEL).all(), (name, n)
        if n >= 2:
            win = got[:n, :n].astype(np.int64)
            bad = np.argwhere((win != want) & upper)
            assert bad.size == 0, (name, n, bad[:5].tolist(), [(int(win[i, j]), int(want[i, j])) for i, j in bad[:5]])
            assert (got[:n, :n][~upper] == (host_below if name == "host" else SENTINEL)).all(), (name, n)


def complete_sums(X):
    """the six sums of every pair over the samples both rows have, int64 [n, n] each: N, P, Sx, Sy, Qx, Qy"""
    x = np.asarray(X).astype(np.int64)
    g, m = np.where(x == 3, 0, x), (x != 3).astype(np.int64)
    N, P, Sx, Qx = m @ m.T, g @ g.T, g @ m.T, (g * g) @ m.T
    return N, P, Sx, Sx.T, Qx, Qx.T


def complete_reference(X):
    """float64 r^2 and r of every pair, and where they are undefined (dx or dy is 0)"""
    N, P, Sx, Sy, Qx, Qy = complete_sums(X)
    num, dx, dy = N * P - Sx * Sy, N * Qx - Sx * Sx, N * Qy - Sy * Sy
    assert (dx >= 0).all() and (dy >= 0).all()
    nan = (dx == 0) | (dy == 0)
    den = np.where(nan, 1, dx * dy).astype(np.float64)
    return {0: num.astype(np.float64) ** 2 / den, 1: num.astype(np.float64) / np.sqrt(den)}, nan, num


@pytest.fixture(scope="module")
def hip_ctx():
    ctx = sb.HipContext(0)
    yield ctx
    ctx.close()


@pytest.fixture()
def options(lib):
    """STORM_hip_set_option for the length of one test: the K2h part options go back to what ships"""
    def set_options(**kw):
        for k, v in kw.items():
            assert lib.STORM_hip_set_option(k.encode(), v) == 0, k
    yield set_options
    set_options(k2_part_min_chunks=8, k2_part_narrow=1)


def planned(hip_ctx, n_a, n_b, S, min_chunks):
    """what the device launches for these options, from the planner itself (the device's CU count, default slots and cost)"""
    return dist.dosage_square_plan(n_a, n_b, (S + 31) // 32, n_cus=hip_ctx.get_option("n_cus"), slots_per_cu=0,
                                   min_chunks=min_chunks, diag_cost_pct=80)


# ------------------------------------------------------------------------------------------ 1. rectangle edges
SQUARE_SHAPES = ((1, 1), (2, 129), (127, 128), (128, 128), (129, 2), (257, 130))
SQUARE_S = (1, 31, 33, 255, 257, 1025)


@pytest.fixture(scope="module")
def square_values():
    """257 rows of A and 130 of B of seeded values 0 .. 3 per S, and their numpy products: computed once"""
    out = {}
    for S in SQUARE_S:
        rng = np.random.default_rng(3000 + S)
        A = rng.integers(0, 4, size=(257, S), dtype=np.uint8)
        B = rng.integers(0, 4, size=(130, S), dtype=np.uint8)
        out[S] = (A, B, A.astype(np.int64) @ B.astype(np.int64).T)
    return out


@pytest.mark.parametrize("S", SQUARE_S)
@pytest.mark.parametrize("n_a,n_b", SQUARE_SHAPES)
def test_rectangle_at_the_row_and_sample_edges(lib, square_values, n_a, n_b, S):
    """one row each, either side of the 128-row tile on either operand, three tiles by two with ragged last ones; samples
    either side of the 32-value word and the 256-value chunk, four chunks and one value"""
    A, B, P = square_values[S]
    a, b = Dosage(lib, A[:n_a]), Dosage(lib, B[:n_b])
    try:
        check_square(a, b, P[:n_a, :n_b])
    finally:
        a.close()
        b.close()


def test_a_container_against_itself_gives_the_whole_symmetric_matrix(lib, square_values):
    A, _, _ = square_values[257]
    a = Dosage(lib, A[:130])
    try:
        g = A[:130].astype(np.int64)
        check_square(a, a, g @ g.T)
    finally:
        a.close()


# ------------------------------------------------------------------------------------------ 2. position probes
@pytest.mark.parametrize("value", [1, 2, 3])
def test_a_single_sample_is_multiplied_only_with_its_own_position(lib, value):
    """rows with ONE non-zero sample at the positions where a class, a word, a 16-byte slot or a chunk changes, in A (values
    `value` and 3) and in B (values 1 and 2): the product is v_a v_b where the positions are equal and 0 elsewhere"""
    S = 1025
    positions = [0, 1, 2, 31, 32, 63, 64, 255, 256, 511, 512, S - 1]
    rows_a = [(p, v) for p in positions for v in (value, 3)]
    rows_b = [(p, v) for v in (1, 2) for p in positions]
    A = np.zeros((len(rows_a), S), dtype=np.uint8)
    B = np.zeros((len(rows_b), S), dtype=np.uint8)
    for i, (p, v) in enumerate(rows_a):
        A[i, p] = v
    for j, (p, v) in enumerate(rows_b):
        B[j, p] = v
    want = np.array([[va * vb if pa == pb else 0 for (pb, vb) in rows_b] for (pa, va) in rows_a], dtype=np.int64)
    assert np.array_equal(want, A.astype(np.int64) @ B.astype(np.int64).T)
    a, b = Dosage(lib, A), Dosage(lib, B)
    try:
        check_square(a, b, want)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------ 3. window limits
@pytest.mark.parametrize("S,min_chunks,narrow_planned", [(14848, 29, 0), (14336, 28, 1)])
@pytest.mark.parametrize("narrow_option", [1, 0])
def test_sixteen_bit_windows_stop_where_a_part_could_overflow_them(lib, hip_ctx, options, S, min_chunks, narrow_planned,
                                                                   narrow_option):
    """130 x 130 rows of all 3s: every product is 9, the most a part can hold. S = 14848 = 58 chunks as two parts of 29: a part
    sums to 66816, beyond 16 bits — wide windows. S = 14336 = 56 chunks as two parts of 28: 64512, just inside — narrow
    windows. Both again with k2_part_narrow = 0. The plan is asserted as well as the result."""
    n = 130
    plan = planned(hip_ctx, n, n, S, min_chunks)
    assert len(plan) == 8 and (plan[:, 6] == 2).all() and (plan[:, 3] == min_chunks).all(), plan.tolist()
    assert (plan[:, 7] == narrow_planned).all(), plan.tolist()
    assert (min_chunks * WEIGHT > 65535) == (narrow_planned == 0)
    options(k2_part_min_chunks=min_chunks, k2_part_narrow=narrow_option)
    G = np.full((n, S), 3, dtype=np.uint8)
    a, b = Dosage(lib, G, packed_only=True), Dosage(lib, G, packed_only=True)
    try:
        check_square(a, b, np.full((n, n), 9 * S, dtype=np.int64))
        assert 9 * S == {14848: 133632, 14336: 129024}[S]
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------ 4. long k
def test_rows_of_2_pow_21_samples_are_summed_exactly_across_parts(lib, hip_ctx, options):
    """3 x 3 rows of S = 2^21 samples of 3s, with one sample of 2 in A's row 1 (first half of k) and one sample of 1 in B's row
    2 (second half): with T = 9 S = 18874368 the products are T, T - 3 (A's row 1), T - 6 (B's row 2) and T - 9 (both) —
    odd and even values above 2^24 that an f32 sum across the parts would round. Two parts of 4096 chunks, from the plan."""
    S = 1 << 21
    plan = planned(hip_ctx, 3, 3, S, 4096)
    assert len(plan) == 2 and (plan[:, 6] == 2).all() and (plan[:, 3] == 4096).all() and (plan[:, 7] == 0).all(), plan.tolist()
    options(k2_part_min_chunks=4096)
    wa = np.full((3, S // 32), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    wb = wa.copy()

    def set_value(words, row, s, v):
        words[row, s // 32] &= ~(np.uint64(3) << np.uint64(2 * (s % 32)))
        words[row, s // 32] |= np.uint64(v) << np.uint64(2 * (s % 32))
    set_value(wa, 1, 777, 2)                   # part 0
    set_value(wb, 2, (1 << 20) + 12345, 1)     # part 1
    T = 9 * S
    assert T == 18874368 and T > 1 << 24
    want = np.full((3, 3), T, dtype=np.int64)
    want[1, :] -= 3
    want[:, 2] -= 6
    a, b = Dosage(lib, None, words=wa, n_samples=S), Dosage(lib, None, words=wb, n_samples=S)
    try:
        check_square(a, b, want)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------ 5. the split: missing, nobs
SPLIT_N = (2, 129, 257)
SPLIT_S = (1, 31, 33, 257, 1025)


@pytest.fixture(scope="module")
def split_values():
    """257 rows of codes 0 .. 3 at 30 % missing per S, their missing counts and shared-sample counts: computed once"""
    out = {}
    for S in SPLIT_S:
        rng = np.random.default_rng(5000 + S)
        X = rng.integers(0, 3, size=(257, S), dtype=np.uint8)
        X[rng.random((257, S)) < 0.3] = 3
        m = (X != 3).astype(np.int64)
        out[S] = (X, (X == 3).sum(axis=1), m @ m.T)
    return out


@pytest.mark.parametrize("S", SPLIT_S)
@pytest.mark.parametrize("n", SPLIT_N)
def test_row_missing_and_shared_sample_counts_against_numpy(lib, split_values, n, S):
    X, miss, N = split_values[S]
    d = Complete(lib, X[:n])
    try:
        assert np.array_equal(d.missing(), miss[:n])
        check_triangle(d.nobs_host(), d.nobs_device(), n, N[:n, :n])
    finally:
        d.close()


@pytest.mark.parametrize("S", [33, 257])
def test_a_row_of_all_3s_shares_no_sample_with_anybody(lib, S):
    """every bit of the row's data words is set: a tail sample of the last word or a pad word counted as present would show
    as N > 0; the other rows are complete, so N = S among them"""
    n = 130
    X = np.random.default_rng(S).integers(0, 3, size=(n, S), dtype=np.uint8)
    X[0] = X[77] = X[129] = 3
    N = np.full((n, n), S, dtype=np.int64)
    for i in (0, 77, 129):
        N[i, :] = N[:, i] = 0
    d = Complete(lib, X)
    try:
        miss = d.missing()
        assert miss.tolist() == [S if i in (0, 77, 129) else 0 for i in range(n)]
        check_triangle(d.nobs_host(), d.nobs_device(), n, N)
    finally:
        d.close()


# ------------------------------------------------------------------------------------------ 6. correlations
def check_complete(d, want, nan, upper, min_finite_share=None):
    """both measures in both forms against the float64 reference: windows, NaN pattern, 1 ulp, r squared against r^2"""
    n = d.n
    got = {}
    for measure in (0, 1):
        host, dev = d.complete_host(measure), d.complete_device(measure)
        for bits, name, below, outside in ((host, "host", 0, HOST_FILL_BITS), (dev, "device", SENTINEL, SENTINEL)):
            inside = np.zeros(bits.shape, dtype=bool)
            inside[:n, :n] = True
            assert (bits[~inside] == outside).all(), (name, measure)
            assert (bits[:n, :n][~upper] == below).all(), (name, measure)
        h, v = host[:n, :n], dev[:n, :n]
        assert np.array_equal(h[upper], v[upper]), measure                              # bit-identical forms
        is_nan = (h & 0x7FFFFFFF) > 0x7F800000
        assert np.array_equal(is_nan & upper, nan & upper), (measure, np.argwhere((is_nan != nan) & upper)[:5].tolist())
        assert (h[nan & upper] == NAN_BITS).all(), measure
        ok = upper & ~nan
        if min_finite_share is not None:
            assert ok.sum() >= min_finite_share * upper.sum()
        ulps = np.abs(ordered(h[ok]) - ordered(want[measure][ok].astype(np.float32).view(np.uint32)))
        print(f"measure {measure}: worst error {int(ulps.max())} ulp over {int(ok.sum())} entries")
        assert int(ulps.max()) <= 1, (measure, int(ulps.max()), np.argwhere(ok)[np.argmax(ulps)].tolist())
        got[measure] = h
    ok = upper & ~nan
    r = got[1][ok].view(np.float32).astype(np.float64)
    squared = (r * r).astype(np.float32).view(np.uint32)
    apart = np.abs(ordered(squared) - ordered(got[0][ok]))
    print(f"r squared against r^2: at most {int(apart.max())} ulp apart")
    assert int(apart.max()) <= 2
    return got


@pytest.fixture(scope="module")
def genotypes_with_missing():
    """tests/test_gpu_dosage.py's generator of `genotypes` at seed 2025 (200 variants x 1000 samples, neighbours correlated,
    rows 17 / 128 / 199 constant), per-row missing rates uniform in [0, 0.2], and the special rows:
      3 complete; 40 all missing; 41 one observed sample; 60 / 61 present on complementary samples (N = 0);
      62 = 1 except 2 on samples 0 - 99 and complete, 63 missing exactly there: 62 is constant on what they share (NaN for
      that pair only).
    The float64 numpy values of r^2 and r over the samples both rows have, once."""
    rng = np.random.default_rng(2025)
    n, S = 200, 1000
    G = np.zeros((n, S), dtype=np.uint8)
    for i in range(n):
        fresh = rng.binomial(2, rng.uniform(0.05, 0.5), size=S).astype(np.uint8)
        G[i] = np.where(rng.random(S) < 0.6, G[i - 1], fresh) if i and i % 10 else fresh
    for i, v in {17: 0, 128: 1, 199: 2}.items():
        G[i] = v
    X = G.copy()
    rates = rng.uniform(0.0, 0.2, size=n)
    X[rng.random((n, S)) < rates[:, None]] = 3
    X[3] = G[3]
    X[40] = 3
    X[41] = 3
    X[41, 500] = 2
    X[60], X[61] = np.where(np.arange(S) % 2 == 0, G[60], 3), np.where(np.arange(S) % 2 == 1, G[61], 3)
    X[62] = 1
    X[62, :100] = 2
    X[63, :100] = 3
    X[63, 100:] = G[63, 100:]
    want, nan, num = complete_reference(X)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    N = complete_sums(X)[0]
    assert N[60, 61] == 0 and (N[40] == 0).all() and N[41].max() == 1 and N[3, 62] == S
    assert nan[62, 63] and not nan[62, :62].all() and (~nan[62, 64:]).sum() > 100 and (~nan[63, 64:]).sum() > 100
    assert (~nan & upper).sum() >= 0.9 * upper.sum()                          # the result is not hollow
    assert (num[upper & ~nan] < 0).sum() > 1000 and (num[upper & ~nan] > 0).sum() > 1000
    # what reading 3 as a value would cost: r^2 more than 1e-3 away on a large share of the pairs
    x = X.astype(np.int64)
    Pv, s, q = x @ x.T, x.sum(axis=1), (x * x).sum(axis=1)
    dv = S * q - s * s
    both = upper & ~nan & (dv[:, None] != 0) & (dv[None, :] != 0)
    naive = (S * Pv - s[:, None] * s[None, :]).astype(np.float64) ** 2 / np.where(both, dv[:, None] * dv[None, :], 1)
    assert (np.abs(naive - want[0])[both] > 1e-3).mean() > 0.2
    return X, want, nan, upper


def test_pairwise_complete_r_and_r2(lib, genotypes_with_missing):
    """NaN exactly where numpy's dx or dy is 0 — the all-missing row, the row with one sample, the constant rows, the
    complementary pair, the pair (62, 63) —, at least 90 % of the triangle finite, more than 1000 entries of each sign,
    elsewhere at most 1 ulp from the float64 value under both measures; r squared against r^2 at most 2 ulps (r carries
    half an ulp, squaring makes that sqrt(2) ulps of r^2, the two roundings add half an ulp each: 2.4, so 2 between floats)"""
    X, want, nan, upper = genotypes_with_missing
    d = Complete(lib, X)
    try:
        got = check_complete(d, want, nan, upper, min_finite_share=0.9)
        ok = upper & ~nan
        r = got[1][ok].view(np.float32)
        assert (r < 0).sum() > 1000 and (r > 0).sum() > 1000
        N = complete_sums(X)[0]
        check_triangle(d.nobs_host(), d.nobs_device(), d.n, N)
        assert np.array_equal(d.missing(), (X == 3).sum(axis=1))
    finally:
        d.close()


# ------------------------------------------------------------------------------------------ 7. identity
def test_without_missing_genotypes_the_bits_are_pairw_corr_s(lib, genotypes):  # noqa: F811
    """tests/test_gpu_dosage.py's complete data: pairw_corr_complete equals pairw_corr bit for bit (NaNs included) under both
    measures and in both forms, and every pair shares all S samples"""
    G, _, nan, upper = genotypes
    n, S = G.shape
    d = Complete(lib, G)
    try:
        for measure in (0, 1):
            old = d.corr_host(measure)[:n, :n]
            host, dev = d.complete_host(measure)[:n, :n], d.complete_device(measure)[:n, :n]
            assert np.array_equal(host[upper], old[upper]) and np.array_equal(dev[upper], old[upper]), measure
            assert (host[~upper] == 0).all() and (dev[~upper] == SENTINEL).all()
            assert np.array_equal((host == NAN_BITS) & upper, nan & upper)
        check_triangle(d.nobs_host(), d.nobs_device(), n, np.full((n, n), S, dtype=np.int64))
        assert (d.missing() == 0).all()
    finally:
        d.close()


# ------------------------------------------------------------------------------------------ 8. Python
def test_python_class_end_to_end():
    import torch
    n, S = 129, 257
    rng = np.random.default_rng(9)
    X = rng.integers(0, 3, size=(n, S), dtype=np.uint8)
    X[rng.random((n, S)) < 0.15] = 3
    X[5] = 3
    d = sb.StormDosage(S)
    for i in range(64):
        d.add(X[i])
    d.add_packed(pack(X[64:]))
    other = sb.StormDosage(S)
    other.add_packed(pack(X[:7]))
    x = X.astype(np.int64)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    # the rectangle: 3 is a value
    sq = d.square_dot(other)
    assert sq.dtype == np.uint32 and sq.shape == (n, 7) and np.array_equal(sq, x @ x[:7].T)
    t = torch.full((n + 2, 9), -1, dtype=torch.int32, device="cuda:0")
    assert d.square_dot(other, device=t) is None
    t = t.cpu().numpy()
    assert np.array_equal(t[:n, :7], x @ x[:7].T) and (t[n:] == -1).all() and (t[:, 7:] == -1).all()
    with pytest.raises(RuntimeError):
        d.square_dot(sb.StormDosage(S + 1))         # (empty, but the sample counts are compared first)
    # missing genotypes
    N = complete_sums(X)[0]
    assert np.array_equal(d.row_missing(), (X == 3).sum(axis=1))
    nobs = d.pairw_nobs()
    assert nobs.dtype == np.uint32 and np.array_equal(nobs, np.where(upper, N, 0))
    t = torch.full((n + 2, n + 7), -1, dtype=torch.int32, device="cuda:0")
    assert d.pairw_nobs(device=t) is None
    t = t.cpu().numpy()
    assert np.array_equal(t[:n, :n][upper], N[upper]) and (t[:n, :n][~upper] == -1).all() and (t[n:] == -1).all() and \
        (t[:, n:] == -1).all()
    want, nan, _ = complete_reference(X)
    r2, r = d.pairw_corr_complete("r2"), d.pairw_corr_complete("r")
    assert r2.dtype == np.float32 and np.isnan(r2[5, 6:]).all() and np.isnan(r2[:5, 5]).all() and (r2[~upper] == 0).all()
    assert np.array_equal(np.isnan(r) & upper, nan & upper) and np.array_equal(np.isnan(r2) & upper, nan & upper)
    ok = upper & ~nan
    assert ok.sum() > 0.9 * upper.sum()
    assert np.abs(ordered(r.view(np.uint32)[ok]) - ordered(want[1].astype(np.float32).view(np.uint32)[ok])).max() <= 1
    assert np.abs(ordered(r2.view(np.uint32)[ok]) - ordered(want[0].astype(np.float32).view(np.uint32)[ok])).max() <= 1
    f = torch.full((n, n + 1), HOST_FILL, dtype=torch.float32, device="cuda:0")
    d.pairw_corr_complete("r", device=f)
    f = f.cpu().numpy()
    assert np.array_equal(f[:, :n].view(np.uint32)[upper], r.view(np.uint32)[upper]) and (f[:, :n][~upper] == HOST_FILL).all() and \
        (f[:, n] == HOST_FILL).all()
    d.free()
    other.free()
