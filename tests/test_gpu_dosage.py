"""Rows of 2-bit dosages on the device (storm.h: STORM_dosage_*): per-pair dot products from K2h in its dosage form
(tile128_kernel<false, 2>: two classes per nibble at block scale 128), the rows' sums, and the genotype correlations r and
r^2 finished in place. Everything goes through the C-ABI, in the host and the _device forms.

The reference for the dot products P is numpy, `G.astype(int64) @ G.T` on the unpacked values: it shares nothing with the
library or the oracle. P must be EQUAL. Correlations are compared with their float64 numpy value: NaN (0x7FC00000)
exactly against a constant row, elsewhere at most 1 float32 ulp (tests/test_dosage_math.py derives the bound on the CPU).
Device outputs are pre-filled with a sentinel and have ld > n: nothing outside the n x n window, and nothing at i >= j
inside it, may change."""
import ctypes as C

import numpy as np
import pytest

import stormbitmaps_amd as sb
from stormbitmaps_amd import dist

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC00000
SENTINEL = 0xDEADBEEF
SENTINEL_I32 = int(np.uint32(SENTINEL).view(np.int32))
WEIGHT = 9 * 256


# ------------------------------------------------------------------------------------------ helpers
def pack(G):
    """[n, S] values 0 .. 3 -> [n, ceil(S / 32)] uint64: sample s in bits 2 (s % 32), 2 (s % 32) + 1 of word s / 32"""
    n, S = G.shape
    v = np.zeros((n, (S + 31) // 32 * 32), dtype=np.uint64)
    v[:, :S] = G
    return (v.reshape(n, -1, 32) << (np.arange(32, dtype=np.uint64) * np.uint64(2))).sum(axis=2, dtype=np.uint64)


def ordered(bits):
    i = np.asarray(bits).astype(np.int64)
    return np.where(i & 0x80000000, -(i & 0x7FFFFFFF), i)


class Dosage:
    """a STORM_dosage_t filled from G [n, S]: even rows through STORM_dosage_add, odd rows through STORM_dosage_add_packed"""

    def __init__(self, lib, G, packed_only=False, words=None, n_samples=None):
        """words (with n_samples): rows that are packed already, G is not read"""
        self.lib = lib
        self.n, self.S = (int(G.shape[0]), int(G.shape[1])) if words is None else (int(words.shape[0]), n_samples)
        self.h = lib.STORM_dosage_new(self.S)
        assert self.h
        if words is not None or packed_only:
            words = pack(np.ascontiguousarray(G, dtype=np.uint8)) if words is None else np.ascontiguousarray(words)
            assert lib.STORM_dosage_add_packed(self.h, words.ctypes.data, self.n) == 0
        else:
            G = np.ascontiguousarray(G, dtype=np.uint8)
            for i in range(self.n):
                if i % 2 == 0:
                    assert lib.STORM_dosage_add(self.h, G[i].ctypes.data, self.S) == 0
                else:
                    w = pack(G[i:i + 1])
                    assert lib.STORM_dosage_add_packed(self.h, w.ctypes.data, 1) == 0
        assert lib.STORM_dosage_n_rows(self.h) == self.n

    def ok(self, rc, what):
        assert rc == 0, (what, rc, self.lib.STORM_hip_error())

    def dot_host(self, ld=None):
        n = self.n
        ld = n + 3 if ld is None else ld
        out = np.full((n + 1, ld), SENTINEL, dtype=np.uint32)
        self.ok(self.lib.STORM_dosage_pairw_dot(self.h, out.ctypes.data, n + 1, ld), "STORM_dosage_pairw_dot")
        return out

    def _device(self, call):
        import torch
        n = self.n
        ld = n + 5
        buf = torch.full(((n + 1) * ld,), SENTINEL_I32, dtype=torch.int32, device="cuda:0")
        self.ok(call(buf.data_ptr(), n + 1, ld), "device form")
        return buf.cpu().numpy().view(np.uint32).reshape(n + 1, ld)

    def dot_device(self):
        return self._device(lambda p, rows, ld: self.lib.STORM_dosage_pairw_dot_device(self.h, C.c_void_p(p), rows, ld))

    def corr_host(self, measure):
        n = self.n
        out = np.full((n + 1, n + 3), -7.5, dtype=np.float32)
        self.ok(self.lib.STORM_dosage_pairw_corr(self.h, measure, out.ctypes.data, n + 1, n + 3), "STORM_dosage_pairw_corr")
        return out.view(np.uint32)

    def corr_device(self, measure):
        return self._device(lambda p, rows, ld: self.lib.STORM_dosage_pairw_corr_device(self.h, measure, C.c_void_p(p), rows, ld))

    def row_sums(self):
        s = np.full(self.n + 1, SENTINEL, dtype=np.uint32)
        q = np.full(self.n + 1, SENTINEL, dtype=np.uint32)
        self.ok(self.lib.STORM_dosage_row_sums(self.h, s.ctypes.data, q.ctypes.data), "STORM_dosage_row_sums")
        assert s[self.n] == SENTINEL and q[self.n] == SENTINEL
        return s[:self.n], q[:self.n]

    def close(self):
        if self.h:
            self.lib.STORM_dosage_free(self.h)
            self.h = None


def check_dot(d, want):
    """host and _device forms of the dot products against `want` [n, n] (int64, full matrix): exact at i < j; host zeros at
    i >= j; the device's i >= j and everything outside the n x n window of either output untouched"""
    n = d.n
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    host, dev = d.dot_host(), d.dot_device()
    for got, name in ((host, "host"), (dev, "device")):
        inside = np.zeros(got.shape, dtype=bool)
        if n >= 2:
            inside[:n, :n] = True
        assert (got[~inside] == SENTINEL).all(), (name, n, d.S, np.argwhere(~inside & (got != SENTINEL))[:5].tolist())
        if n >= 2:
            win = got[:n, :n].astype(np.int64)
            bad = np.argwhere((win != want) & upper)
            assert bad.size == 0, (name, n, d.S, bad[:5].tolist(), [(int(win[i, j]), int(want[i, j])) for i, j in bad[:5]])
            assert (got[:n, :n][~upper] == (0 if name == "host" else SENTINEL)).all(), (name, n, d.S)


def numpy_dot(G):
    G = G.astype(np.int64)
    return G @ G.T


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


# ------------------------------------------------------------------------------------------ 1, 7. edges; row sums
EDGE_N = (1, 2, 127, 128, 129, 257)
EDGE_S = (1, 31, 32, 33, 255, 256, 257, 1023, 1025)


@pytest.fixture(scope="module")
def edge_values():
    """257 rows of seeded values 0 .. 3 per S, and their numpy products: computed once"""
    out = {}
    for S in EDGE_S:
        G = np.random.default_rng(1000 + S).integers(0, 4, size=(257, S), dtype=np.uint8)
        out[S] = (G, numpy_dot(G))
    return out


@pytest.mark.parametrize("S", EDGE_S)
@pytest.mark.parametrize("n", EDGE_N)
def test_dot_products_at_the_row_and_sample_edges(lib, edge_values, n, S):
    """1 and 2 rows, either side of the 128-row tile, three tiles with a ragged last one; samples either side of the 32-value
    word and the 256-value chunk, one chunk short by one value, four chunks and one value"""
    G, P = edge_values[S]
    d = Dosage(lib, G[:n])
    try:
        check_dot(d, P[:n, :n])
    finally:
        d.close()


@pytest.mark.parametrize("S", EDGE_S)
@pytest.mark.parametrize("n", EDGE_N)
def test_row_sums_against_numpy(lib, edge_values, n, S):
    G = edge_values[S][0][:n].astype(np.int64)
    d = Dosage(lib, G)
    try:
        s, q = d.row_sums()
        assert np.array_equal(s, G.sum(axis=1)) and np.array_equal(q, (G * G).sum(axis=1))
    finally:
        d.close()


# ------------------------------------------------------------------------------------------ 2. position probes
@pytest.mark.parametrize("value", [1, 2, 3])
def test_a_single_sample_is_multiplied_only_with_itself(lib, value):
    """rows with ONE non-zero sample at the positions where a class, a word, a 16-byte slot or a chunk changes: P(i, j) is
    v_i v_j where the positions are equal and 0 elsewhere — a class or swizzle mix-up inside a chunk shows here. Every
    position appears in three rows (values `value`, 1 and 3), so equal positions are multiplied as well."""
    S = 1025
    positions = [0, 1, 2, 31, 32, 63, 64, 255, 256, 511, 512, S - 1]
    rows = [(p, v) for p in positions for v in (value, 1, 3)]
    G = np.zeros((len(rows), S), dtype=np.uint8)
    for i, (p, v) in enumerate(rows):
        G[i, p] = v
    want = np.array([[vi * vj if pi == pj else 0 for (pj, vj) in rows] for (pi, vi) in rows], dtype=np.int64)
    assert np.array_equal(want, numpy_dot(G))
    d = Dosage(lib, G)
    try:
        check_dot(d, want)
    finally:
        d.close()


# ------------------------------------------------------------------------------------------ 3. parity rows
def test_even_and_odd_samples_do_not_leak_into_each_other(lib):
    """even samples are class 0 of a nibble, odd samples class 1: A = 1 on even samples, B = 2 on odd, C = 3 on even, D = 3 on
    odd, E = 1 everywhere. Closed forms with S = 1000 (500 even, 500 odd samples)."""
    S = 1000
    even = (np.arange(S) % 2 == 0).astype(np.uint8)
    A, B, Cc, D, E = even, 2 * (1 - even), 3 * even, 3 * (1 - even), np.ones(S, dtype=np.uint8)
    G = np.stack([A, B, Cc, D, E]).astype(np.uint8)
    ev, od = (S + 1) // 2, S // 2
    want = np.array([[1 * ev, 0, 3 * ev, 0, ev],
                     [0, 4 * od, 0, 6 * od, 2 * od],
                     [3 * ev, 0, 9 * ev, 0, 3 * ev],
                     [0, 6 * od, 0, 9 * od, 3 * od],
                     [ev, 2 * od, 3 * ev, 3 * od, S]], dtype=np.int64)
    assert np.array_equal(want, numpy_dot(G))
    d = Dosage(lib, G)
    try:
        check_dot(d, want)
    finally:
        d.close()


# ------------------------------------------------------------------------------------------ 4. window limits
def planned(hip_ctx, n_rows, S, min_chunks):
    """what the device launches for these options, from the planner itself (the device's CU count, default slots and cost)"""
    return dist.dosage_plan(n_rows, (S + 31) // 32, n_cus=hip_ctx.get_option("n_cus"), slots_per_cu=0, min_chunks=min_chunks,
                            diag_cost_pct=80)


@pytest.mark.parametrize("S,min_chunks,narrow_planned", [(14848, 29, 0), (14336, 28, 1)])
@pytest.mark.parametrize("narrow_option", [1, 0])
def test_sixteen_bit_windows_stop_where_a_part_could_overflow_them(lib, hip_ctx, options, S, min_chunks, narrow_planned,
                                                                   narrow_option):
    """130 rows of all 3s: every product is 9, the most a part can hold. (a) S = 14848 = 58 chunks as two parts of 29: a part
    sums to 66816, beyond 16 bits — the planner must give wide windows (a bit-weighted rule, narrow up to 127 chunks, would
    wrap every entry by 65536 per part). (b) S = 14336 = 56 chunks as two parts of 28: 64512 per part, just inside — narrow
    windows. (c) both again with k2_part_narrow = 0. The plan is asserted as well as the result, so that a planner change
    cannot hollow the test silently."""
    n = 130
    plan = planned(hip_ctx, n, S, min_chunks)
    assert len(plan) == 6 and (plan[:, 6] == 2).all() and (plan[:, 3] == min_chunks).all(), plan.tolist()
    assert (plan[:, 7] == narrow_planned).all(), plan.tolist()
    assert (min_chunks * WEIGHT > 65535) == (narrow_planned == 0)
    options(k2_part_min_chunks=min_chunks, k2_part_narrow=narrow_option)
    G = np.full((n, S), 3, dtype=np.uint8)
    d = Dosage(lib, G, packed_only=True)
    try:
        check_dot(d, np.full((n, n), 9 * S, dtype=np.int64))
        assert 9 * S == {14848: 133632, 14336: 129024}[S]
    finally:
        d.close()


# ------------------------------------------------------------------------------------------ 5. long k
def test_rows_of_2_pow_21_samples_are_summed_exactly_across_parts(lib, hip_ctx, options):
    """3 rows of S = 2^21 samples, all 3s except one sample of 2 in row 1 (in the first half of k) and one sample of 1 in
    row 2 (in the second half): with T = 9 S = 18874368,
        P(0, 1) = T - 9 + 6 = T - 3,   P(0, 2) = T - 9 + 3 = T - 6,   P(1, 2) = T - 18 + 6 + 3 = T - 9
    — odd and even values above 2^24 that an f32 sum across the parts would round (T - 3 and T - 9 are odd). 8192 chunks
    x 2304 exceed 2^24, so the planner must cut every tile; k2_part_min_chunks = 4096 makes that two parts of 4096 chunks,
    asserted from the plan. The option's range caps a forced part at 4096 chunks; the single-item limit of 7281 chunks cannot
    be forced on a 256-CU device without a matrix of gigabytes: that limit is tests/test_dosage_plan.py's."""
    S = 1 << 21
    plan = planned(hip_ctx, 3, S, 4096)
    assert len(plan) == 2 and (plan[:, 6] == 2).all() and (plan[:, 3] == 4096).all() and (plan[:, 7] == 0).all(), plan.tolist()
    options(k2_part_min_chunks=4096)
    words = np.full((3, S // 32), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)

    def set_value(row, s, v):
        words[row, s // 32] &= ~(np.uint64(3) << np.uint64(2 * (s % 32)))
        words[row, s // 32] |= np.uint64(v) << np.uint64(2 * (s % 32))
    set_value(1, 777, 2)                   # chunk 3 of part 0
    set_value(2, (1 << 20) + 12345, 1)     # part 1
    T = 9 * S
    assert T == 18874368
    want = np.zeros((3, 3), dtype=np.int64)
    want[0, 1], want[0, 2], want[1, 2] = T - 3, T - 6, T - 9
    d = Dosage(lib, None, words=words, n_samples=S)
    try:
        check_dot(d, want + want.T)
        s, q = d.row_sums()
        assert s.tolist() == [3 * S, 3 * S - 1, 3 * S - 2] and q.tolist() == [T, T - 5, T - 8]
    finally:
        d.close()


# ------------------------------------------------------------------------------------------ 6. correlation
@pytest.fixture(scope="module")
def genotypes():
    """200 variants x 1000 samples: dosages 0 / 1 / 2 drawn at seeded allele frequencies in [0.05, 0.5], neighbouring
    variants correlated (a variant copies most samples of the one before, as LD does), and three constant rows (all 0, all
    1, all 2). The float64 numpy values of r and r^2, once."""
    rng = np.random.default_rng(2024)
    n, S = 200, 1000
    G = np.zeros((n, S), dtype=np.uint8)
    for i in range(n):
        fresh = rng.binomial(2, rng.uniform(0.05, 0.5), size=S).astype(np.uint8)
        G[i] = np.where(rng.random(S) < 0.6, G[i - 1], fresh) if i and i % 10 else fresh
    constant = {17: 0, 128: 1, 199: 2}
    for i, v in constant.items():
        G[i] = v
    g = G.astype(np.int64)
    P, s, q = g @ g.T, g.sum(axis=1), (g * g).sum(axis=1)
    num = S * P - s[:, None] * s[None, :]
    dd = S * q - s * s
    nan = (dd[:, None] == 0) | (dd[None, :] == 0)
    assert sorted(np.flatnonzero(dd == 0).tolist()) == sorted(constant)       # no other row came out constant
    den = np.where(nan, 1, dd[:, None] * dd[None, :]).astype(np.float64)
    r2 = (num.astype(np.float64) ** 2) / den
    r = num.astype(np.float64) / np.sqrt(den)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    assert (~nan & upper).sum() >= 0.9 * upper.sum()                          # the result is not hollow
    assert (num[upper & ~nan] < 0).sum() > 1000 and (num[upper & ~nan] > 0).sum() > 1000
    return G, {0: r2, 1: r}, nan, upper


def test_correlations_r_and_r2(lib, genotypes):
    """both measures in the host and the _device form: NaN (0x7FC00000) exactly in the constant rows and columns, elsewhere at
    most 1 ulp from the float64 numpy value; the two forms bit-identical; at least 90 % of the triangle finite. r squared
    against r^2: r carries at most half an ulp, which squaring turns into at most sqrt(2) ulps of r^2; rounding the square and
    r^2 itself add half an ulp each: 2.4 ulps between two float32 values, that is at most 2."""
    G, want, nan, upper = genotypes
    n = G.shape[0]
    d = Dosage(lib, G)
    try:
        got = {}
        for measure in (0, 1):
            host, dev = d.corr_host(measure), d.corr_device(measure)
            for bits, name, below in ((host, "host", 0), (dev, "device", SENTINEL)):
                inside = np.zeros(bits.shape, dtype=bool)
                inside[:n, :n] = True
                outside = int(np.float32(-7.5).view(np.uint32)) if name == "host" else SENTINEL
                assert (bits[~inside] == outside).all(), (name, measure)
                assert (bits[:n, :n][~upper] == below).all(), (name, measure)
            h, v = host[:n, :n], dev[:n, :n]
            assert np.array_equal(h[upper], v[upper]), measure                              # bit-identical forms
            is_nan = (h & 0x7FFFFFFF) > 0x7F800000
            assert np.array_equal(is_nan & upper, nan & upper), measure
            assert (h[nan & upper] == NAN_BITS).all(), measure
            ok = upper & ~nan
            assert ok.sum() >= 0.9 * upper.sum()
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
        assert (got[1][ok].view(np.float32) < 0).sum() > 1000                                # the sign of r is kept
    finally:
        d.close()


# ------------------------------------------------------------------------------------------ 8. Python
def test_python_class_end_to_end():
    import torch
    n, S = 129, 257
    G = np.random.default_rng(8).integers(0, 3, size=(n, S), dtype=np.uint8)
    G[5] = 1
    d = sb.StormDosage(S)
    for i in range(64):
        d.add(G[i])
    d.add_packed(pack(G[64:]))
    assert d.n_rows == n
    g = G.astype(np.int64)
    P = g @ g.T
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    s, q = d.row_sums()
    assert np.array_equal(s, g.sum(axis=1)) and np.array_equal(q, (g * g).sum(axis=1))
    dot = d.pairw_dot()
    assert dot.dtype == np.uint32 and np.array_equal(dot, np.where(upper, P, 0))
    t = torch.full((n + 2, n + 7), -1, dtype=torch.int32, device="cuda:0")
    assert d.pairw_dot(device=t) is None
    t = t.cpu().numpy()
    assert np.array_equal(t[:n, :n][upper], P[upper]) and (t[:n, :n][~upper] == -1).all() and (t[n:] == -1).all() and \
        (t[:, n:] == -1).all()
    r2, r = d.pairw_corr("r2"), d.pairw_corr("r")
    assert r2.dtype == np.float32 and np.isnan(r2[5, 6:]).all() and np.isnan(r2[:5, 5]).all() and (r2[~upper] == 0).all()
    num = S * P - s.astype(np.int64)[:, None] * s.astype(np.int64)[None, :]
    dd = S * q.astype(np.int64) - s.astype(np.int64) ** 2
    ok = upper & (dd[:, None] != 0) & (dd[None, :] != 0)
    ref = num.astype(np.float64) / np.sqrt(np.where(ok, dd[:, None] * dd[None, :], 1).astype(np.float64))
    assert np.abs(ordered(r.view(np.uint32)[ok]) - ordered(ref.astype(np.float32).view(np.uint32)[ok])).max() <= 1
    assert np.abs(ordered(r2.view(np.uint32)[ok]) - ordered((ref * ref).astype(np.float32).view(np.uint32)[ok])).max() <= 1
    f = torch.full((n, n + 1), -7.5, dtype=torch.float32, device="cuda:0")
    d.pairw_corr("r", device=f)
    f = f.cpu().numpy()
    assert np.array_equal(f[:, :n].view(np.uint32)[upper], r.view(np.uint32)[upper]) and (f[:, :n][~upper] == -7.5).all() and \
        (f[:, n] == -7.5).all()
    d.clear()
    assert d.n_rows == 0
    d.free()
