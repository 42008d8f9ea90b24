"""Stratified LD scores in a distance window on the device (storm.h: STORM_dosage_lag_ldscore_annot, _annot_complete and their
_device forms; storm_hip.h: storm_hip_lag_band_annot_sums_device): the band of r^2 the lag calls write times an annotation
matrix, with a window per row, reduced by lag_band_annot_sums_kernel. Everything goes through the C-ABI
(StormDosage.lag_ldscore_annot, HipContext.lag_band_annot_sums_device), in the host and the _device forms.

Expected values: the counts EXACTLY and the scores within tests/_ldscore_annot.py's derived bound — ulp32(ref) + 2^-36 (sum
|t a| + m max |a|), which a float accumulation does not meet — from the library's own pairw_lag_corr[_complete] host matrix
(and pairw_lag_nobs), reduced in numpy with math.fsum; once, independently of that matrix, against np.corrcoef on the
unpacked dosages; against the plain lag_ldscore call; bit for bit on one-hot columns. Every row and every column is checked.
Shapes: the 64-row block edge and the 64-row tile edge on both sides, L clipped to n - 1, many blocks; columns: 1, 63, 64,
65 and 130 (the 64-column chunk edge)."""
import numpy as np
import pytest

import stormbitmaps_amd as sb
from tests import _ldscore, _ldscore_annot
from tests._ldscore import ADJ, R2
from tests.test_gpu_ldscore import lag_of, rows_of

pytestmark = pytest.mark.gpu

SHAPES = [(2, 40, 1), (65, 96, 64), (130, 257, 63), (130, 257, 65), (200, 1000, 129), (300, 4099, 10000), (1100, 64, 17)]
STATS = {"r2": R2, "r2_adj": ADJ}
COLS = 130                                                                         # two full chunks of 64 columns and 2 more
COLUMN_COUNTS = (1, 63, 64, 65, 130)
GUARD = 3                                                                          # rows behind n of a device output
GUARD_F, GUARD_I = -77.5, 0x5EADBEEF


def annotations(n, seed):
    """[n, 130] random normal floats, some exact zeros, half of them negative"""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, COLS)).astype(np.float32)
    a[rng.random((n, COLS)) < 0.1] = 0.0
    return a


class Case:
    """one container per (shape, kind), its annotations, and what the library itself says about its pairs: fetched once,
    never modified"""

    def __init__(self, n, S, max_lag, kind):
        self.n, self.S, self.max_lag, self.kind, self.L = n, S, max_lag, kind, lag_of(n, max_lag)
        self.complete = kind == "missing"
        self.G = rows_of(n, S, kind)
        self.annot = annotations(n, 7 * n + S)
        self.annot.setflags(write=False)
        self.d = sb.StormDosage(S)
        for row in self.G:
            self.d.add(row)
        self._memo = {}

    def memo(self, key, make):
        if key not in self._memo:
            v = make()
            for a in (v if isinstance(v, tuple) else (v,)):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._memo[key] = v
        return self._memo[key]

    def band(self, max_lag=None):
        """the library's own float matrix in the lag layout (host form)"""
        max_lag = self.max_lag if max_lag is None else max_lag
        f = self.d.pairw_lag_corr_complete if self.complete else self.d.pairw_lag_corr
        return self.memo(("band", max_lag), lambda: f(max_lag, "r2"))

    def nobs(self, max_lag=None):
        max_lag = self.max_lag if max_lag is None else max_lag
        return self.memo(("nobs", max_lag), lambda: self.d.pairw_lag_nobs(max_lag))

    def reference(self, stat, max_lag=None, lo=None, hi=None, cols=slice(None), key=None):
        max_lag = self.max_lag if max_lag is None else max_lag

        def make():
            if self.complete:
                return _ldscore_annot.annot_sums(self.band(max_lag), self.n, max_lag, STATS[stat], self.annot[:, cols],
                                                 nobs=self.nobs(max_lag), lo=lo, hi=hi)
            return _ldscore_annot.annot_sums(self.band(max_lag), self.n, max_lag, STATS[stat], self.annot[:, cols], n_const=self.S,
                                             lo=lo, hi=hi)
        return self.memo(("ref", stat, max_lag, key), make) if (lo is None or key) and cols == slice(None) else make()

    def host(self, stat):
        """the host form over all 130 columns, the count window"""
        return self.memo(("host", stat), lambda: self.d.lag_ldscore_annot(self.annot, self.max_lag, stat, complete=self.complete))


_cases = {}


def case(n, S, max_lag, kind):
    key = (n, S, max_lag, kind)
    if key not in _cases:
        _cases[key] = Case(*key)
    return _cases[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------ 1: against the restatement
@pytest.mark.parametrize("stat", ["r2", "r2_adj"])
@pytest.mark.parametrize("kind", ["plain", "const", "missing"])
@pytest.mark.parametrize("n,S,max_lag", SHAPES)
def test_counts_and_scores_against_the_restatement(n, S, max_lag, kind, stat):
    """plain rows; constant rows at 0, 63, 64 and n - 1 (their pairs are NaN); 10 % missing values with the N = 2 and N = 3
    pairs of tests/test_gpu_ldscore.py through the pairwise-complete call"""
    c = case(n, S, max_lag, kind)
    score, pairs = c.host(stat)
    assert score.shape == (n, COLS) and pairs.shape == (n,)
    ref, sum_abs, m, a_max = c.reference(stat)
    _ldscore_annot.assert_scores(score, pairs, ref, sum_abs, m, a_max, (n, S, max_lag, kind, stat))
    if kind == "const":
        for i in {0, 63, 64, n - 1}:
            if i < n:
                assert pairs[i] == 0 and (bits(score[i]) == 0).all(), i            # a constant row: +0.0f in every column
        assert pairs.max() > 0 or n <= 2
    if kind == "plain":
        i = np.arange(n)
        assert np.array_equal(pairs, np.minimum(i, c.L) + np.minimum(n - 1 - i, c.L))   # nothing is NaN: the whole window
    if kind == "missing":
        assert c.nobs()[0, 0] == 2
        if n == 2:
            assert pairs.tolist() == ([1, 1] if stat == "r2" else [0, 0])          # the N = 2 pair is dropped under ADJ
        if n >= 5:
            assert pairs[2] == 0 and (bits(score[2]) == 0).all() and c.nobs()[3, 0] == 3


@pytest.mark.parametrize("inner", ["fma", "mfma"])
@pytest.mark.parametrize("n,S,max_lag,kind", [(65, 96, 64, "const"), (130, 257, 65, "missing"), (200, 1000, 129, "plain"),
                                              (1100, 64, 17, "missing")])
def test_both_inner_products_meet_the_bound(monkeypatch, n, S, max_lag, kind, inner):
    """STORM_HIP_LDSCORE_ANNOT_INNER picks the inner product of the kernel per launch — v_fma_f64 from LDS operands or
    v_mfma_f64_16x16x4_f64: whichever ships, either is inside the restatement's bound, counts exactly, and a column has the
    same bits alone as among 130"""
    c = case(n, S, max_lag, kind)
    monkeypatch.setenv("STORM_HIP_LDSCORE_ANNOT_INNER", inner)
    for stat in STATS:
        score, pairs = c.d.lag_ldscore_annot(c.annot, max_lag, stat, complete=c.complete)
        ref, sum_abs, m, a_max = c.reference(stat)
        _ldscore_annot.assert_scores(score, pairs, ref, sum_abs, m, a_max, (n, S, max_lag, kind, stat, inner))
        alone = c.d.lag_ldscore_annot(c.annot[:, 70:71], max_lag, stat, complete=c.complete)
        assert same_bits(alone[0], score[:, 70:71]) and np.array_equal(alone[1], pairs)


# ------------------------------------------------------------------------------------------ 2: against numpy alone
@pytest.mark.parametrize("n,S,max_lag", [(130, 257, 63), (200, 1000, 129)])
def test_scores_against_corrcoef_on_the_unpacked_dosages(n, S, max_lag):
    """independent of the library's matrix: a swapped direction or a window off by one shows here. Each float r^2 is at
    most one float from the correctly rounded value (storm_dosage_math.h): 2^-23 relative each, so a column's sum is within
    2^-23 sum |r^2 a| of the sum of the exact terms; the one rounding to float and the float64 reference's own error fit
    into as much again plus 2^-22 of ONE annotation's magnitude — tests/test_gpu_ldscore.py's 2^-22 (sum + 1) with the 1
    scaled by max |a|: 2^-22 (sum |r^2 a| + max |a|)"""
    c = case(n, S, max_lag, "plain")
    score, pairs = c.host("r2")
    r2 = np.corrcoef(c.G.astype(np.float64)) ** 2
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    window = (np.abs(i - j) >= 1) & (np.abs(i - j) <= c.L)
    w = np.where(window, r2, 0.0)
    a = c.annot.astype(np.float64)
    want, mag = w @ a, w @ np.abs(a)
    a_max = np.array([np.abs(a[window[r]]).max(axis=0) for r in range(n)])
    assert np.array_equal(pairs, window.sum(axis=1))
    err = np.abs(score.astype(np.float64) - want)
    lim = 2.0 ** -22 * (mag + a_max)
    assert (err <= lim).all(), (np.unravel_index(int(np.argmax(err - lim)), err.shape), float((err / lim).max()))


# ------------------------------------------------------------------------------------------ 3: against the plain call
@pytest.mark.parametrize("stat", ["r2", "r2_adj"])
@pytest.mark.parametrize("kind", ["const", "missing"])
@pytest.mark.parametrize("n,S,max_lag", SHAPES)
def test_a_column_of_ones_is_the_plain_call(n, S, max_lag, kind, stat):
    """pos = NULL and one column of ones: the sums of lag_ldscore in another order of additions — inside the plain call's own
    bound around the plain call's own reference, with the same counts"""
    c = case(n, S, max_lag, kind)
    score, pairs = c.d.lag_ldscore_annot(np.ones((n, 1), dtype=np.float32), max_lag, stat, complete=c.complete)
    plain, plain_pairs = c.d.lag_ldscore(max_lag, stat, complete=c.complete)
    assert np.array_equal(pairs, plain_pairs)
    if c.complete:
        ref, sum_abs, m = _ldscore.band_sums(c.band(), n, max_lag, STATS[stat], nobs=c.nobs())
    else:
        ref, sum_abs, m = _ldscore.band_sums(c.band(), n, max_lag, STATS[stat], n_const=S)
    _ldscore.assert_scores(score[:, 0], pairs, ref, sum_abs, m, (n, S, max_lag, kind, stat))
    _ldscore.assert_scores(plain, plain_pairs, ref, sum_abs, m)
    assert (np.abs(score[:, 0].astype(np.float64) - plain.astype(np.float64)) <= 2 * _ldscore.bound(ref, sum_abs, m)).all()


# ------------------------------------------------------------------------------------------ 4: one-hot columns
@pytest.mark.parametrize("stat", ["r2", "r2_adj"])
@pytest.mark.parametrize("n,S,max_lag,kind", [(130, 257, 63, "plain"), (130, 257, 65, "missing"), (200, 1000, 129, "const"),
                                              (1100, 64, 17, "missing")])
def test_one_hot_columns_give_the_terms_bits(n, S, max_lag, kind, stat):
    """column c is 1 at row j_c alone: score[i, c] has exactly the bits of float(t(i, j_c)) for the rows i of j_c's window
    whose pair is summed and +0.0f elsewhere — a swapped direction or a window off by one cannot hide. j_c: 0, 63, 64,
    n - 1, and the two window edges i - L and i + L of a row i in the middle (and the rows just outside them)"""
    c = case(n, S, max_lag, kind)
    L, mid = c.L, n // 2
    hot = [0, 63, 64, n - 1] + [j for j in (mid - L, mid + L, mid - L - 1, mid + L + 1) if 0 <= j < n]
    annot = np.zeros((n, len(hot)), dtype=np.float32)
    annot[hot, np.arange(len(hot))] = 1.0
    score, pairs = c.d.lag_ldscore_annot(annot, max_lag, stat, complete=c.complete)
    rho = _ldscore.both_sides(c.band(), n, L, np.float32(np.nan)).astype(np.float64)  # [n, 2 L]: ahead, then behind
    N = _ldscore.both_sides(c.nobs().astype(np.int64), n, L, 0) if c.complete else np.full((n, 2 * L), S, dtype=np.int64)
    with np.errstate(all="ignore"):
        t = rho if stat == "r2" else np.where(N >= 3, rho - (1.0 - rho) / (N - 2).astype(np.float64), np.nan)
    want = np.zeros((n, len(hot)), dtype=np.float32)
    for k, j in enumerate(hot):
        for i in range(max(j - L, 0), min(j + L, n - 1) + 1):
            if i != j:
                v = t[i, j - i - 1] if j > i else t[i, L + i - j - 1]
                want[i, k] = 0.0 if np.isnan(v) else np.float32(v)
    assert same_bits(score, want), np.argwhere(bits(score) != bits(want))[:8]
    assert np.array_equal(pairs, c.host(stat)[1])                                  # the counts do not depend on the columns
    if mid - L >= 0:
        assert want[mid, 4] != 0 or kind != "plain"                                # the edge itself is inside the window


# ------------------------------------------------------------------------------------------ 5: positions
@pytest.mark.parametrize("n,S,max_lag,kind,lag", [(130, 257, 65, "plain", 17), (200, 1000, 129, "missing", 64),
                                                  (1100, 64, 17, "const", 1)])
def test_unit_positions_are_the_count_window(n, S, max_lag, kind, lag):
    """pos = 0, 1, 2, .. with max_dist = L' gives the bits of the count-window call at lag L'; max_lag = 0 (None) takes
    the lag the windows need, the exact lag gives the same bits, and one row less is refused with both numbers named"""
    c = case(n, S, max_lag, kind)
    pos = np.arange(n, dtype=np.float64)
    for stat in STATS:
        count = c.d.lag_ldscore_annot(c.annot, lag, stat, complete=c.complete)
        free = c.d.lag_ldscore_annot(c.annot, None, stat, complete=c.complete, pos=pos, max_dist=float(lag))
        exact = c.d.lag_ldscore_annot(c.annot, lag, stat, complete=c.complete, pos=pos, max_dist=lag + 0.5)
        wide = c.d.lag_ldscore_annot(c.annot, lag + 70, stat, complete=c.complete, pos=pos, max_dist=float(lag))
        for got in (free, exact, wide):
            assert same_bits(got[0], count[0]) and np.array_equal(got[1], count[1]), stat
    assert c.d.ldscore_window_lag(pos, float(lag)) == lag
    if lag > 1:
        with pytest.raises(RuntimeError, match=f"lag of {lag} rows, max_lag is {lag - 1}"):
            c.d.lag_ldscore_annot(c.annot, lag - 1, "r2", complete=c.complete, pos=pos, max_dist=float(lag))


HAND_N = 65


def hand_positions():
    """65 rows: twenty at steps of 0.5 (within 2.0: four rows on each side, fewer at the ends — row 19 has four behind and
    none ahead, row 17 four behind and two ahead), two rows alone behind gaps wider than max_dist, then pairs of tied rows
    at steps of 1"""
    pos = np.empty(HAND_N, dtype=np.float64)
    pos[:20] = 0.5 * np.arange(20)
    pos[20], pos[21] = 100.0, 200.0
    pos[22:] = 300.0 + (np.arange(HAND_N - 22) // 2)
    return pos


@pytest.mark.parametrize("kind", ["plain", "missing"])
def test_a_hand_made_position_set(kind):
    n, S, max_lag = 65, 96, 64
    c = case(n, S, max_lag, kind)
    pos, dist = hand_positions(), 2.0
    lo, hi = _ldscore_annot.windows(pos, dist)
    need = _ldscore_annot.window_lag(lo, hi)
    assert (lo[20], hi[20], lo[21], hi[21]) == (20, 20, 21, 21) and (lo[19], hi[19]) == (15, 19) and (lo[17], hi[17]) == (13, 19)
    assert (lo[22], hi[22]) == (22, 27) and (lo[30], hi[30]) == (26, 35) and need == 5      # ties widen the windows: 5 rows
    assert c.d.ldscore_window_lag(pos, dist) == need
    for stat in STATS:
        score, pairs = c.d.lag_ldscore_annot(c.annot, None, stat, complete=c.complete, pos=pos, max_dist=dist)
        ref, sum_abs, m, a_max = c.reference(stat, need, lo, hi)
        _ldscore_annot.assert_scores(score, pairs, ref, sum_abs, m, a_max, (kind, stat))
        for i in (20, 21):
            assert pairs[i] == 0 and (bits(score[i]) == 0).all()                   # an empty window: +0.0f in every column
        if kind == "plain":
            assert np.array_equal(pairs, hi.astype(np.int64) - lo)                 # nothing is NaN: the window but the row
        again = c.d.lag_ldscore_annot(c.annot, need, stat, complete=c.complete, pos=pos, max_dist=dist)
        wide = c.d.lag_ldscore_annot(c.annot, 64, stat, complete=c.complete, pos=pos, max_dist=dist)
        for got in (again, wide):
            assert same_bits(got[0], score) and np.array_equal(got[1], pairs)
        with pytest.raises(RuntimeError, match=f"lag of {need} rows, max_lag is {need - 1}"):
            c.d.lag_ldscore_annot(c.annot, need - 1, stat, complete=c.complete, pos=pos, max_dist=dist)
    everything = c.d.lag_ldscore_annot(c.annot, None, "r2", complete=c.complete, pos=pos, max_dist=np.inf)
    assert same_bits(everything[0], c.host("r2")[0]) and np.array_equal(everything[1], c.host("r2")[1])   # +inf: the whole matrix
    nothing = c.d.lag_ldscore_annot(c.annot, None, "r2", complete=c.complete, pos=np.arange(n), max_dist=0.5)
    assert (bits(nothing[0]) == 0).all() and (nothing[1] == 0).all()               # every window empty


# ------------------------------------------------------------------------------------------ 6: columns, repeatability
@pytest.mark.parametrize("n,S,max_lag,kind", [(65, 96, 64, "const"), (200, 1000, 129, "missing"), (1100, 64, 17, "plain")])
def test_a_column_has_the_same_bits_whatever_is_passed_with_it(n, S, max_lag, kind):
    """columns computed alone, as the first 1, 63, 64 and 65, and within all 130: the same bits; a second call: the same
    bits. (The restatement has checked the 130: every column count is checked through them.)"""
    c = case(n, S, max_lag, kind)
    for stat in STATS:
        full, pairs = c.host(stat)
        again = c.d.lag_ldscore_annot(c.annot, max_lag, stat, complete=c.complete)
        assert same_bits(again[0], full) and np.array_equal(again[1], pairs), stat
        for count in COLUMN_COUNTS:
            got = c.d.lag_ldscore_annot(c.annot[:, :count], max_lag, stat, complete=c.complete)
            assert same_bits(got[0], full[:, :count]) and np.array_equal(got[1], pairs), (stat, count)
        for k in (64, 70, 129):
            alone = c.d.lag_ldscore_annot(c.annot[:, k:k + 1], max_lag, stat, complete=c.complete)
            assert same_bits(alone[0], full[:, k:k + 1]) and np.array_equal(alone[1], pairs), (stat, k)


# ------------------------------------------------------------------------------------------ 7: the device forms
@pytest.mark.parametrize("kind", ["const", "missing"])
@pytest.mark.parametrize("n,S,max_lag", SHAPES)
def test_the_device_forms_give_the_host_forms_bits(n, S, max_lag, kind):
    """annotations of pitch C + 5 with NaN in the pitch columns, scores of pitch C + 3, guard rows behind n: the host form's
    bits, nothing else touched; n_pairs = NULL works"""
    import torch
    c = case(n, S, max_lag, kind)
    pos = np.arange(n, dtype=np.float64) // 2                                      # tied pairs of rows
    for count in ((COLS, 65) if n in (65, 200) else (COLS,)):
        d_annot = torch.full((n, count + 5), float("nan"), dtype=torch.float32, device="cuda")
        d_annot[:, :count] = torch.from_numpy(c.annot[:, :count].copy()).cuda()
        for stat in STATS:
            for px, dist, lag in ((None, None, max_lag), (pos, 3.0, None)):
                host = (c.host(stat) if px is None and count == COLS else
                        c.d.lag_ldscore_annot(c.annot[:, :count], lag, stat, complete=c.complete, pos=px, max_dist=dist))
                for with_pairs in (True, False):
                    d_score = torch.full((n + GUARD, count + 3), GUARD_F, dtype=torch.float32, device="cuda")
                    d_pairs = torch.full((n + GUARD,), GUARD_I, dtype=torch.int32, device="cuda")
                    assert c.d.lag_ldscore_annot(d_annot[:, :count], lag, stat, complete=c.complete, pos=px, max_dist=dist,
                                                 device=(d_score[:, :count], d_pairs if with_pairs else None)) is None
                    score, pairs = d_score.cpu().numpy(), d_pairs.cpu().numpy().view(np.uint32)
                    assert same_bits(score[:n, :count], host[0]), (stat, with_pairs, count)
                    assert (score[n:] == np.float32(GUARD_F)).all() and (score[:, count:] == np.float32(GUARD_F)).all()
                    assert (pairs[n:] == GUARD_I).all()
                    assert np.array_equal(pairs[:n], host[1]) if with_pairs else (pairs == GUARD_I).all()
    # the C call itself with n_pairs = NULL and score_ld > C, host form
    score = np.full((n + GUARD, COLS + 3), GUARD_F, dtype=np.float32)
    f = c.d._lib.STORM_dosage_lag_ldscore_annot_complete if c.complete else c.d._lib.STORM_dosage_lag_ldscore_annot
    assert f(c.d._h, ADJ, max_lag, None, 0.0, c.annot.ctypes.data, COLS, COLS, score.ctypes.data, COLS + 3, None, n) == 0
    assert same_bits(score[:n, :COLS], c.host("r2_adj")[0])
    assert (score[n:] == np.float32(GUARD_F)).all() and (score[:, COLS:] == np.float32(GUARD_F)).all()


# ------------------------------------------------------------------------------------------ 8: the generic shim call
@pytest.mark.parametrize("n,max_lag,extra,count", [(200, 70, 5, 67), (65, 1000, 1, 1), (130, 63, 0, 64)])
def test_band_annot_sums_over_a_band_the_test_wrote_itself(hip_ctx, n, max_lag, extra, count):
    """storm_hip_lag_band_annot_sums_device directly: a pitch ld > L, NaNs and garbage in the corner and the pitch columns of
    the band, of the matrix behind the strided N view (row 3 i + 2, column 3 d + 2, as the pairwise-complete call passes it)
    and of the annotations; with and without lo / hi"""
    import torch
    rng = np.random.default_rng(n + max_lag)
    L = lag_of(n, max_lag)
    ld = L + extra
    poison = np.where(rng.integers(0, 2, size=(n, ld)) == 1, 0xDEADBEEF, 0x7FC00000).astype(np.uint32)
    ok = (np.arange(n)[:, None] + 1 + np.arange(ld)[None, :] < n) & (np.arange(ld)[None, :] < L)
    vals = rng.random((n, ld), dtype=np.float32)
    vals[rng.random((n, ld)) < 0.05] = np.nan
    band = np.where(ok, bits(vals), poison).view(np.float32)
    N = rng.choice(np.array([0, 1, 2, 3, 4, 77, 5000], dtype=np.uint32), size=(n, ld))
    lds = (3 * L + 2 + 3) // 4 * 4
    sums = np.full((3 * n, lds), 0xDEADBEEF, dtype=np.uint32)
    sums[2::3, 2:3 * L + 2:3] = np.where(ok, N, 0xDEADBEEF)[:, :L]
    nobs = sums[2::3, 2:3 * L + 2:3]
    annot_ld, score_ld = count + 5, count + 3
    annot = np.full((n, annot_ld), np.nan, dtype=np.float32)
    annot[:, :count] = annotations(n, n)[:, :count]
    pos = np.cumsum(rng.choice([0.0, 0.0, 1.0, 1.0, 2.0, 40.0], size=n))
    lo, hi = _ldscore_annot.windows(pos, 6.0)
    d_band = torch.from_numpy(band.copy()).cuda()
    d_sums = torch.from_numpy(sums.view(np.int32).copy()).cuda()
    d_annot = torch.from_numpy(annot).cuda()
    d_lo, d_hi = torch.from_numpy(lo.view(np.int32).copy()).cuda(), torch.from_numpy(hi.view(np.int32).copy()).cuda()
    for windowed in (False, True):
        for stat, n_const, view in (("r2", 0, False), ("r2_adj", 2, False), ("r2_adj", 900, False), ("r2_adj", 0, True), ("r2", 0, True)):
            for with_pairs in (True, False):
                d_score = torch.full((n + GUARD, score_ld), GUARD_F, dtype=torch.float32, device="cuda")
                d_pairs = torch.full((n + GUARD,), GUARD_I, dtype=torch.int32, device="cuda")
                hip_ctx.lag_band_annot_sums_device(d_band.data_ptr(), ld, n, max_lag, d_annot.data_ptr(), annot_ld, count,
                                                   d_score.data_ptr(), score_ld, d_pairs.data_ptr() if with_pairs else None, stat,
                                                   n_const, d_sums.data_ptr() + 4 * (2 * lds + 2) if view else None, 3 * lds, 3,
                                                   d_lo.data_ptr() if windowed else None, d_hi.data_ptr() if windowed else None)
                hip_ctx.synchronize()
                score, pairs = d_score.cpu().numpy(), d_pairs.cpu().numpy().view(np.uint32)
                assert (score[n:] == np.float32(GUARD_F)).all() and (score[:, count:] == np.float32(GUARD_F)).all()
                assert (pairs[n:] == GUARD_I).all()
                ref, sum_abs, m, a_max = _ldscore_annot.annot_sums(band, n, max_lag, STATS[stat], annot[:, :count], n_const,
                                                                   nobs if view else None, lo if windowed else None,
                                                                   hi if windowed else None)
                _ldscore_annot.assert_scores(score[:n, :count], pairs[:n] if with_pairs else None, ref, sum_abs, m, a_max,
                                             (stat, n_const, view, windowed))
                if not with_pairs:
                    assert (pairs == GUARD_I).all()
                if stat == "r2_adj" and not view and n_const < 3:
                    assert (pairs[:n] == 0).all() or not with_pairs


def test_the_shim_refuses_what_it_cannot_reduce(hip_ctx, lib):
    import torch
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = t.data_ptr()
    f = lib.storm_hip_lag_band_annot_sums_device
    err = lib.storm_hip_last_error
    h = hip_ctx._h
    assert f(h, None, 4, 5, 4, 0, 9, None, 0, 0, None, None, p, 2, 2, p, 2, None) == -1 and b"NULL argument" in err()   # no band
    assert f(h, p, 4, 5, 4, 0, 9, None, 0, 0, None, None, p, 2, 2, None, 2, None) == -1 and b"NULL argument" in err()   # no score
    assert f(h, p, 4, 5, 0, 0, 9, None, 0, 0, None, None, p, 2, 2, p, 2, None) == -1 and b"max_lag 0" in err()
    assert f(h, p, 4, 5, 4, 2, 9, None, 0, 0, None, None, None, 2, 0, p, 1, None) == -1 and b"unknown stat" in err()     # the old order
    assert f(h, p, 3, 5, 4, 0, 9, None, 0, 0, None, None, None, 2, 0, p, 1, None) == -1 and b"leading dimension" in err()
    assert f(h, p, 4, 5, 4, 0, 9, None, 0, 0, None, None, None, 2, 0, p, 1, None) == -1 and b"NULL annotations" in err()
    for n_annot in (0, 1025):
        assert f(h, p, 4, 5, 4, 0, 9, None, 0, 0, p, None, p, 1, n_annot, p, 1, None) == -1 and b"annotation columns (1 .. 1024)" in err()
    assert f(h, p, 4, 5, 4, 0, 9, None, 0, 0, p, None, p, 2, 3, p, 3, None) == -1 and b"annot_ld 2" in err()
    assert f(h, p, 4, 5, 4, 0, 9, None, 0, 0, p, None, p, 3, 3, p, 2, None) == -1 and b"score_ld 2" in err()
    assert f(h, p, 4, 5, 4, 0, 9, None, 0, 0, p, None, p, 3, 3, p, 3, None) == -1 and b"come together" in err()
    assert f(h, p, 4, 5, 4, 0, 9, None, 0, 0, None, p, p, 3, 3, p, 3, None) == -1 and b"come together" in err()
    assert f(h, p, 0, 1, 4, 0, 9, None, 0, 0, None, None, p, 3, 3, p, 3, None) == 0                                      # one row: nothing to do
    hip_ctx.synchronize()
    assert (t.cpu().numpy() == 0).all()
