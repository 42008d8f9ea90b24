"""Per-variant LD scores on the device (storm.h: STORM_dosage_lag_ldscore, _ldscore_complete and their _device forms;
storm_hip.h: storm_hip_lag_band_sums_device): the band of r^2 the lag calls write, reduced by lag_band_sums_kernel over
both sides of every row. Everything goes through the C-ABI (StormDosage.lag_ldscore), in the host and the _device forms.

Expected values: the counts EXACTLY and the scores within tests/_ldscore.py's derived bound — ulp32(ref) + 2^-36 (sum |t| + m),
which a float accumulation does not meet — from the library's own pairw_lag_corr[_complete] host matrix (and pairw_lag_nobs),
reduced in numpy with math.fsum; once, independently of that matrix, against np.corrcoef on the unpacked dosages; at
L = n - 1 against the n x n pairw_corr matrix. Every row is checked. Shapes: one partial block, the 64-row block edge on
both sides, L = 1, L just below, at and above 64, L clipped to n - 1, many blocks, samples that do not fill a word."""
import numpy as np
import pytest

import stormbitmaps_amd as sb
from tests import _ldscore
from tests._ldscore import ADJ, R2

pytestmark = pytest.mark.gpu

SHAPES = [(2, 40, 1), (5, 40, 100), (63, 96, 62), (64, 96, 1), (65, 96, 64), (130, 257, 63), (130, 257, 65), (200, 1000, 129),
          (300, 4099, 10000), (1100, 64, 17)]                                      # (n, samples, max_lag)
STATS = {"r2": R2, "r2_adj": ADJ}
GUARD = 7                                                                          # elements behind n of a device output
GUARD_F, GUARD_I = -77.5, 0x5EADBEEF


def lag_of(n, max_lag):
    return min(max_lag, n - 1)


def dosages(rng, n, S):
    """0 .. 2 copies per sample at a per-row allele frequency in [0.05, 0.5]; no row is constant"""
    G = np.empty((n, S), dtype=np.uint8)
    for i in range(n):
        while True:
            G[i] = rng.binomial(2, rng.uniform(0.05, 0.5), size=S)
            if G[i].min() != G[i].max():
                break
    return G


def rows_of(n, S, kind):
    rng = np.random.default_rng(1000 * n + S + {"plain": 0, "const": 1, "missing": 2}[kind])
    G = dosages(rng, n, S)
    if kind == "const":                                                            # their pairs are NaN: never summed
        for i, v in ((0, 0), (63, 2), (64, 1), (n - 1, 0)):
            if i < n:
                G[i] = v
    if kind == "missing":
        G[rng.random((n, S)) < 0.10] = 3
        h = S // 2

        def sharing(a, k, xs, ys):
            """rows a and a + 1 have exactly the k samples [h, h + k) in common, with variance on them"""
            G[a, h + k:] = 3
            G[a + 1, :h] = 3
            G[a, h:h + k], G[a + 1, h:h + k] = xs, ys
            G[a + 1, h + k:][G[a + 1, h + k:] == 3] = 1
            G[a, :h][G[a, :h] == 3] = 1
        sharing(0, 2, [0, 1], [1, 0])                                              # N = 2: dropped under ADJ
        if n >= 5:
            G[2] = 3                                                               # nobody shares a sample with it
            sharing(3, 3, [0, 1, 2], [1, 0, 1])                                    # N = 3: the smallest N that ADJ keeps
    return G


class Case:
    """one container per (shape, kind), and what the library itself says about its pairs: fetched once, never modified"""

    def __init__(self, n, S, max_lag, kind):
        self.n, self.S, self.max_lag, self.kind, self.L = n, S, max_lag, kind, lag_of(n, max_lag)
        self.G = rows_of(n, S, kind)
        self.d = sb.StormDosage(S)
        for row in self.G:
            self.d.add(row)
        self._memo = {}

    def memo(self, key, make):
        if key not in self._memo:
            v = make()
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
            self._memo[key] = v
        return self._memo[key]

    def band(self, complete):
        """the library's own float matrix in the lag layout (host form)"""
        f = self.d.pairw_lag_corr_complete if complete else self.d.pairw_lag_corr
        return self.memo(("band", complete), lambda: f(self.max_lag, "r2"))

    def nobs(self):
        return self.memo("nobs", lambda: self.d.pairw_lag_nobs(self.max_lag))

    def reference(self, stat, complete):
        def make():
            if complete:
                return _ldscore.band_sums(self.band(True), self.n, self.max_lag, STATS[stat], nobs=self.nobs())
            return _ldscore.band_sums(self.band(False), self.n, self.max_lag, STATS[stat], n_const=self.S)
        return self.memo(("ref", stat, complete), make)

    def host(self, stat, complete):
        return self.memo(("host", stat, complete), lambda: self.d.lag_ldscore(self.max_lag, stat, complete=complete))


_cases = {}


def case(n, S, max_lag, kind):
    key = (n, S, max_lag, kind)
    if key not in _cases:
        _cases[key] = Case(*key)
    return _cases[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------ 1, 2: counts and scores
@pytest.mark.parametrize("stat", ["r2", "r2_adj"])
@pytest.mark.parametrize("kind", ["plain", "const"])
@pytest.mark.parametrize("n,S,max_lag", SHAPES)
def test_counts_and_scores_complete_case(n, S, max_lag, kind, stat):
    c = case(n, S, max_lag, kind)
    score, pairs = c.host(stat, False)
    ref, sum_abs, m = c.reference(stat, False)
    _ldscore.assert_scores(score, pairs, ref, sum_abs, m, (n, S, max_lag, kind, stat))
    if kind == "const":
        for i in {0, 63, 64, n - 1}:
            if i < n:
                assert pairs[i] == 0 and bits(score)[i] == 0, i                    # a constant row: score +0.0f, no pair
        assert pairs.max() > 0 or n <= 2
    else:
        i = np.arange(n)
        assert np.array_equal(pairs, np.minimum(i, c.L) + np.minimum(n - 1 - i, c.L))   # nothing is NaN: the whole window


@pytest.mark.parametrize("stat", ["r2", "r2_adj"])
@pytest.mark.parametrize("n,S,max_lag", SHAPES)
def test_counts_and_scores_pairwise_complete(n, S, max_lag, stat):
    """10 % missing, a row with no sample at all, a pair that shares exactly 2 samples (dropped under ADJ, kept under R2)
    and one that shares exactly 3 (kept)"""
    c = case(n, S, max_lag, "missing")
    score, pairs = c.host(stat, True)
    ref, sum_abs, m = c.reference(stat, True)
    _ldscore.assert_scores(score, pairs, ref, sum_abs, m, (n, S, max_lag, stat))
    band, nobs = c.band(True), c.nobs()
    assert nobs[0, 0] == 2 and band[0, 0] == 1.0                                   # r = -1 on the two shared samples
    if n == 2:
        assert pairs.tolist() == ([1, 1] if stat == "r2" else [0, 0])
    if n >= 5:
        assert pairs[2] == 0 and bits(score)[2] == 0
        assert nobs[3, 0] == 3 and not np.isnan(band[3, 0])
        without = _ldscore.band_sums(band, n, max_lag, R2, nobs=nobs)[2]           # what R2 counts
        if stat == "r2_adj":
            assert pairs[0] < without[0] and pairs[1] < without[1]                 # the N = 2 pair left both rows
            assert pairs[3] >= 1 and pairs[4] >= 1


# ------------------------------------------------------------------------------------------ 3: against numpy alone
@pytest.mark.parametrize("n,S,max_lag", SHAPES)
def test_scores_against_corrcoef_on_the_unpacked_dosages(n, S, max_lag):
    """independent of the library's matrix: a swapped direction or a window off by one shows here. Each float r^2 is at
    most one float from the correctly rounded value (storm_dosage_math.h): 2^-23 relative each, 2^-22 (sum + 1) with the
    float64 reference's own error"""
    c = case(n, S, max_lag, "plain")
    score, pairs = c.host("r2", False)
    r2 = np.corrcoef(c.G.astype(np.float64)) ** 2
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    window = (np.abs(i - j) >= 1) & (np.abs(i - j) <= c.L)
    want = np.where(window, r2, 0.0).sum(axis=1)
    assert np.array_equal(pairs, window.sum(axis=1))
    err = np.abs(score.astype(np.float64) - want)
    assert (err <= 2.0 ** -22 * (want + 1.0)).all(), (int(np.argmax(err)), float(err.max()))


# ------------------------------------------------------------------------------------------ 4: the complete forms agree
@pytest.mark.parametrize("stat", ["r2", "r2_adj"])
@pytest.mark.parametrize("kind", ["plain", "const"])
@pytest.mark.parametrize("n,S,max_lag", SHAPES)
def test_rows_without_a_missing_value_give_the_same_bits_in_both_forms(n, S, max_lag, kind, stat):
    c = case(n, S, max_lag, kind)
    a, b = c.host(stat, False), c.host(stat, True)
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------ 5: repeatability, device forms
@pytest.mark.parametrize("complete", [False, True])
@pytest.mark.parametrize("n,S,max_lag", SHAPES)
def test_repeatable_and_the_device_form_gives_the_host_forms_bits(n, S, max_lag, complete):
    import torch
    c = case(n, S, max_lag, "missing" if complete else "const")
    for stat in STATS:
        first = c.host(stat, complete)
        again = c.d.lag_ldscore(max_lag, stat, complete=complete)
        assert np.array_equal(bits(first[0]), bits(again[0])) and np.array_equal(first[1], again[1]), stat
        for with_pairs in (True, False):
            d_score = torch.full((n + GUARD,), GUARD_F, dtype=torch.float32, device="cuda")
            d_pairs = torch.full((n + GUARD,), GUARD_I, dtype=torch.int32, device="cuda")
            assert c.d.lag_ldscore(max_lag, stat, complete=complete, device=(d_score, d_pairs if with_pairs else None)) is None
            score, pairs = d_score.cpu().numpy(), d_pairs.cpu().numpy().view(np.uint32)
            assert np.array_equal(bits(score[:n]), bits(first[0])), (stat, with_pairs)
            assert (score[n:] == np.float32(GUARD_F)).all() and (pairs[n:] == GUARD_I).all()
            assert np.array_equal(pairs[:n], first[1]) if with_pairs else (pairs == GUARD_I).all()
    # the C call itself with n_pairs = NULL, host form
    score = np.full(n + GUARD, GUARD_F, dtype=np.float32)
    f = c.d._lib.STORM_dosage_lag_ldscore_complete if complete else c.d._lib.STORM_dosage_lag_ldscore
    assert f(c.d._h, ADJ, max_lag, score.ctypes.data, None, n) == 0
    assert np.array_equal(bits(score[:n]), bits(c.host("r2_adj", complete)[0])) and (score[n:] == np.float32(GUARD_F)).all()


# ------------------------------------------------------------------------------------------ 6: the whole triangle
@pytest.mark.parametrize("stat", ["r2", "r2_adj"])
def test_at_full_lag_the_score_is_the_reduction_of_the_square_matrix(stat):
    n, S, max_lag = 300, 4099, 10000
    c = case(n, S, max_lag, "const")
    assert c.L == n - 1
    tri = c.memo("square", lambda: c.d.pairw_corr("r2"))                           # entries i < j, 0 elsewhere
    band = np.zeros((n, n - 1), dtype=np.float32)
    for i in range(n - 1):
        band[i, :n - 1 - i] = tri[i, i + 1:]
    ref, sum_abs, m = _ldscore.band_sums(band, n, n - 1, STATS[stat], n_const=S)
    score, pairs = c.host(stat, False)
    _ldscore.assert_scores(score, pairs, ref, sum_abs, m, stat)


# ------------------------------------------------------------------------------------------ 7: the generic shim call
@pytest.mark.parametrize("n,max_lag,extra", [(200, 70, 5), (65, 1000, 1)])
def test_band_sums_over_a_band_the_test_wrote_itself(hip_ctx, n, max_lag, extra):
    """storm_hip_lag_band_sums_device directly: a pitch ld > L, NaNs and garbage in the corner and the pitch columns of the
    band and of the matrix behind the strided N view (row 3 i + 2, column 3 d + 2, as the pairwise-complete call passes it)"""
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
    d_band = torch.from_numpy(band.copy()).cuda()
    d_sums = torch.from_numpy(sums.view(np.int32).copy()).cuda()
    for stat, n_const, view in (("r2", 0, False), ("r2_adj", 2, False), ("r2_adj", 900, False), ("r2_adj", 0, True), ("r2", 0, True)):
        for with_pairs in (True, False):
            d_score = torch.full((n + GUARD,), GUARD_F, dtype=torch.float32, device="cuda")
            d_pairs = torch.full((n + GUARD,), GUARD_I, dtype=torch.int32, device="cuda")
            hip_ctx.lag_band_sums_device(d_band.data_ptr(), ld, n, max_lag, d_score.data_ptr(),
                                         d_pairs.data_ptr() if with_pairs else None, stat, n_const,
                                         d_sums.data_ptr() + 4 * (2 * lds + 2) if view else None, 3 * lds, 3)
            hip_ctx.synchronize()
            score, pairs = d_score.cpu().numpy(), d_pairs.cpu().numpy().view(np.uint32)
            assert (score[n:] == np.float32(GUARD_F)).all() and (pairs[n:] == GUARD_I).all()
            ref, sum_abs, m = _ldscore.band_sums(band, n, max_lag, STATS[stat], n_const, nobs if view else None)
            _ldscore.assert_scores(score[:n], pairs[:n] if with_pairs else m, ref, sum_abs, m, (stat, n_const, view))
            if not with_pairs:
                assert (pairs == GUARD_I).all()
            if stat == "r2_adj" and not view and n_const < 3:
                assert (pairs[:n] == 0).all() or not with_pairs


def test_the_shim_refuses_what_it_cannot_reduce(hip_ctx, lib):
    import torch
    t = torch.zeros(64, dtype=torch.float32, device="cuda")
    p = t.data_ptr()
    f = lib.storm_hip_lag_band_sums_device
    assert f(hip_ctx._h, None, 4, 5, 4, 0, 9, None, 0, 0, p, None) == -1           # no band
    assert f(hip_ctx._h, p, 4, 5, 4, 0, 9, None, 0, 0, None, None) == -1           # no score
    assert f(hip_ctx._h, p, 4, 5, 0, 0, 9, None, 0, 0, p, None) == -1              # max_lag 0
    assert f(hip_ctx._h, p, 3, 5, 4, 0, 9, None, 0, 0, p, None) == -1              # ld < L
    assert f(hip_ctx._h, p, 4, 5, 4, 2, 9, None, 0, 0, p, None) == -1              # unknown stat
    assert b"stat" in lib.storm_hip_last_error()
    assert f(hip_ctx._h, p, 0, 1, 4, 0, 9, None, 0, 0, p, None) == 0               # one row: nothing to do
    hip_ctx.synchronize()
    assert (t.cpu().numpy() == 0).all()
