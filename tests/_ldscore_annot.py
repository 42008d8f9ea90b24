"""A numpy restatement of the stratified LD-score reduction (storm.h: STORM_dosage_lag_ldscore_annot; storm_hip.h:
storm_hip_lag_band_annot_sums_device) over a float matrix in the lag layout, an annotation matrix and a window per row, for
tests/test_ldscore_annot_math.py and tests/test_gpu_ldscore_annot.py: the checker, never the thing under test. It builds
on tests/_ldscore.py's both_sides."""
import math

import numpy as np

from tests import _ldscore
from tests._ldscore import ADJ, R2  # noqa: F401  (re-exported)


def windows(pos, max_dist):
    """(lo, hi) uint32: row i is summed against the rows j of [lo[i], hi[i]], j != i — those with |pos[j] - pos[i]| <=
    max_dist — by np.searchsorted on the non-decreasing positions. (The tests use positions and distances whose sums and
    differences are exact in double, so pos - max_dist here and the planner's pos[i] - pos[j] <= max_dist agree.)"""
    pos = np.asarray(pos, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        lo = np.searchsorted(pos, pos - max_dist, "left")
        hi = np.searchsorted(pos, pos + max_dist, "right") - 1
    return lo.astype(np.uint32), hi.astype(np.uint32)


def window_lag(lo, hi):
    """the lag the windows need: max_i max(i - lo[i], hi[i] - i)"""
    i = np.arange(len(lo), dtype=np.int64)
    return int(max((i - lo).max(), (hi - i).max())) if len(lo) else 0


def annot_sums(band, n, max_lag, stat, annot, n_const=0, nobs=None, lo=None, hi=None):
    """(ref [n, C], sum_abs [n, C], m [n], a_max [n, C]): per (row, column) the exactly rounded sum (math.fsum) of the double
    products t(i, j) * a[j, c] over the summed pairs of row i's window — within max_lag AND inside [lo[i], hi[i]] where
    bounds are given — the sum of their magnitudes, the number of summed pairs of the row and the largest |a[j, c]| among
    them. band: [n, >= L] float32 in the lag layout; nobs: [n, >= L] integers in the same layout, or None: n_const;
    annot: [n, C] float32."""
    L = min(max_lag, max(n - 1, 0))
    annot = np.asarray(annot, dtype=np.float32)
    C = annot.shape[1]
    rho = _ldscore.both_sides(np.asarray(band, dtype=np.float32), n, L, np.float32(np.nan)).astype(np.float64)
    N = (_ldscore.both_sides(np.asarray(nobs).astype(np.int64), n, L, 0) if nobs is not None
         else np.full((n, 2 * L), int(n_const), dtype=np.int64))
    i = np.arange(n, dtype=np.int64)[:, None]
    d = np.arange(L, dtype=np.int64)[None, :]
    J = np.concatenate([i + 1 + d, i - 1 - d], axis=1)                             # the other row of both_sides' column
    summed = ~np.isnan(rho)
    if lo is not None:
        summed &= (J >= np.asarray(lo, dtype=np.int64)[:, None]) & (J <= np.asarray(hi, dtype=np.int64)[:, None])
    if stat == ADJ:
        summed &= N >= 3
        with np.errstate(all="ignore"):
            t = rho - (1.0 - rho) / (N - 2).astype(np.float64)
    else:
        t = rho
    a64 = annot.astype(np.float64)
    ref, sum_abs, a_max = np.zeros((n, C)), np.zeros((n, C)), np.zeros((n, C))
    for r in range(n):
        js = J[r][summed[r]]
        if js.size == 0:
            continue
        prod = t[r][summed[r]][:, None] * a64[js]                                  # [m, C]: each product rounded to double
        mag = np.abs(prod)
        a_max[r] = np.abs(a64[js]).max(axis=0)
        for c in range(C):
            ref[r, c] = math.fsum(prod[:, c])
            sum_abs[r, c] = math.fsum(mag[:, c])
    return ref, sum_abs, summed.sum(axis=1).astype(np.uint32), a_max


def bound(ref, sum_abs, m, a_max):
    """|score - float32(ref)| may reach ulp32(ref) + 2^-36 (sum |t a| + m max |a|), per (row, column), for double arithmetic in
    any order:
      * the device adds m <= 2^17 products with one fused multiply-add each: every step rounds the running sum once, by at
        most 2^-53 of a partial sum that sum |t a| bounds — (m - 1) 2^-53 sum |t a| in all, whatever the order;
      * the reference rounds each product to double (2^-53 |t a| each) before its exact sum: 2^-53 sum |t a| more;
      * the three double operations of an adjusted term err by a few 2^-53 of a term of magnitude <= 1 or so, each scaled by
        |a| <= max |a|: a few 2^-53 m max |a|;
      together below 2^-36 (sum |t a| + m max |a|) for m <= 2^17 - 2;
      * the one rounding to float errs by half an ulp; a whole one covers a sum that falls on the other side of a rounding
        boundary than the reference.
    A float32 accumulation of the same terms errs by about m 2^-25 sum |t a| and does not meet this
    (tests/test_ldscore_annot_math.py shows it)."""
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return ulp + 2.0 ** -36 * (sum_abs + m.astype(np.float64)[:, None] * a_max)


def violations(score, ref, sum_abs, m, a_max):
    """[n, C] bool: where a score misses the bound"""
    err = np.abs(np.asarray(score).astype(np.float64) - ref.astype(np.float32).astype(np.float64))
    return err > bound(ref, sum_abs, m, a_max)


def assert_scores(score, pairs, ref, sum_abs, m, a_max, what=""):
    """every row and column: the count exactly, the score within the bound, +0.0f where nothing is summed"""
    score = np.asarray(score)
    assert score.shape == ref.shape, (what, score.shape, ref.shape)
    if pairs is not None:
        assert np.array_equal(pairs, m), (what, np.flatnonzero(pairs != m)[:8])
    err = np.abs(score.astype(np.float64) - ref.astype(np.float32).astype(np.float64))
    lim = bound(ref, sum_abs, m, a_max)
    worst = np.unravel_index(int(np.argmax(err - lim)), err.shape)
    assert (err <= lim).all(), (what, worst, float(score[worst]), float(ref[worst]), float(err[worst]), float(lim[worst]))
    empty = m == 0
    assert (np.ascontiguousarray(score[empty]).view(np.uint32) == 0).all(), what
