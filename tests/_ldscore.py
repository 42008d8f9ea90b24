"""A numpy restatement of the LD-score reduction (storm.h: STORM_dosage_lag_ldscore; storm_hip.h:
storm_hip_lag_band_sums_device) over a float matrix in the lag layout, for tests/test_ldscore_math.py and
tests/test_gpu_ldscore.py: the checker, never the thing under test."""
import math

import numpy as np

R2, ADJ = 0, 1


def both_sides(band, n, L, fill):
    """[n, 2 L]: row i's entries of the lag layout `band` (pair (i, i + 1 + d) at band[i, d]) — columns [0, L) the pairs ahead
    of it, band[i, d], columns [L, 2 L) the pairs behind it, band[i - 1 - d, d] — and `fill` where there is no such pair.
    Nothing of the lower-right corner (i + 1 + d >= n) or of the columns from L on is read."""
    out = np.full((n, 2 * L), fill, dtype=band.dtype)
    for d in range(L):
        rows = n - 1 - d                                                           # the pairs (i, i + 1 + d), i < rows
        if rows <= 0:
            break
        out[:rows, d] = band[:rows, d]
        out[d + 1:, L + d] = band[:rows, d]
    return out


def band_sums(band, n, max_lag, stat, n_const=0, nobs=None):
    """(ref, sum_abs, m): per row the exactly rounded sum (math.fsum) of the double terms of its summed pairs, the sum of
    their magnitudes, and their number. band: [n, >= L] float32; nobs: [n, >= L] integers in the same layout, or None:
    n_const."""
    L = min(max_lag, max(n - 1, 0))
    rho = both_sides(np.asarray(band, dtype=np.float32), n, L, np.float32(np.nan)).astype(np.float64)
    N = (both_sides(np.asarray(nobs).astype(np.int64), n, L, 0) if nobs is not None
         else np.full((n, 2 * L), int(n_const), dtype=np.int64))
    summed = ~np.isnan(rho)
    if stat == ADJ:
        summed &= N >= 3
        with np.errstate(all="ignore"):
            t = rho - (1.0 - rho) / (N - 2).astype(np.float64)
    else:
        t = rho
    ref = np.array([math.fsum(t[i][summed[i]]) for i in range(n)], dtype=np.float64)
    sum_abs = np.array([math.fsum(np.abs(t[i][summed[i]])) for i in range(n)], dtype=np.float64)
    return ref, sum_abs, summed.sum(axis=1).astype(np.uint32)


def bound(ref, sum_abs, m):
    """|score - float32(ref)| may reach ulp32(ref) + 2^-36 (sum |t| + m): m <= 2^17 terms added in double in any order err by
    at most (m - 1) 2^-53 sum |t|, the three double operations of an adjusted term by a few 2^-53 each, the one rounding to
    float by half an ulp (a whole one covers a sum that falls on the other side of a rounding boundary)."""
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return ulp + 2.0 ** -36 * (sum_abs + m.astype(np.float64))


def assert_scores(score, pairs, ref, sum_abs, m, what=""):
    """every row: the count exactly, the score within the bound, +0.0f where nothing is summed"""
    assert np.array_equal(pairs, m), (what, np.flatnonzero(pairs != m)[:8])
    err = np.abs(score.astype(np.float64) - ref.astype(np.float32).astype(np.float64))
    lim = bound(ref, sum_abs, m)
    worst = int(np.argmax(err - lim))
    assert (err <= lim).all(), (what, worst, float(score[worst]), float(ref[worst]), float(err[worst]), float(lim[worst]))
    empty = m == 0
    assert (score[empty].view(np.uint32) == 0).all(), what
