"""storm_ldscore_math.h's accumulate line of lag_band_annot_sums_kernel — ldscore_annot_add, one fused multiply-add per pair
and column — built by the host C++ compiler (-ffp-contract=off) and driven by a plain C restatement of the whole windowed,
annotated reduction over a lag-layout array. Compared with the numpy restatement of tests/_ldscore_annot.py on hand-made
bands whose lower-right corner and pitch columns hold NaNs and 0xDEADBEEF patterns that must not influence anything, with
and without windows. And the bound has teeth: a float32 accumulation of the same terms does not meet it. No device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _ldscore_annot
from tests._ldscore import ADJ, R2
from tests.test_ldscore_math import make_band

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = r"""
#include "storm_ldscore_math.h"
extern "C" double add(double sum, double term, float a) { return storm::ldscore_annot_add(sum, term, a); }
extern "C" void annot_sums(const float* vals, uint64_t ld, uint64_t n, uint64_t max_lag, int stat, uint64_t n_const,
                           const uint32_t* nobs, uint64_t pitch, uint64_t stride, const uint32_t* lo, const uint32_t* hi,
                           const float* annot, uint64_t annot_ld, uint64_t n_annot, float* score, uint64_t score_ld,
                           uint32_t* n_pairs) {
    const uint64_t L = n ? (max_lag < n - 1 ? max_lag : n - 1) : 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t first = lo ? lo[i] : 0, last = hi ? hi[i] : n - 1;
        uint32_t m = 0;
        for (uint64_t c = 0; c < n_annot; ++c) {
            double sum = 0.0, t;
            m = 0;
            for (uint64_t d = L; d-- > 0;) {                                     /* the pairs (j, i), j = i - 1 - d, j ascending */
                if (d + 1 > i) continue;
                const uint64_t j = i - 1 - d;
                if (j < first) continue;
                if (storm::ldscore_term(vals[j * ld + d], stat, nobs ? storm::ldscore_nobs_at(nobs, pitch, stride, j, d) : n_const, &t))
                    sum = storm::ldscore_annot_add(sum, t, annot[j * annot_ld + c]), ++m;
            }
            for (uint64_t d = 0; d < L && i + 1 + d < n && i + 1 + d <= last; ++d)   /* the pairs (i, i + 1 + d): row i */
                if (storm::ldscore_term(vals[i * ld + d], stat, nobs ? storm::ldscore_nobs_at(nobs, pitch, stride, i, d) : n_const, &t))
                    sum = storm::ldscore_annot_add(sum, t, annot[(i + 1 + d) * annot_ld + c]), ++m;
            score[i * score_ld + c] = (float)sum;
        }
        if (n_pairs) n_pairs[i] = m;
    }
}
"""


@pytest.fixture(scope="module")
def math(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "a host C++ compiler"
    d = tmp_path_factory.mktemp("ldscore_annot")
    src, so = d / "ldscore_annot.cpp", d / "libldscore_annot.so"
    src.write_text(SOURCE)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "stormbitmaps_amd", "csrc"), str(src), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.add.restype = C.c_double
    lib.add.argtypes = [C.c_double, C.c_double, C.c_float]
    lib.annot_sums.restype = None
    lib.annot_sums.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_void_p, C.c_uint64,
                               C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                               C.c_void_p]
    return lib


def test_the_accumulate_line_rounds_once(math):
    """sum + t a with the product exact: where the rounded product and the fused one differ, the line gives the fused one"""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    differed = 0
    for _ in range(2000):
        s, t, a = float(rng.normal()), float(rng.random()), np.float32(rng.normal())
        got = math.add(s, t, a)
        exact = Fraction(s) + Fraction(t) * Fraction(float(a))
        assert got == float(exact), (s, t, a)                                      # float(Fraction) rounds correctly, once
        differed += got != s + t * float(a)
    assert differed > 0                                                            # ... which two roundings do not always give
    assert math.add(0.0, 0.0, np.float32(-3.0)) == 0.0 and np.signbit(math.add(0.0, 0.0, np.float32(-3.0))) == 0
    assert math.add(1.25, 0.0, np.float32(-3.0)) == 1.25                           # a pair that is not summed changes nothing


def annotations(rng, n, C):
    """random normal floats with some exact zeros and (half of them) negative values"""
    a = rng.normal(size=(n, C)).astype(np.float32)
    a[rng.random((n, C)) < 0.15] = 0.0
    return a


def random_windows(rng, n):
    """symmetric windows from random non-decreasing positions with ties and gaps"""
    pos = np.cumsum(rng.choice([0.0, 0.0, 1.0, 1.0, 2.0, 9.0], size=n))
    dist = float(rng.choice([0.0, 1.0, 2.0, 4.0, 11.0]))
    return _ldscore_annot.windows(pos, dist)


@pytest.mark.parametrize("n,max_lag,ld_extra", [(2, 1, 0), (2, 9, 3), (5, 100, 0), (9, 3, 2), (40, 7, 1), (70, 64, 5), (70, 69, 0),
                                                (131, 65, 3)])
def test_reduction_against_numpy_on_poisoned_bands(math, n, max_lag, ld_extra):
    band, nobs, L, ld = make_band(n, max_lag, ld_extra, 17 * n + max_lag, nan_rows=(0, n // 2))
    rng = np.random.default_rng(n + max_lag)
    Cn, annot_ld, score_ld = 5, 5 + 2, 5 + 3
    annot = np.full((n, annot_ld), np.nan, dtype=np.float32)                       # NaN in the pitch columns: never read
    annot[:, :Cn] = annotations(rng, n, Cn)
    for lo, hi in ((None, None), random_windows(rng, n)):
        for stat in (R2, ADJ):
            for view in (None, nobs):
                for n_const in ((2, 500) if view is None else (0,)):
                    score = np.full((n + 1, score_ld), -77.5, dtype=np.float32)
                    pairs = np.full(n + 3, 0xABCDABCD, dtype=np.uint32)
                    math.annot_sums(band.ctypes.data, ld, n, max_lag, stat, n_const, None if view is None else view.ctypes.data, ld, 1,
                                    None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data,
                                    annot.ctypes.data, annot_ld, Cn, score.ctypes.data, score_ld, pairs.ctypes.data)
                    assert (score[n:] == -77.5).all() and (score[:, Cn:] == -77.5).all() and (pairs[n:] == 0xABCDABCD).all()
                    ref, sum_abs, m, a_max = _ldscore_annot.annot_sums(band, n, max_lag, stat, annot[:, :Cn], n_const, view, lo, hi)
                    _ldscore_annot.assert_scores(score[:n, :Cn], pairs[:n], ref, sum_abs, m, a_max,
                                                 (stat, n_const, view is not None, lo is not None))
                    assert pairs[0] == 0 and (score[0, :Cn] == 0).all()            # every pair of a NaN row is dropped
    # the poison is inert: another poison, the same answer
    band2, nobs2, annot2 = band.copy(), nobs.copy(), annot.copy()
    annot2[:, Cn:] = 1e30
    for i in range(n):
        for d in range(ld):
            if d >= L or i + 1 + d >= n:
                band2.view(np.uint32)[i, d] = 0x3F800000
                nobs2[i, d] = 1000
    lo, hi = random_windows(rng, n)
    out = []
    for b, v, a in ((band, nobs, annot), (band2, nobs2, annot2)):
        s = np.zeros((n, Cn), dtype=np.float32)
        p = np.zeros(n, dtype=np.uint32)
        math.annot_sums(b.ctypes.data, ld, n, max_lag, ADJ, 0, v.ctypes.data, ld, 1, lo.ctypes.data, hi.ctypes.data, a.ctypes.data,
                        annot_ld, Cn, s.ctypes.data, Cn, p.ctypes.data)
        out.append((s, p))
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32)) and np.array_equal(out[0][1], out[1][1])


def test_a_column_of_ones_without_windows_is_the_plain_reduction():
    from tests import _ldscore
    band, nobs, L, ld = make_band(70, 64, 5, 7)
    ref, sum_abs, m, a_max = _ldscore_annot.annot_sums(band, 70, 64, ADJ, np.ones((70, 1), dtype=np.float32), nobs=nobs)
    ref1, sum_abs1, m1 = _ldscore.band_sums(band, 70, 64, ADJ, nobs=nobs)
    assert np.array_equal(ref[:, 0], ref1) and np.array_equal(sum_abs[:, 0], sum_abs1) and np.array_equal(m, m1)
    assert (a_max[m > 0] == 1).all()


def test_the_numpy_restatement_on_a_band_worked_by_hand():
    """n = 4, L = 2: rows 0 .. 3 see {1, 2}, {0, 2, 3}, {0, 1, 3}, {1, 2}; the windows then cut row 0 <-> row 2"""
    x = np.float32(np.nan)
    band = np.array([[0.5, 0.25], [0.125, x], [1.0, 9.0], [9.0, 9.0]], dtype=np.float32)   # (0,1) (0,2) / (1,2) (1,3) / (2,3)
    annot = np.array([[1, 2], [1, 0], [1, -4], [1, 8]], dtype=np.float32)
    ref, sum_abs, m, a_max = _ldscore_annot.annot_sums(band, 4, 2, R2, annot)
    assert ref[:, 0].tolist() == [0.75, 0.625, 1.375, 1.0] and m.tolist() == [2, 2, 3, 1]
    assert ref[:, 1].tolist() == [0.5 * 0 + 0.25 * -4, 0.5 * 2 + 0.125 * -4, 0.25 * 2 + 0.125 * 0 + 1.0 * 8, 1.0 * -4]
    assert sum_abs[:, 1].tolist() == [1.0, 1.5, 8.5, 4.0] and a_max[:, 1].tolist() == [4, 4, 8, 4]
    lo, hi = np.array([0, 0, 1, 2], dtype=np.uint32), np.array([1, 2, 3, 3], dtype=np.uint32)
    ref, _, m, _ = _ldscore_annot.annot_sums(band, 4, 2, R2, annot, lo=lo, hi=hi)
    assert ref[:, 0].tolist() == [0.5, 0.625, 1.125, 1.0] and m.tolist() == [1, 2, 2, 1]
    lo, hi = _ldscore_annot.windows([0.0, 1.0, 2.0, 3.0], 1.0)
    assert lo.tolist() == [0, 0, 1, 2] and hi.tolist() == [1, 2, 3, 3] and _ldscore_annot.window_lag(lo, hi) == 1


def test_a_float32_accumulation_does_not_meet_the_bound():
    """the teeth of the bound, at the shape (200 rows, lag 129) of tests/test_gpu_ldscore_annot.py: the same terms, the same
    order, one float32 running sum instead of the double one — rows miss the bound by orders of magnitude"""
    n, max_lag, Cn = 200, 129, 3
    rng = np.random.default_rng(200129)
    band, _, L, ld = make_band(n, max_lag, 0, 5)
    annot = annotations(rng, n, Cn)
    ref, sum_abs, m, a_max = _ldscore_annot.annot_sums(band, n, max_lag, R2, annot)
    rho = _ldscore_annot._ldscore.both_sides(band, n, L, np.float32(np.nan))
    i = np.arange(n)[:, None]
    d = np.arange(L)[None, :]
    J = np.concatenate([i + 1 + d, i - 1 - d], axis=1)
    in_float = np.zeros((n, Cn), dtype=np.float32)
    in_double = np.zeros((n, Cn), dtype=np.float64)
    for r in range(n):
        keep = ~np.isnan(rho[r])
        for t, j in zip(rho[r][keep], J[r][keep]):
            in_float[r] += np.float32(t) * annot[j]
            in_double[r] += np.float64(t) * annot[j].astype(np.float64)
    assert not _ldscore_annot.violations(in_double.astype(np.float32), ref, sum_abs, m, a_max).any()   # double, any order: inside
    miss = _ldscore_annot.violations(in_float, ref, sum_abs, m, a_max)
    assert miss.any() and miss.mean() > 0.25, float(miss.mean())
