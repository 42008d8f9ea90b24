"""storm_ldscore_math.h — the per-pair line of lag_band_sums_kernel — built by the host C++ compiler (-ffp-contract=off) and
driven by a plain C restatement of the whole reduction over a lag-layout array: for every row the pairs ahead of it along
its own row, the pairs behind it down the anti-diagonal, one double sum, one rounding. Compared with the numpy restatement
of tests/_ldscore.py on hand-made bands whose lower-right corner and pitch columns hold NaNs and 0xDEADBEEF patterns that
must not influence anything. No device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _ldscore
from tests._ldscore import ADJ, R2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = r"""
#include "storm_ldscore_math.h"
extern "C" int term(float rho, int stat, uint64_t N, double* t) { return storm::ldscore_term(rho, stat, N, t) ? 1 : 0; }
extern "C" void band_sums(const float* vals, uint64_t ld, uint64_t n, uint64_t max_lag, int stat, uint64_t n_const,
                          const uint32_t* nobs, uint64_t pitch, uint64_t stride, float* score, uint32_t* n_pairs) {
    const uint64_t L = n ? (max_lag < n - 1 ? max_lag : n - 1) : 0;
    for (uint64_t i = 0; i < n; ++i) {
        double sum = 0.0, t;
        uint32_t m = 0;
        for (uint64_t d = 0; d < L && i + 1 + d < n; ++d)                     /* the pairs (i, i + 1 + d): row i */
            if (storm::ldscore_term(vals[i * ld + d], stat, nobs ? storm::ldscore_nobs_at(nobs, pitch, stride, i, d) : n_const, &t)) sum += t, ++m;
        for (uint64_t d = 0; d < L && d + 1 <= i; ++d) {                      /* the pairs (j, i), j = i - 1 - d: column d of row j */
            const uint64_t j = i - 1 - d;
            if (storm::ldscore_term(vals[j * ld + d], stat, nobs ? storm::ldscore_nobs_at(nobs, pitch, stride, j, d) : n_const, &t)) sum += t, ++m;
        }
        score[i] = (float)sum;
        if (n_pairs) n_pairs[i] = m;
    }
}
"""


@pytest.fixture(scope="module")
def math(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "a host C++ compiler"
    d = tmp_path_factory.mktemp("ldscore")
    src, so = d / "ldscore.cpp", d / "libldscore.so"
    src.write_text(SOURCE)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "stormbitmaps_amd", "csrc"), str(src), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.term.restype = C.c_int
    lib.term.argtypes = [C.c_float, C.c_int, C.c_uint64, C.POINTER(C.c_double)]
    lib.band_sums.restype = None
    lib.band_sums.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_void_p, C.c_uint64,
                              C.c_uint64, C.c_void_p, C.c_void_p]
    return lib


def test_one_term(math):
    """R2: the float widened; ADJ: rho - (1 - rho) / (N - 2) in double, the same bits as numpy's three operations; NaN is
    never summed, N < 3 not under ADJ"""
    t = C.c_double(7.0)
    rng = np.random.default_rng(5)
    rhos = np.concatenate([rng.random(200, dtype=np.float32), np.float32([0.0, 1.0, 1e-30, 0.99999994])])
    for rho in rhos:
        assert math.term(rho, R2, 0, C.byref(t)) == 1 and t.value == float(rho)
        for N in (3, 4, 100, 65536, 1 << 24, (1 << 32) - 1):
            assert math.term(rho, ADJ, N, C.byref(t)) == 1
            assert t.value == np.float64(rho) - (np.float64(1.0) - np.float64(rho)) / np.float64(N - 2), (rho, N)
        for N in (0, 1, 2):
            t.value = 7.0
            assert math.term(rho, ADJ, N, C.byref(t)) == 0 and t.value == 7.0
    for stat in (R2, ADJ):
        t.value = 7.0
        assert math.term(np.float32(np.nan), stat, 100, C.byref(t)) == 0 and t.value == 7.0
    assert math.term(np.float32(1.0), ADJ, 3, C.byref(t)) == 1 and t.value == 1.0          # a perfect pair is not corrected


def poisoned(n, L, ld, rng, dtype=np.float32):
    """[n, ld] of alternating NaN / 0xDEADBEEF patterns: whatever is not overwritten below is the corner or the pitch"""
    a = np.empty((n, ld), dtype=np.uint32)
    a[:] = np.where(rng.integers(0, 2, size=(n, ld)) == 1, 0xDEADBEEF, 0x7FC00000 if dtype == np.float32 else 0xFFFFFFFF)
    return a


def make_band(n, max_lag, ld_extra, seed, nan_rows=()):
    rng = np.random.default_rng(seed)
    L = min(max_lag, n - 1)
    ld = L + ld_extra
    band = poisoned(n, L, ld, rng).view(np.float32)
    nobs = poisoned(n, L, ld, rng, np.uint32)
    for i in range(n):
        for d in range(L):
            if i + 1 + d < n:
                band[i, d] = np.nan if (i in nan_rows or i + 1 + d in nan_rows or rng.random() < 0.05) else rng.random(dtype=np.float32)
                nobs[i, d] = rng.choice([0, 1, 2, 3, 4, 50, 1000])
    return band, nobs, L, ld


@pytest.mark.parametrize("n,max_lag,ld_extra", [(2, 1, 0), (2, 9, 3), (5, 100, 0), (9, 3, 2), (40, 7, 1), (70, 64, 5), (70, 69, 0),
                                                (131, 65, 3)])
def test_reduction_against_numpy_on_poisoned_bands(math, n, max_lag, ld_extra):
    band, nobs, L, ld = make_band(n, max_lag, ld_extra, 31 * n + max_lag, nan_rows=(0, n // 2))
    for stat in (R2, ADJ):
        for view in (None, nobs):
            for n_const in ((2, 3, 500) if view is None else (0,)):
                score = np.full(n + 3, -77.5, dtype=np.float32)
                pairs = np.full(n + 3, 0xABCDABCD, dtype=np.uint32)
                math.band_sums(band.ctypes.data, ld, n, max_lag, stat, n_const, None if view is None else view.ctypes.data, ld, 1,
                               score.ctypes.data, pairs.ctypes.data)
                assert (score[n:] == -77.5).all() and (pairs[n:] == 0xABCDABCD).all()
                ref, sum_abs, m = _ldscore.band_sums(band, n, max_lag, stat, n_const, view)
                _ldscore.assert_scores(score[:n], pairs[:n], ref, sum_abs, m, (stat, n_const, view is not None))
                if stat == ADJ and view is None and n_const < 3:
                    assert (pairs[:n] == 0).all()                                  # no N - 2 to divide by: nothing is summed
                assert pairs[0] == 0 and pairs[n // 2] == 0 and score[0] == 0      # every pair of a NaN row is dropped
    # the poison is inert: another poison, the same answer
    band2, nobs2 = band.copy(), nobs.copy()
    for i in range(n):
        for d in range(ld):
            if d >= L or i + 1 + d >= n:
                band2.view(np.uint32)[i, d] = 0x3F800000
                nobs2[i, d] = 1000
    for a, b in ((band, nobs), (band2, nobs2)):
        s = np.zeros(n, dtype=np.float32)
        p = np.zeros(n, dtype=np.uint32)
        math.band_sums(a.ctypes.data, ld, n, max_lag, ADJ, 0, b.ctypes.data, ld, 1, s.ctypes.data, p.ctypes.data)
        if a is band:
            first = (s.copy(), p.copy())
    assert np.array_equal(first[0].view(np.uint32), s.view(np.uint32)) and np.array_equal(first[1], p)


def test_a_strided_nobs_view_and_a_null_count(math):
    """N(i, d) at nobs[i * pitch + d * stride]: the view the pairwise-complete call passes (row 3 i + 2, column 3 d + 2 of its
    sums); n_pairs may be NULL"""
    n, max_lag = 23, 6
    band, nobs, L, ld = make_band(n, max_lag, 2, 99)
    lds = (3 * L + 2 + 3) // 4 * 4
    sums = np.full((3 * n, lds), 0xDEADBEEF, dtype=np.uint32)
    for i in range(n):
        for d in range(L):
            if i + 1 + d < n:
                sums[3 * i + 2, 3 * d + 2] = nobs[i, d]
    score = np.zeros(n, dtype=np.float32)
    math.band_sums(band.ctypes.data, ld, n, max_lag, ADJ, 0, sums.ctypes.data + 4 * (2 * lds + 2), 3 * lds, 3, score.ctypes.data, None)
    ref, sum_abs, m = _ldscore.band_sums(band, n, max_lag, ADJ, 0, nobs)
    _ldscore.assert_scores(score, m, ref, sum_abs, m)


def test_the_numpy_restatement_on_a_band_worked_by_hand():
    """n = 4, L = 2: rows 0 .. 3 see {1, 2}, {0, 2, 3}, {0, 1, 3}, {1, 2}"""
    x = np.float32(np.nan)
    band = np.array([[0.5, 0.25], [0.125, x], [1.0, 9.0], [9.0, 9.0]], dtype=np.float32)   # (0,1) (0,2) / (1,2) (1,3) / (2,3)
    ref, sum_abs, m = _ldscore.band_sums(band, 4, 2, R2)
    assert ref.tolist() == [0.75, 0.625, 1.375, 1.0] and m.tolist() == [2, 2, 3, 1]
    ref, _, m = _ldscore.band_sums(band, 4, 2, ADJ, n_const=4)
    assert ref.tolist() == [0.75 - 0.25 - 0.375, 0.625 - 0.25 - 0.4375, 1.375 - 0.375 - 0.4375, 1.0] and m.tolist() == [2, 2, 3, 1]
    ref, _, m = _ldscore.band_sums(band, 4, 2, ADJ, nobs=np.array([[4, 2], [3, 7], [0, 7], [7, 7]]))
    assert m.tolist() == [1, 2, 1, 0] and ref.tolist() == [0.25, 0.25 - 0.75, -0.75, 0.0]
