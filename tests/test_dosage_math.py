"""The arithmetic of finish_tiles_kernel<DosageStat, true> without a device: storm_dosage_math.h holds the lines the kernel runs per entry
(the Pearson correlation r and r^2 of two rows of 2-bit dosages from their dot product, sums and sums of squares), and a
host compiler builds the same lines here (IEEE double division and square root on both sides, no fast-math, no
contraction). Every value is compared with the exactly rounded rational (Python integers, fractions.Fraction, the
`_rn32` of tests/test_gpu_similarity.py): the one NaN pattern exactly where a row is constant, elsewhere at most
1 float32 ulp — the project's bound for "integers exact, a handful of f64 operations, one rounding"."""
import ctypes as C
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests.test_gpu_similarity import NAN_BITS, _ordered, _rn32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURES = ("r2", "r")   # STORM_DOSAGE_R2 = 0, STORM_DOSAGE_R = 1

SOURCE = r"""
#include "storm_dosage_math.h"
extern "C" void corr_bits(const uint32_t* p, const uint32_t* si, const uint32_t* qi, const uint32_t* sj, const uint32_t* qj,
                          uint64_t n, int measure, uint64_t S, uint32_t* out) {
    for (uint64_t k = 0; k < n; ++k) out[k] = storm::dosage_corr_bits(p[k], si[k], qi[k], sj[k], qj[k], measure, S);
}
"""


@pytest.fixture(scope="module")
def corr_bits(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "a host C++ compiler"
    d = tmp_path_factory.mktemp("dosagemath")
    src, so = d / "dosage.cpp", d / "libdosage.so"
    src.write_text(SOURCE)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "stormbitmaps_amd", "csrc"), str(src), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.corr_bits.restype = None
    lib.corr_bits.argtypes = [C.c_void_p] * 5 + [C.c_uint64, C.c_int, C.c_uint64, C.c_void_p]

    def run(cases, measure, S):
        cols = [np.ascontiguousarray([c[k] for c in cases], dtype=np.uint32) for k in range(5)]
        out = np.empty(len(cases), dtype=np.uint32)
        lib.corr_bits(*(c.ctypes.data for c in cols), len(cases), MEASURES.index(measure), S, out.ctypes.data)
        return out
    return run


def exact(measure, case, S):
    """float32 of one entry from Python integers; None = undefined (a constant row)"""
    P, si, qi, sj, qj = (int(x) for x in case)
    num, di, dj = S * P - si * sj, S * qi - si * si, S * qj - sj * sj
    assert di >= 0 and dj >= 0
    if di == 0 or dj == 0:
        return None
    q = Fraction(num * num, di * dj)
    if measure == "r2":
        return _rn32(q)
    v = _rn32(q, root=True)
    return np.float32(-v) if num < 0 else v


def joint_case(rng, S, weights=None):
    """(P, s_i, q_i, s_j, q_j) of two rows of S values 0 .. 3 from a random joint table of the 16 value pairs"""
    w = rng.dirichlet(np.ones(16) if weights is None else weights)
    n = rng.multinomial(S, w).reshape(4, 4).astype(object)
    v = np.arange(4, dtype=object)
    P = int(sum(n[a, b] * a * b for a in range(4) for b in range(4)))
    si, qi = int((n.sum(axis=1) * v).sum()), int((n.sum(axis=1) * v * v).sum())
    sj, qj = int((n.sum(axis=0) * v).sum()), int((n.sum(axis=0) * v * v).sum())
    return P, si, qi, sj, qj


def independent_case(rng, S):
    """two rows whose joint table is (almost) the product of its margins: num within a few counts of 0, of either sign"""
    a, b = rng.dirichlet(np.ones(4)), rng.dirichlet(np.ones(4))
    return joint_case(rng, S, weights=np.outer(a, b).ravel() * 1e6 + 1e-3)


def ulps(got, want):
    return np.abs(_ordered(got) - _ordered(np.asarray(want, dtype=np.float32).view(np.uint32)))


@pytest.mark.parametrize("measure", MEASURES)
def test_both_measures_are_within_one_ulp_of_the_exact_rational(corr_bits, measure):
    rng = np.random.default_rng(500 + MEASURES.index(measure))
    worst, negative, defined = 0, 0, 0
    for S in (1, 2, 3, 33, 1000, 65536, 100003, (1 << 24) - 1, 1 << 24):
        cases = [joint_case(rng, S) for _ in range(600)] + [independent_case(rng, S) for _ in range(600)]
        got = corr_bits(cases, measure, S)
        want = [exact(measure, c, S) for c in cases]
        nan = np.array([w is None for w in want])
        assert np.array_equal(got == NAN_BITS, nan), (measure, S)
        assert np.array_equal((got & 0x7FFFFFFF) > 0x7F800000, nan), (measure, S)   # no other NaN pattern either
        if (~nan).any():
            u = ulps(got[~nan], [w for w in want if w is not None])
            assert int(u.max()) <= 1, (measure, S, cases[int(np.flatnonzero(~nan)[np.argmax(u)])])
            worst = max(worst, int(u.max()))
        negative += sum(1 for c in cases if S * c[0] < c[1] * c[3])
        defined += int((~nan).sum())
    assert negative > 500 and defined > 5000      # both signs of num and mostly defined entries were seen
    print(f"{measure}: worst error {worst} ulp")


def test_the_extremes(corr_bits):
    """S = 2^24 with rows of all 3s but one sample (every integer at its largest, d at its smallest non-zero), num < 0,
    num = 0, and the constant rows: NaN is 0x7FC00000 exactly when d_i or d_j is 0"""
    S = 1 << 24
    low2 = (3 * S - 1, 9 * S - 5)        # all 3s, one sample of 2: (s, q)
    low1 = (3 * S - 2, 9 * S - 8)        # all 3s, one sample of 1
    cases = {
        "same sample, 2 and 1": (9 * (S - 1) + 2, *low2, *low1),          # num = 2 S - 2 > 0 ... r = 1
        "different samples": (9 * (S - 2) + 6 + 3, *low2, *low1),          # num = -2 < 0
        "a row against itself": (9 * (S - 1) + 4, *low2, *low2),           # r = 1 exactly
        "all 3s against one low": (9 * (S - 1) + 6, 3 * S, 9 * S, *low2),  # constant row: NaN
        "all 0s": (0, 0, 0, *low1),
        "both constant": (S, S, S, S, S),
    }
    for name, c in cases.items():
        P, si, qi, sj, qj = c
        assert max(S * P, si * sj, S * qi, si * si) < 9 * (1 << 48) + 1, name     # the header's bound on every term
    for measure in MEASURES:
        got = corr_bits(list(cases.values()), measure, S)
        for g, (name, c) in zip(got, cases.items()):
            w = exact(measure, c, S)
            if w is None:
                assert int(g) == NAN_BITS, (measure, name)
            else:
                assert int(ulps(np.array([g]), [w])[0]) <= 1, (measure, name, hex(int(g)), w)
    assert [exact("r", c, S) is None for c in cases.values()] == [False, False, False, True, True, True]
    assert exact("r", cases["different samples"], S) < 0 and exact("r", cases["a row against itself"], S) == 1.0
    # num = 0: two independent halves, S = 4, v_i = 0 0 1 1, v_j = 0 1 0 1 -> +0.0 under both measures, no sign
    for measure in MEASURES:
        assert int(corr_bits([(1, 2, 2, 2, 2)], measure, 4)[0]) == 0
    # num < 0 at the smallest shapes: v_i = 0 1, v_j = 1 0 -> r = -1, r^2 = 1
    assert corr_bits([(0, 1, 1, 1, 1)], "r", 2).view(np.float32)[0] == -1.0
    assert corr_bits([(0, 1, 1, 1, 1)], "r2", 2).view(np.float32)[0] == 1.0
