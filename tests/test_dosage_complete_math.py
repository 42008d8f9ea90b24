"""The arithmetic of the pairwise-complete dosage correlation without a device: storm_dosage_math.h holds the lines that
dosage_complete_finish_kernel runs per entry (dosage_corr_complete_bits) and that dosage_split_missing_kernel runs per
word (dosage_split_word, dosage_valid_mask), and a host compiler builds the same lines here, as tests/test_dosage_math.py
does for the complete-case formula. Every correlation is compared with the exactly rounded rational (Python integers,
fractions.Fraction, `_rn32`): NaN (0x7FC00000) exactly when dx or dy is 0, elsewhere at most 1 float32 ulp — the project's
bound for "integers exact, a handful of f64 operations, one rounding". The word split is compared with a per-sample loop."""
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
extern "C" void complete_bits(const uint32_t* c, uint64_t n, int measure, uint32_t* out) {
    for (uint64_t k = 0; k < n; ++k)
        out[k] = storm::dosage_corr_complete_bits(c[6 * k], c[6 * k + 1], c[6 * k + 2], c[6 * k + 3], c[6 * k + 4], c[6 * k + 5],
                                                  measure);
}
extern "C" void corr_bits(const uint32_t* c, uint64_t n, int measure, uint64_t S, uint32_t* out) {
    for (uint64_t k = 0; k < n; ++k)
        out[k] = storm::dosage_corr_bits(c[5 * k], c[5 * k + 1], c[5 * k + 2], c[5 * k + 3], c[5 * k + 4], measure, S);
}
extern "C" void split_row(const uint64_t* x, uint32_t n_words, uint32_t stride_words, uint64_t n_samples, uint64_t* g,
                          uint64_t* h, uint64_t* m) {
    for (uint32_t w = 0; w < stride_words; ++w)
        storm::dosage_split_word(w < n_words ? x[w] : 0, storm::dosage_valid_mask(w, n_words, n_samples), g + w, h + w, m + w);
}
"""


@pytest.fixture(scope="module")
def math(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "a host C++ compiler"
    d = tmp_path_factory.mktemp("dosagecomplete")
    src, so = d / "complete.cpp", d / "libcomplete.so"
    src.write_text(SOURCE)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "stormbitmaps_amd", "csrc"), str(src), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.complete_bits.restype = lib.corr_bits.restype = lib.split_row.restype = None
    lib.complete_bits.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    lib.corr_bits.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_void_p]
    lib.split_row.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64] + [C.c_void_p] * 3
    return lib


def complete_bits(math, cases, measure):
    c = np.ascontiguousarray(cases, dtype=np.uint32).reshape(-1, 6)
    out = np.empty(len(c), dtype=np.uint32)
    math.complete_bits(c.ctypes.data, len(c), MEASURES.index(measure), out.ctypes.data)
    return out


def exact(measure, case):
    """float32 of one entry from Python integers; None = undefined (dx or dy is 0)"""
    P, N, sx, sy, qx, qy = (int(x) for x in case)
    num, dx, dy = N * P - sx * sy, N * qx - sx * sx, N * qy - sy * sy
    assert dx >= 0 and dy >= 0
    if dx == 0 or dy == 0:
        return None
    q = Fraction(num * num, dx * dy)
    if measure == "r2":
        return _rn32(q)
    v = _rn32(q, root=True)
    return np.float32(-v) if num < 0 else v


def joint_case(rng, S, N=None, weights=None):
    """(P, N, sx, sy, qx, qy) of two rows of S samples from a random joint table of the 16 code pairs (code 3 = missing); N:
    exactly that many samples present in both rows (the rest has a 3 on one side at least)"""
    if N is None:
        n = rng.multinomial(S, rng.dirichlet(np.ones(16) if weights is None else weights)).reshape(4, 4).astype(object)
    else:
        n = np.zeros((4, 4), dtype=object)
        n[:3, :3] = rng.multinomial(N, rng.dirichlet(np.ones(9) if weights is None else weights)).reshape(3, 3)
        rest = rng.multinomial(S - N, rng.dirichlet(np.ones(7))).astype(object)
        n[3, :] = rest[:4]
        n[:3, 3] = rest[4:]
    assert int(n.sum()) == S
    shared = n[:3, :3]
    v = np.arange(3, dtype=object)
    N_ = int(shared.sum())
    P = int(sum(shared[a, b] * a * b for a in range(3) for b in range(3)))
    sx, qx = int((shared.sum(axis=1) * v).sum()), int((shared.sum(axis=1) * v * v).sum())
    sy, qy = int((shared.sum(axis=0) * v).sum()), int((shared.sum(axis=0) * v * v).sum())
    return P, N_, sx, sy, qx, qy


def independent_case(rng, S):
    """a joint table that is (almost) the product of its margins: num within a few counts of 0, of either sign"""
    a, b = rng.dirichlet(np.ones(4)), rng.dirichlet(np.ones(4))
    return joint_case(rng, S, weights=np.outer(a, b).ravel() * 1e6 + 1e-3)


def ulps(got, want):
    return np.abs(_ordered(got) - _ordered(np.asarray(want, dtype=np.float32).view(np.uint32)))


@pytest.mark.parametrize("measure", MEASURES)
def test_both_measures_are_within_one_ulp_of_the_exact_rational(math, measure):
    rng = np.random.default_rng(700 + MEASURES.index(measure))
    worst, negative, defined, undefined = 0, 0, 0, 0
    for S in (1, 2, 3, 33, 1000, 65536, 100003, (1 << 24) - 1, 1 << 24):
        cases = [joint_case(rng, S) for _ in range(400)] + [independent_case(rng, S) for _ in range(400)]
        cases += [joint_case(rng, S, N=N) for N in (0, 1, 2) if N <= S for _ in range(40)]
        got = complete_bits(math, cases, measure)
        want = [exact(measure, c) for c in cases]
        nan = np.array([w is None for w in want])
        assert np.array_equal(got == NAN_BITS, nan), (measure, S)
        assert np.array_equal((got & 0x7FFFFFFF) > 0x7F800000, nan), (measure, S)   # no other NaN pattern either
        for c, w in zip(cases, want):
            assert c[1] >= 2 or w is None, c                    # N = 0 and N = 1 are always undefined
        if (~nan).any():
            u = ulps(got[~nan], [w for w in want if w is not None])
            assert int(u.max()) <= 1, (measure, S, cases[int(np.flatnonzero(~nan)[np.argmax(u)])])
            worst = max(worst, int(u.max()))
        negative += sum(1 for c in cases if c[1] * c[0] < c[2] * c[3])
        defined += int((~nan).sum())
        undefined += int(nan.sum())
    assert negative > 500 and defined > 4000 and undefined > 200     # both signs, mostly defined, and the NaN cases were seen
    print(f"{measure}: worst error {worst} ulp")


def test_every_term_stays_below_2_pow_51_at_the_largest_shape(math):
    """S = N = 2^24, every shared sample a 2 but one: the integers at their largest (the header's bound on every term), dx at
    its smallest non-zero"""
    S = 1 << 24
    low = (2 * S - 1, 4 * S - 3)         # all 2s, one sample of 1: (s, q)
    lower = (2 * S - 2, 4 * S - 4)       # all 2s, one sample of 0
    cases = {
        "same sample": (4 * (S - 1) + 0, S, low[0], lower[0], low[1], lower[1]),
        "different samples": (4 * (S - 2) + 2 + 0, S, low[0], lower[0], low[1], lower[1]),
        "a row against itself": (4 * (S - 1) + 1, S, low[0], low[0], low[1], low[1]),
        "constant on the shared samples": (4 * S - 2, S, 2 * S, low[0], 4 * S, low[1]),
        "nothing shared": (0, 0, 0, 0, 0, 0),
        "one shared sample": (2, 1, 1, 2, 1, 4),
    }
    for name, (P, N, sx, sy, qx, qy) in cases.items():
        assert max(N * P, sx * sy, N * qx, sx * sx, N * qy, sy * sy) < 1 << 51, name
    for measure in MEASURES:
        got = complete_bits(math, list(cases.values()), measure)
        for g, (name, c) in zip(got, cases.items()):
            w = exact(measure, c)
            if w is None:
                assert int(g) == NAN_BITS, (measure, name)
            else:
                assert int(ulps(np.array([g]), [w])[0]) <= 1, (measure, name, hex(int(g)), w)
    assert [exact("r", c) is None for c in cases.values()] == [False, False, False, True, True, True]
    assert exact("r", cases["different samples"]) < 0 and exact("r", cases["a row against itself"]) == 1.0
    # N = 2, the smallest defined shape: g_i = 0 1, g_j = 1 0 -> r = -1; num = 0 -> +0.0 under both measures
    assert complete_bits(math, [(0, 2, 1, 1, 1, 1)], "r").view(np.float32)[0] == -1.0
    assert complete_bits(math, [(0, 2, 1, 1, 1, 1)], "r2").view(np.float32)[0] == 1.0
    for measure in MEASURES:
        assert int(complete_bits(math, [(1, 4, 2, 2, 2, 2)], measure)[0]) == 0


@pytest.mark.parametrize("measure", MEASURES)
def test_without_a_missing_sample_the_bits_are_those_of_the_complete_case_formula(math, measure):
    """N = S, sx = s_i, sy = s_j, qx = q_i, qy = q_j: bit-identical to dosage_corr_bits, NaNs included"""
    rng = np.random.default_rng(900)
    for S in (1, 2, 7, 1000, 65536, 1 << 24):
        cases = []
        for k in range(1500):
            c = joint_case(rng, S, N=S) if k % 2 else joint_case(rng, S, N=S, weights=np.outer(rng.dirichlet(np.ones(3)),
                                                                                              rng.dirichlet(np.ones(3))).ravel() * 1e6 + 1e-3)
            assert c[1] == S
            cases.append(c)
        old = np.ascontiguousarray([(P, sx, qx, sy, qy) for (P, N, sx, sy, qx, qy) in cases], dtype=np.uint32)
        want = np.empty(len(cases), dtype=np.uint32)
        math.corr_bits(old.ctypes.data, len(cases), MEASURES.index(measure), S, want.ctypes.data)
        got = complete_bits(math, cases, measure)
        assert np.array_equal(got, want), (measure, S)
        assert S < 3 or (got != NAN_BITS).sum() > 1000


def split_by_hand(values, n_samples, stride_words):
    """the three rows sample by sample: g, h, m as lists of `stride_words` Python integers"""
    g, h, m = [0] * stride_words, [0] * stride_words, [0] * stride_words
    for s in range(n_samples):
        x, w, sh = int(values[s]), s // 32, 2 * (s % 32)
        g[w] |= (0 if x == 3 else x) << sh
        h[w] |= (1 if x == 2 else 0) << sh
        m[w] |= (0 if x == 3 else 1) << sh
    return g, h, m


@pytest.mark.parametrize("tail", range(1, 33))
def test_the_word_split_against_a_per_sample_loop_for_every_tail_length(math, tail):
    """rows of 2 words and `tail` samples in the third, three pad words behind; the tail samples of the last word and the pad
    words are absent from M whatever the row holds (row 0: all 3s, row 1: all 0s — present everywhere —, row 2: every
    code)"""
    n_words, stride = 3, 6
    S = 64 + tail
    rng = np.random.default_rng(tail)
    for row in range(6):
        values = [np.full(S, 3), np.zeros(S), np.arange(S) % 4][row] if row < 3 else rng.integers(0, 4, size=S)
        x = np.zeros(n_words, dtype=np.uint64)
        for s in range(S):
            x[s // 32] |= np.uint64(int(values[s]) << (2 * (s % 32)))
        g, h, m = (np.full(stride, 0xDEADBEEFDEADBEEF, dtype=np.uint64) for _ in range(3))
        math.split_row(x.ctypes.data, n_words, stride, S, g.ctypes.data, h.ctypes.data, m.ctypes.data)
        wg, wh, wm = split_by_hand(values, S, stride)
        assert g.tolist() == wg and h.tolist() == wh and m.tolist() == wm, (tail, row)
        assert not any(m[n_words:]) and not any(g[n_words:]) and not any(h[n_words:])      # pad words
        assert int(m[n_words - 1]) >> (2 * tail) == 0                                       # tail samples
        assert sum(bin(int(w)).count("1") for w in m) == int((np.asarray(values) != 3).sum())
        # g^2 = g + 2 h sample by sample
        for s in range(S):
            gv = (int(g[s // 32]) >> (2 * (s % 32))) & 3
            hv = (int(h[s // 32]) >> (2 * (s % 32))) & 3
            assert gv * gv == gv + 2 * hv and gv <= 2 and hv <= 1
