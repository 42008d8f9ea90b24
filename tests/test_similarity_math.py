"""The arithmetic of finish_tiles_kernel<SimilarityStat> without a device: storm_similarity_math.h holds the lines the kernel runs
per entry, and a host compiler builds the same lines here (IEEE double division and square root on both sides, no
fast-math, no contraction). Every value is compared with the exactly rounded rational of tests/test_gpu_similarity.py's
generator (`_exact`: Python integers and fractions.Fraction): the one NaN pattern exactly where a measure is undefined,
elsewhere at most 1 float32 ulp — the bound derived there (float64 evaluation, one rounding). What a device adds to this,
the indexing and the calls around the kernel, is tests/test_gpu_similarity.py's."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_gpu_similarity import MEASURES, NAN_BITS, _exact, _ordered

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = r"""
#include "storm_similarity_math.h"
extern "C" void sim_bits(const uint32_t* c, const uint32_t* a, const uint32_t* b, uint64_t n, int measure, uint64_t M,
                         uint32_t* out) {
    for (uint64_t i = 0; i < n; ++i) out[i] = storm::similarity_bits(c[i], a[i], b[i], measure, M);
}
"""


@pytest.fixture(scope="module")
def sim_bits(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "a host C++ compiler"
    d = tmp_path_factory.mktemp("simmath")
    src, so = d / "sim.cpp", d / "libsim.so"
    src.write_text(SOURCE)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "stormbitmaps_amd", "csrc"), str(src), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.sim_bits.restype = None
    lib.sim_bits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_void_p]

    def run(c, a, b, measure, M):
        c, a, b = (np.ascontiguousarray(x, dtype=np.uint32) for x in (c, a, b))
        out = np.empty(c.size, dtype=np.uint32)
        lib.sim_bits(c.ctypes.data, a.ctypes.data, b.ctypes.data, c.size, MEASURES.index(measure), M, out.ctypes.data)
        return out
    return run


def _cases(rng, M, n, near_independence):
    """(c, a, b) a pair of sets over M bits could have; near_independence: M c within a few counts of a b"""
    a = rng.integers(1, M, size=n, dtype=np.int64)
    b = rng.integers(1, M, size=n, dtype=np.int64)
    lo, hi = np.maximum(0, a + b - M), np.minimum(a, b)
    if near_independence:
        mid = np.array([int(x) * int(y) // M for x, y in zip(a, b)], dtype=np.int64)
        c = np.clip(mid + rng.integers(-2, 3, size=n), lo, hi)
    else:
        c = np.clip(lo + (rng.random(n) * (hi - lo + 1)).astype(np.int64), lo, hi)
    return c, a, b


@pytest.mark.parametrize("measure", MEASURES)
def test_every_measure_is_within_one_ulp_of_the_exact_rational(sim_bits, measure):
    rng = np.random.default_rng(100 + MEASURES.index(measure))
    worst = 0
    for M, near in ((64, False), (4096, False), (65536, False), (65536, True), (100003, True), (1 << 31, True),
                    (1 << 32, False), (1 << 32, True), ((1 << 32) - 5, True)):
        c, a, b = _cases(rng, M, 1500, near)
        got = sim_bits(c, a, b, measure, M)
        want = [_exact(measure, x, y, z, M) for x, y, z in zip(c, a, b)]
        assert all(w is not None for w in want)          # 0 < a, b < M: every measure is defined
        want = np.array(want, dtype=np.float32).view(np.uint32)
        ulps = np.abs(_ordered(got) - _ordered(want))
        assert int(ulps.max()) <= 1, (measure, M, near, int(np.argmax(ulps)))
        worst = max(worst, int(ulps.max()))
    print(f"{measure}: worst error {worst} ulp")


def test_nan_exactly_where_the_measure_is_undefined(sim_bits):
    M = 64
    # (c, a, b): empty rows, full rows, a row beyond the universe, identical and complementary halves
    rows = [(0, 0, 0), (0, 0, 32), (0, 32, 0), (32, 64, 32), (32, 32, 64), (64, 64, 64), (32, 32, 32), (0, 32, 32),
            (3, 70, 5), (2, 32, 3)]
    c, a, b = (np.array(x) for x in zip(*rows))
    for measure in MEASURES:
        got = sim_bits(c, a, b, measure, M)
        want = [_exact(measure, x, y, z, M) for x, y, z in rows]
        for g, w, row in zip(got, want, rows):
            if w is None:
                assert int(g) == NAN_BITS, (measure, row)
            else:
                assert abs(int(_ordered(np.array([g]))[0]) - int(_ordered(np.array([w]).view(np.uint32))[0])) <= 1, (measure, row)
    undefined = {m: [w is None for w in (_exact(m, x, y, z, M) for x, y, z in rows)] for m in MEASURES}
    assert undefined["jaccard"] == [True] + [False] * 9
    assert undefined["cosine"] == [True, True, True] + [False] * 7
    assert undefined["ld_d"] == [False] * 10
    assert undefined["ld_r2"] == [True, True, True, True, True, True, False, False, True, False]
