"""storm_prune_math.h — the edge predicate of lag_band_threshold_kernel and the geometry of a row's adjacency mask — built by
the host C++ compiler and asked about the floats where a comparison can go wrong: NaN, the threshold itself, one ulp either
side of it, thresholds of 0 and 1, negative zero. No device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _prune

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = r"""
#include "storm_prune_math.h"
extern "C" int edge(float rho, float min_r2) { return storm::prune_edge(rho, min_r2) ? 1 : 0; }
extern "C" uint64_t mask_base(uint64_t v, uint64_t L) { return storm::prune_mask_base(v, L); }
extern "C" uint64_t mask_pitch(uint64_t L) { return storm::prune_mask_pitch(L); }
"""


@pytest.fixture(scope="module")
def math(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "a host C++ compiler"
    d = tmp_path_factory.mktemp("prune")
    src, so = d / "prune.cpp", d / "libprune.so"
    src.write_text(SOURCE)
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "stormbitmaps_amd", "csrc"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.edge.restype = C.c_int
    lib.edge.argtypes = [C.c_float, C.c_float]
    for f in (lib.mask_base, lib.mask_pitch):
        f.restype = C.c_uint64
    lib.mask_base.argtypes = [C.c_uint64, C.c_uint64]
    lib.mask_pitch.argtypes = [C.c_uint64]
    return lib


def test_the_edge_predicate_at_the_floats_that_matter(math):
    f32 = np.float32
    nan, inf = f32(np.nan), f32(np.inf)
    for t in (f32(0.0), f32(-0.0), f32(0.2), f32(0.5), f32(1.0), -inf, inf):
        assert math.edge(nan, t) == 0                                    # a NaN rho is never an edge
    for t in (f32(0.2), f32(0.5), f32(1e-30), f32(0.99999994)):
        up, down = np.nextafter(t, inf), np.nextafter(t, -inf)
        assert math.edge(t, t) == 0                                      # exactly at the threshold: not an edge
        assert math.edge(up, t) == 1 and math.edge(down, t) == 0         # one ulp either side
    # min_r2 = 0: every positive r2, the smallest subnormal too; not 0 itself, whatever its sign
    assert math.edge(f32(1e-45), f32(0.0)) == 1 and math.edge(f32(1.0), f32(0.0)) == 1
    for a in (f32(0.0), f32(-0.0)):
        for b in (f32(0.0), f32(-0.0)):
            assert math.edge(a, b) == 0
    # min_r2 = 1: nothing a correlation can reach
    assert math.edge(f32(1.0), f32(1.0)) == 0 and math.edge(f32(0.99999994), f32(1.0)) == 0
    assert math.edge(np.nextafter(f32(1.0), inf), f32(1.0)) == 1         # (a rounding above 1 would be an edge: strict, as floats)
    assert math.edge(f32(0.0), f32(-1.0)) == 1                           # a negative threshold: every number
    rng = np.random.default_rng(3)
    for rho, t in zip(rng.random(300, dtype=np.float32), rng.random(300, dtype=np.float32)):
        assert math.edge(rho, t) == int(rho > t)


def test_the_mask_of_a_row_covers_both_sides_within_the_pitch(math):
    for L in (1, 2, 31, 32, 33, 62, 63, 64, 65, 129, 299, 4096):
        pitch = math.mask_pitch(L)
        assert pitch == 2 * ((L + 31) // 32) + 2 == _prune.mask_pitch(L)
        for v in list(range(0, 200)) + [L - 1, L, L + 1, L + 31, L + 32, L + 33, 5 * L + 7, (1 << 20) - 1]:
            if v < 0:
                continue
            base = math.mask_base(v, L)
            assert base % 32 == 0 and base == 32 * (max(v - L, 0) // 32)
            assert base <= max(v - L, 0) and v + L < base + 32 * pitch   # rows v - L .. v + L all have a bit
