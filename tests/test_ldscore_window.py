"""The window planner of the stratified LD scores (stormbitmaps_amd/csrc/storm_ldscore_window.c) built by the host C compiler
alone — it includes no HIP and no container state — and loaded with ctypes, against np.searchsorted (tests/_ldscore_annot.py):
the empty shapes, ties at the start, in the middle and at the end, max_dist 0 and +inf, a gap wider than max_dist, every
refusal with nothing written behind it, the reported lag, and the symmetry the kernel relies on. No device. The same
planner through the library: STORM_ldscore_window_lag."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _ldscore_annot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_DIST, NOT_FINITE, DECREASING = 0, 1, 2, 3
GUARD = 0xABCDABCD


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a host C compiler"
    so = tmp_path_factory.mktemp("ldscore_window") / "libwindow.so"
    csrc = os.path.join(ROOT, "stormbitmaps_amd", "csrc")
    subprocess.run([cc, "-O2", "-std=gnu11", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", csrc,
                    os.path.join(csrc, "storm_ldscore_window.c"), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.storm_ldscore_window_plan.restype = C.c_int
    lib.storm_ldscore_window_plan.argtypes = [C.c_void_p, C.c_uint64, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_uint64)]
    return lib


def plan(planner, pos, max_dist, bounds=True):
    """(code, lo, hi, lag, bad) with guard values where nothing was written"""
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    n = len(pos)
    lo, hi = np.full(n + 2, GUARD, dtype=np.uint32), np.full(n + 2, GUARD, dtype=np.uint32)
    lag, bad = C.c_uint64(777), C.c_uint64(777)
    code = planner.storm_ldscore_window_plan(pos.ctypes.data if n else None, n, max_dist, lo.ctypes.data if bounds else None,
                                             hi.ctypes.data if bounds else None, C.byref(lag), C.byref(bad))
    assert (lo[n:] == GUARD).all() and (hi[n:] == GUARD).all()                     # nothing behind n, ever
    return code, lo[:n], hi[:n], lag.value, bad.value


def check(planner, pos, max_dist):
    code, lo, hi, lag, _ = plan(planner, pos, max_dist)
    assert code == OK
    want_lo, want_hi = _ldscore_annot.windows(pos, max_dist)
    assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), (pos, max_dist, lo, hi, want_lo, want_hi)
    assert lag == _ldscore_annot.window_lag(want_lo, want_hi)
    i = np.arange(len(pos))
    assert (lo <= i).all() and (i <= hi).all()                                     # a row is inside its own bounds
    assert plan(planner, pos, max_dist, bounds=False)[3] == lag                    # the lag alone, without the arrays
    return lo, hi, lag


def test_the_empty_shapes(planner):
    assert plan(planner, [], 5.0)[0] == OK and plan(planner, [], 5.0)[3] == 0
    lo, hi, lag = check(planner, [3.0], 5.0)
    assert lo.tolist() == [0] and hi.tolist() == [0] and lag == 0
    lo, hi, lag = check(planner, [3.0, 4.0], 5.0)
    assert lo.tolist() == [0, 0] and hi.tolist() == [1, 1] and lag == 1
    lo, hi, lag = check(planner, [3.0, 40.0], 5.0)
    assert lo.tolist() == [0, 1] and hi.tolist() == [0, 1] and lag == 0
    lo, hi, lag = check(planner, [3.0, 3.0], 0.0)                                  # a tie is inside the window at distance 0
    assert lo.tolist() == [0, 0] and hi.tolist() == [1, 1] and lag == 1


def test_ties_at_the_start_in_the_middle_and_at_the_end(planner):
    pos = [1.0, 1.0, 1.0, 2.0, 4.0, 4.0, 5.0, 9.0, 9.0, 9.0]
    for dist in (0.0, 0.5, 1.0, 2.0, 3.0, 4.0, 8.0, 100.0):
        check(planner, pos, dist)
    lo, hi, lag = check(planner, pos, 0.0)                                         # max_dist 0 with ties: the ties alone
    assert lo.tolist() == [0, 0, 0, 3, 4, 4, 6, 7, 7, 7] and hi.tolist() == [2, 2, 2, 3, 5, 5, 6, 9, 9, 9] and lag == 2
    lo, hi, lag = check(planner, [0.0, 1.0, 2.0, 3.0], 0.0)                        # ... and without: every window is empty
    assert lo.tolist() == hi.tolist() == [0, 1, 2, 3] and lag == 0


def test_a_gap_wider_than_max_dist_leaves_empty_windows(planner):
    pos = [0.0, 1.0, 2.0, 50.0, 100.0, 101.0]
    lo, hi, lag = check(planner, pos, 2.0)
    assert (lo[3], hi[3]) == (3, 3)                                                # row 3 is alone
    assert lo.tolist() == [0, 0, 0, 3, 4, 4] and hi.tolist() == [2, 2, 2, 3, 5, 5] and lag == 2


def test_an_infinite_distance_is_the_whole_matrix(planner):
    for n in (1, 2, 7, 100):
        lo, hi, lag = check(planner, np.arange(n) * 3.5, np.inf)
        assert (lo == 0).all() and (hi == n - 1).all() and lag == n - 1
    check(planner, [-1e308, 0.0, 1e308], np.inf)                                   # a difference that overflows is still <= inf


def test_the_reported_lag_is_the_widest_side(planner):
    pos = np.array([0, 10, 11, 12, 13, 14, 30, 31], dtype=np.float64)
    lo, hi, lag = check(planner, pos, 4.0)
    assert lag == 4 and hi[1] - 1 == 4 and 5 - lo[5] == 4
    lo, hi, lag = check(planner, np.arange(50.0), 7.0)
    assert lag == 7
    assert check(planner, np.arange(50.0), 7.5)[2] == 7 and check(planner, np.arange(50.0) * 0.5, 7.0)[2] == 14


def test_every_refusal_writes_nothing(planner):
    good = [0.0, 1.0, 2.0, 3.0]
    for dist in (-1.0, -0.0001, np.nan, -np.inf):
        code, lo, hi, lag, bad = plan(planner, good, dist)
        assert code == BAD_DIST and (lo == GUARD).all() and (hi == GUARD).all() and lag == 777
    assert plan(planner, good, -0.0)[0] == OK                                      # minus zero is zero
    for k in range(4):
        for v in (np.nan, np.inf, -np.inf):
            pos = list(good)
            pos[k] = v
            code, lo, hi, lag, bad = plan(planner, pos, 1.0)
            assert code == NOT_FINITE and bad == k and (lo == GUARD).all() and (hi == GUARD).all() and lag == 777
    for k in range(1, 4):
        pos = list(good)
        pos[k] = pos[k - 1] - 0.5
        code, lo, hi, lag, bad = plan(planner, pos, 1.0)
        assert code == DECREASING and bad == k and (lo == GUARD).all() and (hi == GUARD).all() and lag == 777
    assert plan(planner, [np.nan], -1.0)[0] == BAD_DIST                            # the distance is looked at first
    assert plan(planner, [2.0, 1.0, np.nan], 1.0)[0] == DECREASING                 # then the first offending position
    assert plan(planner, [2.0, 1.0, np.nan], 1.0, bounds=False)[0] == DECREASING


def test_the_windows_are_symmetric_on_200_random_position_sets(planner):
    """j in W(i) <=> i in W(j), the property the kernel relies on (it tests lo[i] behind a row and hi[i] ahead of it) — on
    positions with arbitrary fractions, where pos - max_dist rounds: the planner computes a pair's distance one way only"""
    rng = np.random.default_rng(20)
    for k in range(200):
        n = int(rng.integers(2, 120))
        kind = k % 4
        if kind == 0:
            pos = np.sort(rng.random(n) * 50)
        elif kind == 1:
            pos = np.sort(rng.integers(0, 40, size=n)).astype(np.float64)          # many ties
        elif kind == 2:
            pos = np.cumsum(rng.exponential(1.0, size=n)) * 1e-3 + 1e6             # large offset: differences round
        else:
            pos = np.sort(rng.normal(size=n))
        dist = float(rng.choice([0.0, 0.1, 1.0, 2.5, 1e-3 * rng.random(), 5.0 * rng.random()]))
        code, lo, hi, lag, _ = plan(planner, pos, dist)
        assert code == OK
        i = np.arange(n)
        inside = (lo[:, None] <= i[None, :]) & (i[None, :] <= hi[:, None])         # inside[i, j]: j in [lo[i], hi[i]]
        assert np.array_equal(inside, inside.T), k
        assert np.array_equal(inside, np.abs(pos[:, None] - pos[None, :]) <= dist), k   # and they are the rows within max_dist
        assert (np.diff(lo.astype(np.int64)) >= 0).all() and (np.diff(hi.astype(np.int64)) >= 0).all()
        assert lag == max((i - lo).max(), (hi - i).max())


def test_the_library_reports_the_lag_and_the_refusals(lib):
    f = lib.STORM_ldscore_window_lag
    lag = C.c_uint64(777)
    pos = np.array([0.0, 1.0, 2.0, 50.0, 100.0, 101.0])
    assert f(pos.ctypes.data, 6, 2.0, C.byref(lag)) == 0 and lag.value == 2
    assert f(pos.ctypes.data, 6, float("inf"), C.byref(lag)) == 0 and lag.value == 5
    assert f(None, 0, 2.0, C.byref(lag)) == 0 and lag.value == 0
    lag.value = 777
    assert f(None, 6, 2.0, C.byref(lag)) == -2 and f(pos.ctypes.data, 6, 2.0, None) == -2
    assert f(pos.ctypes.data, 6, -1.0, C.byref(lag)) == -3 and b"max_dist" in lib.STORM_hip_error()
    assert f(pos.ctypes.data, 6, float("nan"), C.byref(lag)) == -3 and b"max_dist" in lib.STORM_hip_error()
    bad = pos.copy()
    bad[4] = 3.0
    assert f(bad.ctypes.data, 6, 2.0, C.byref(lag)) == -3 and b"pos[4]" in lib.STORM_hip_error()
    assert b"decrease" in lib.STORM_hip_error()
    bad[4] = np.inf
    assert f(bad.ctypes.data, 6, 2.0, C.byref(lag)) == -3 and b"pos[4] is not finite" in lib.STORM_hip_error()
    assert lag.value == 777
