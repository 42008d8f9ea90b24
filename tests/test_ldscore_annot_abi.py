"""The host side of the stratified LD-score calls (storm.h: STORM_dosage_lag_ldscore_annot, _annot_complete, their _device
forms and STORM_ldscore_window_lag; storm_hip.h: storm_hip_lag_band_annot_sums_device and the four
storm_hip_lag_dosage_ldscore_annot calls) without a GPU: the exports, the declarations, the bindings, every refusal code in
its order with the outputs' guard values unchanged behind it, the shim's NULL context, and, no CPU fallback, compute calls
that fail with a reason when no device is visible. The planner is tests/test_ldscore_window.py's, the arithmetic
tests/test_ldscore_annot_math.py's, what the device computes tests/test_gpu_ldscore_annot.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stormbitmaps_amd as sb
from stormbitmaps_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HOST = ("STORM_dosage_lag_ldscore_annot", "STORM_dosage_lag_ldscore_annot_device", "STORM_dosage_lag_ldscore_annot_complete",
        "STORM_dosage_lag_ldscore_annot_complete_device")
SHIM = ("storm_hip_lag_band_annot_sums_device", "storm_hip_lag_dosage_ldscore_annot", "storm_hip_lag_dosage_ldscore_annot_device",
        "storm_hip_lag_dosage_ldscore_annot_complete", "storm_hip_lag_dosage_ldscore_annot_complete_device")
R2, ADJ = 0, 1
GUARD_F, GUARD_U = np.float32(-77.5), np.uint32(0xDEADBEEF)
ROWS, COLS = 8, 3


def test_the_library_exports_and_binds_the_calls(lib):
    for name in HOST + SHIM + ("STORM_ldscore_window_lag",):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "stormbitmaps_amd", "libstorm_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(HOST + SHIM) <= exported and "STORM_ldscore_window_lag" in exported
    assert not {s for s in exported if "_kernel" in s and not s.startswith("storm_hip_")}   # the kernel's handle stays inside
    assert "storm_ldscore_window_plan" not in exported                             # the planner is the library's own
    header = open(os.path.join(ROOT, "include", "storm.h")).read()
    for name in HOST + ("STORM_ldscore_window_lag",):
        assert f"int {name}(" in header, name
    assert "annot[i][c] + score[i][c]" in header                                   # LDSC's l counts the variant itself
    assert "one call per chromosome" in header and "#define STORM_LDSCORE_MAX_ANNOT 1024" in header
    header = open(os.path.join(ROOT, "include", "storm_hip.h")).read()
    for name in SHIM:
        assert f"int {name}(" in header, name
    for cls, names in ((sb.StormDosage, ("lag_ldscore_annot", "ldscore_window_lag")),
                       (sb.HipMatrix, ("lag_dosage_ldscore_annot", "lag_dosage_ldscore_annot_device")),
                       (sb.HipContext, ("lag_band_annot_sums_device",))):
        for name in names:
            assert callable(getattr(cls, name)), name


def outputs():
    return np.full((ROWS, COLS), GUARD_F, dtype=np.float32), np.full(ROWS, GUARD_U, dtype=np.uint32)


def untouched(score, pairs):
    return (score == GUARD_F).all() and (pairs == GUARD_U).all()


def test_every_refusal_code_and_the_empty_shapes(lib):
    S = 40
    h = lib.STORM_dosage_new(S)
    good = np.arange(S, dtype=np.uint8) % 3
    score, pairs = outputs()
    annot = np.ones((ROWS, COLS), dtype=np.float32)
    pos = np.arange(ROWS, dtype=np.float64)
    s, p, a, x = score.ctypes.data, pairs.ctypes.data, annot.ctypes.data, pos.ctypes.data
    for name in HOST:
        f = getattr(lib, name)
        assert f(None, R2, 1, None, 0.0, a, COLS, COLS, s, COLS, p, ROWS) == -1, name      # NULL handle
        assert f(h, R2, 1, None, 0.0, a, COLS, COLS, None, COLS, p, ROWS) == -2, name      # NULL score
        assert f(h, R2, 1, None, 0.0, None, COLS, COLS, s, COLS, p, ROWS) == -2, name      # NULL annot
        assert f(h, R2, 3, None, 0.0, a, COLS, COLS, s, COLS, p, 0) == 0, name             # empty: 0, nothing written, no device
        assert f(h, R2, 3, x, 2.0, a, COLS, COLS, s, COLS, None, 0) == 0, name             # ... n_pairs may be NULL
        assert f(h, R2, 0, x, 2.0, a, COLS, COLS, s, COLS, None, 0) == 0, name             # ... max_lag 0 with positions is a request
        assert f(h, R2, 0, None, 0.0, a, COLS, COLS, s, COLS, p, ROWS) == -3, name         # max_lag 0 without, even when empty
        assert b"max_lag" in lib.STORM_hip_error()
    assert lib.STORM_dosage_add(h, good.ctypes.data, S) == 0
    for name in HOST:
        f = getattr(lib, name)
        assert f(h, ADJ, 3, x, 1.0, a, COLS, COLS, s, COLS, p, 1) == 0, name               # one row: nothing written
        assert f(h, R2, 3, None, 0.0, a, COLS, COLS, s, COLS, p, 0) == -4, name            # out_rows < n
    for _ in range(4):
        assert lib.STORM_dosage_add(h, good.ctypes.data, S) == 0
    assert lib.STORM_dosage_n_rows(h) == 5
    bad_pos = pos.copy()
    bad_pos[3] = 1.5
    nan_pos = pos.copy()
    nan_pos[2] = np.nan
    for name in HOST:
        f = getattr(lib, name)
        assert f(h, R2, 3, None, 0.0, a, COLS, COLS, s, COLS, p, 4) == -4, name            # out_rows < n
        assert f(h, R2, 0, x, -1.0, a, COLS, COLS, s, COLS, p, 4) == -4, name              # ... also with positions and max_lag 0
        assert f(h, R2, 0, None, 0.0, a, COLS, COLS, s, COLS, p, 4) == -3, name            # max_lag 0 is said before the size
        assert b"max_lag" in lib.STORM_hip_error()
        for stat in (2, -1, 99):                                                           # before any device is asked for
            assert f(h, stat, 3, x, -1.0, a, 0, COLS, s, COLS, p, ROWS) == -3, name        # ... and before the new checks
            assert b"stat" in lib.STORM_hip_error()
            assert f(h, stat, 3, None, 0.0, a, COLS, COLS, s, COLS, p, 4) == -4, name      # ... and behind the size check
        # ---- the new checks, in their order
        for n_annot in (0, 1025, 1 << 40):
            assert f(h, R2, 3, x, -1.0, a, n_annot, 1 << 41, s, 1 << 41, p, ROWS) == -3, name
            assert b"n_annot" in lib.STORM_hip_error()
        assert f(h, R2, 3, x, -1.0, a, COLS, COLS - 1, s, COLS, p, ROWS) == -4, name       # annot_ld < n_annot
        assert f(h, R2, 3, x, -1.0, a, COLS, COLS, s, COLS - 1, p, ROWS) == -4, name       # score_ld < n_annot
        for dist in (-1.0, float("nan"), -float("inf")):
            assert f(h, R2, 3, x, dist, a, COLS, COLS, s, COLS, p, ROWS) == -3, name
            assert b"max_dist" in lib.STORM_hip_error()
        assert f(h, R2, 3, nan_pos.ctypes.data, 1.0, a, COLS, COLS, s, COLS, p, ROWS) == -3, name
        assert b"pos[2] is not finite" in lib.STORM_hip_error()
        assert f(h, R2, 3, bad_pos.ctypes.data, 1.0, a, COLS, COLS, s, COLS, p, ROWS) == -3, name
        assert b"pos[3]" in lib.STORM_hip_error() and b"decrease" in lib.STORM_hip_error()
        assert f(h, R2, 2, x, 3.0, a, COLS, COLS, s, COLS, p, ROWS) == -3, name            # the windows need 3 rows: never clipped
        assert b"lag of 3 rows, max_lag is 2" in lib.STORM_hip_error() and name.encode() + b":" in lib.STORM_hip_error()
    for name in HOST[::2]:                                                                 # the host forms read the annotations
        f = getattr(lib, name)
        for v in (np.nan, np.inf, -np.inf):
            bad = annot.copy()
            bad[4, 1] = v
            bad[4, 2] = v
            assert f(h, R2, 3, None, 0.0, bad.ctypes.data, COLS, COLS, s, COLS, p, ROWS) == -3, name
            assert b"annot[4][1] is not finite" in lib.STORM_hip_error()                   # the first (row, column)
    assert untouched(score, pairs)
    lib.STORM_dosage_free(h)


def test_several_device_slots_in_view_are_refused(lib):
    """-5: the outputs live on ONE device. Three slots in view (the same device three times: nothing is asked of the
    hardware, the refusal comes before any device is) — every call names itself and writes nothing; one slot again after"""
    S = 40
    h = lib.STORM_dosage_new(S)
    row = np.arange(S, dtype=np.uint8) % 3
    for _ in range(3):
        assert lib.STORM_dosage_add(h, row.ctypes.data, S) == 0
    score, pairs = outputs()
    annot = np.ones((ROWS, COLS), dtype=np.float32)
    pos = np.arange(ROWS, dtype=np.float64)
    s, p, a, x = score.ctypes.data, pairs.ctypes.data, annot.ctypes.data, pos.ctypes.data
    assert lib.STORM_hip_set_devices(3, (C.c_int * 3)(0, 0, 0)) == 0
    try:
        for name in HOST:
            f = getattr(lib, name)
            for stat, max_lag, px, dist, n_annot, out_rows in ((R2, 2, None, 0.0, COLS, ROWS), (ADJ, 0, x, 1.0, COLS, ROWS),
                                                               (R2, 2, None, 0.0, COLS, 1), (7, 2, x, -1.0, 0, ROWS),
                                                               (R2, 0, None, 0.0, COLS, ROWS)):
                assert f(h, stat, max_lag, px, dist, a, n_annot, COLS, s, COLS, p, out_rows) == -5, name   # ahead of every other check
                assert name.encode() + b":" in lib.STORM_hip_error() and b"ONE device" in lib.STORM_hip_error(), name
            assert f(None, R2, 2, None, 0.0, a, COLS, COLS, s, COLS, p, ROWS) == -1, name  # the NULL checks come first
            assert f(h, R2, 2, None, 0.0, a, COLS, COLS, None, COLS, p, ROWS) == -2, name
    finally:
        assert lib.STORM_hip_set_devices(1, (C.c_int * 1)(0)) == 0
    assert untouched(score, pairs)
    for name in HOST:                                                              # one slot again: the size check answers
        assert getattr(lib, name)(h, R2, 2, None, 0.0, a, COLS, COLS, s, COLS, p, 1) == -4, name
    assert untouched(score, pairs)
    lib.STORM_dosage_free(h)


def test_the_adjusted_statistic_needs_three_samples(lib):
    """N - 2 of the complete-case call is n_samples - 2: refused below 3, before any device is asked for; the
    pairwise-complete call has its N per pair and does not refuse here"""
    score, pairs = outputs()
    annot = np.ones((ROWS, COLS), dtype=np.float32)
    for S in (1, 2):
        h = lib.STORM_dosage_new(S)
        row = np.zeros(S, dtype=np.uint8)
        for _ in range(3):
            assert lib.STORM_dosage_add(h, row.ctypes.data, S) == 0
        for name in HOST[:2]:
            assert getattr(lib, name)(h, ADJ, 2, None, 0.0, annot.ctypes.data, COLS, COLS, score.ctypes.data, COLS, pairs.ctypes.data,
                                      ROWS) == -3, name
            assert b"3 samples" in lib.STORM_hip_error()
        lib.STORM_dosage_free(h)
    assert untouched(score, pairs)


def test_the_device_layer_refuses_a_null_context(lib):
    score, pairs = outputs()
    s, p = score.ctypes.data, pairs.ctypes.data
    assert lib.storm_hip_lag_band_annot_sums_device(None, s, 4, 4, 1, R2, 4, None, 0, 0, None, None, s, COLS, COLS, s, COLS, p) == -1
    assert b"NULL context" in lib.storm_hip_last_error()
    for name in SHIM[1:]:
        assert getattr(lib, name)(None, None, R2, 4, 1, None, None, s, COLS, COLS, s, COLS, p) == -1, name
        assert b"NULL context" in lib.storm_hip_last_error()
    assert untouched(score, pairs)


def test_no_cpu_fallback_without_device(lib):
    if lib.storm_hip_device_count() != 0:
        pytest.skip("a GPU is visible; the loud-failure path is exercised on the CPU container")
    S, n = 100, 3
    h = lib.STORM_dosage_new(S)
    rng = np.random.default_rng(1)
    for _ in range(n):
        r = rng.integers(0, 4, size=S, dtype=np.uint8)
        assert lib.STORM_dosage_add(h, r.ctypes.data, S) == 0
    score, pairs = outputs()
    annot = np.ones((ROWS, COLS), dtype=np.float32)
    pos = np.arange(ROWS, dtype=np.float64)
    for name in HOST:
        for stat in (R2, ADJ):
            for px, max_lag in ((None, 2), (pos.ctypes.data, 0), (pos.ctypes.data, 5)):
                assert getattr(lib, name)(h, stat, max_lag, px, 1.0, annot.ctypes.data, COLS, COLS, score.ctypes.data, COLS,
                                          pairs.ctypes.data, n) == -3, name
                assert lib.STORM_hip_error()
    assert untouched(score, pairs)
    lib.STORM_dosage_free(h)
    d = sb.StormDosage(S)
    d.add(np.zeros(S, dtype=np.uint8))
    d.add(np.full(S, 3, dtype=np.uint8))
    ones = np.ones((2, 2), dtype=np.float32)
    for f in (lambda: d.lag_ldscore_annot(ones, 1), lambda: d.lag_ldscore_annot(ones, 1, "r2_adj"),
              lambda: d.lag_ldscore_annot(ones, complete=True, pos=[0.0, 1.0], max_dist=1.0),
              lambda: d.lag_ldscore_annot(ones, 5, "r2_adj", complete=True, pos=[0.0, 0.0], max_dist=0.0)):
        with pytest.raises(RuntimeError):
            f()
    with pytest.raises(KeyError):
        d.lag_ldscore_annot(ones, 1, "r")


def test_python_answers_the_empty_shapes_and_the_refusals_without_a_device():
    d = sb.StormDosage(10)
    for n in range(2):
        score, pairs = d.lag_ldscore_annot(np.ones((n, 4), dtype=np.float32), 4, "r2_adj", complete=True)
        assert score.shape == (n, 4) and pairs.shape == (n,) and score.dtype == np.float32 and pairs.dtype == np.uint32
        score, pairs = d.lag_ldscore_annot(np.ones((n, 4), dtype=np.float32), pos=np.arange(n), max_dist=3.0)
        assert score.shape == (n, 4) and pairs.shape == (n,)
        d.add(np.ones(10, dtype=np.uint8))
    assert d.n_rows == 2
    ones = np.ones((2, 4), dtype=np.float32)
    with pytest.raises(RuntimeError):
        d.lag_ldscore_annot(ones)                                                  # neither a lag nor positions
    with pytest.raises(RuntimeError):
        d.lag_ldscore_annot(ones, pos=[1.0, 0.0], max_dist=1.0)                    # decreasing
    with pytest.raises(RuntimeError):
        d.lag_ldscore_annot(ones * np.float32(np.inf), 1)
    with pytest.raises(ValueError):
        d.lag_ldscore_annot(ones, pos=[0.0, 1.0])                                  # positions without a distance
    with pytest.raises(ValueError):
        d.lag_ldscore_annot(np.ones((3, 4), dtype=np.float32), 1)                  # a row too many
    assert d.ldscore_window_lag([0.0, 1.0, 2.0, 10.0], 2.0) == 2 and d.ldscore_window_lag([], 2.0) == 0
    with pytest.raises(RuntimeError):
        d.ldscore_window_lag([0.0, -1.0], 2.0)
