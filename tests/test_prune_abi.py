"""The host side of the prune / clump calls (storm.h: STORM_dosage_lag_prune, _complete and their _device forms; storm_hip.h:
storm_hip_lag_band_prune_device and the four storm_hip_lag_dosage_prune calls) without a GPU: the exports, the declarations,
the bindings, every refusal code in its documented order with guard bytes unchanged around the outputs, the shim's NULL
context, the shapes that need no device (no rows, one row), and, no CPU fallback, compute calls that fail with a reason when
no device is visible. The planner is tests/test_prune_order.py's, the predicate tests/test_prune_math.py's, what the device
computes tests/test_gpu_prune.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stormbitmaps_amd as sb
from stormbitmaps_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HOST = ("STORM_dosage_lag_prune", "STORM_dosage_lag_prune_device", "STORM_dosage_lag_prune_complete",
        "STORM_dosage_lag_prune_complete_device")
SHIM = ("storm_hip_lag_band_prune_device", "storm_hip_lag_dosage_prune", "storm_hip_lag_dosage_prune_device",
        "storm_hip_lag_dosage_prune_complete", "storm_hip_lag_dosage_prune_complete_device")
GUARD_K, GUARD_O = np.uint8(0x77), np.uint32(0xDEADBEEF)
ROWS = 8
NAN = float("nan")


def test_the_library_exports_and_binds_the_calls(lib):
    for name in HOST + SHIM:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "stormbitmaps_amd", "libstorm_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(HOST + SHIM) <= exported
    assert not {s for s in exported if "_kernel" in s and not s.startswith("storm_hip_")}   # the kernels' handles stay inside
    assert "storm_prune_order_plan" not in exported                                # the planner is the library's own
    header = open(os.path.join(ROOT, "include", "storm.h")).read()
    for name in HOST:
        assert f"int {name}(" in header, name
    assert "#define STORM_PRUNE_MAX_ROWS 1048576" in header
    assert "NOT PLINK's --indep-pairwise" in header                                # which greedy this is, and which it is not
    assert "keep[0] = 1 and owner[0] = 0" in header and "CONSTANT row" in header
    header = open(os.path.join(ROOT, "include", "storm_hip.h")).read()
    for name in SHIM:
        assert f"int {name}(" in header, name
    for cls, names in ((sb.StormDosage, ("lag_prune",)), (sb.HipContext, ("lag_band_prune_device",))):
        for name in names:
            assert callable(getattr(cls, name)), name


def outputs():
    """keep and owner with guard elements before and after the ROWS a call may write"""
    return np.full(ROWS + 2, GUARD_K, dtype=np.uint8), np.full(ROWS + 2, GUARD_O, dtype=np.uint32)


def untouched(keep, owner):
    return (keep == GUARD_K).all() and (owner == GUARD_O).all()


def test_every_refusal_code_in_its_order_and_the_shapes_without_a_device(lib):
    S = 40
    h = lib.STORM_dosage_new(S)
    good = np.arange(S, dtype=np.uint8) % 3
    keep, owner = outputs()
    pos = np.arange(ROWS, dtype=np.float64)
    prio = np.arange(ROWS, dtype=np.float32)
    k, o, x, p = keep.ctypes.data + 1, owner.ctypes.data + 4, pos.ctypes.data, prio.ctypes.data
    for name in HOST:
        f = getattr(lib, name)
        assert f(None, 0.2, 1, None, 0.0, None, k, o, ROWS) == -1, name                    # NULL handle
        assert f(h, 0.2, 1, None, 0.0, None, None, o, ROWS) == -2, name                    # NULL keep
        assert f(h, 0.2, 3, None, 0.0, None, k, None, 0) == 0, name                        # empty: 0, nothing written, no device
        assert f(h, 0.2, 3, x, 2.0, p, k, o, 0) == 0, name
        assert f(h, 0.2, 0, x, 2.0, None, k, o, 0) == 0, name                              # max_lag 0 with positions is a request
        assert f(h, 0.2, 0, None, 0.0, None, k, o, ROWS) == -3, name                       # max_lag 0 without, even when empty
        assert b"max_lag" in lib.STORM_hip_error() and name.encode() + b":" in lib.STORM_hip_error()
    assert untouched(keep, owner)
    assert lib.STORM_dosage_add(h, good.ctypes.data, S) == 0
    for name in HOST[::2]:                                                                 # one row, host forms: no device is asked
        f = getattr(lib, name)
        one_k, one_o = outputs()
        assert f(h, 0.2, 3, None, 0.0, None, one_k.ctypes.data + 1, one_o.ctypes.data + 4, 1) == 0, name
        assert one_k.tolist() == [GUARD_K, 1] + [GUARD_K] * ROWS and one_o.tolist() == [GUARD_O, 0] + [GUARD_O] * ROWS
        one_k, one_o = outputs()
        assert f(h, 0.2, 0, x, 1.0, p, one_k.ctypes.data + 1, None, 5) == 0, name          # owner may be NULL
        assert one_k.tolist() == [GUARD_K, 1] + [GUARD_K] * ROWS and untouched(one_k[2:], one_o)
    for name in HOST:
        assert getattr(lib, name)(h, 0.2, 3, None, 0.0, None, k, o, 0) == -4, name         # out_len < n
    for _ in range(4):
        assert lib.STORM_dosage_add(h, good.ctypes.data, S) == 0
    assert lib.STORM_dosage_n_rows(h) == 5
    bad_pos = pos.copy()
    bad_pos[3] = 1.5
    nan_pos = pos.copy()
    nan_pos[2] = np.nan
    nan_prio = prio.copy()
    nan_prio[1] = nan_prio[4] = np.nan
    for name in HOST:
        f = getattr(lib, name)
        assert f(h, 0.2, 3, None, 0.0, None, k, o, 4) == -4, name                          # out_len < n
        assert f(h, NAN, 0, x, -1.0, nan_prio.ctypes.data, k, o, 4) == -4, name            # ... ahead of everything behind it
        assert f(h, 0.2, 0, None, 0.0, None, k, o, 4) == -3, name                          # max_lag 0 is said before the size
        assert b"max_lag" in lib.STORM_hip_error()
        assert f(h, NAN, 3, x, -1.0, nan_prio.ctypes.data, k, o, ROWS) == -3, name         # a NaN threshold, before the positions
        assert b"min_r2 is NaN" in lib.STORM_hip_error()
        for dist in (-1.0, NAN, -float("inf")):
            assert f(h, 0.2, 3, x, dist, nan_prio.ctypes.data, k, o, ROWS) == -3, name     # ... the positions before the priorities
            assert b"max_dist" in lib.STORM_hip_error()
        assert f(h, 0.2, 3, nan_pos.ctypes.data, 1.0, p, k, o, ROWS) == -3, name
        assert b"pos[2] is not finite" in lib.STORM_hip_error()
        assert f(h, 0.2, 3, bad_pos.ctypes.data, 1.0, p, k, o, ROWS) == -3, name
        assert b"pos[3]" in lib.STORM_hip_error() and b"decrease" in lib.STORM_hip_error()
        assert f(h, 0.2, 2, x, 3.0, nan_prio.ctypes.data, k, o, ROWS) == -3, name          # the windows need 3 rows: never clipped
        assert b"lag of 3 rows, max_lag is 2" in lib.STORM_hip_error() and name.encode() + b":" in lib.STORM_hip_error()
        assert f(h, 0.2, 3, x, 3.0, nan_prio.ctypes.data, k, o, ROWS) == -3, name          # a NaN priority: the first such row
        assert b"priority[1] is NaN" in lib.STORM_hip_error()
        assert f(h, 0.2, 3, None, 0.0, nan_prio.ctypes.data, k, None, ROWS) == -3, name
        assert b"priority[1] is NaN" in lib.STORM_hip_error()
    assert untouched(keep, owner)
    lib.STORM_dosage_free(h)


def test_several_device_slots_in_view_are_refused(lib):
    """-5: the outputs live on ONE device. Three slots in view (the same device three times: nothing is asked of the
    hardware) — every call names itself and writes nothing; one slot again after"""
    S = 40
    h = lib.STORM_dosage_new(S)
    row = np.arange(S, dtype=np.uint8) % 3
    for _ in range(3):
        assert lib.STORM_dosage_add(h, row.ctypes.data, S) == 0
    keep, owner = outputs()
    k, o = keep.ctypes.data + 1, owner.ctypes.data + 4
    pos = np.arange(ROWS, dtype=np.float64)
    assert lib.STORM_hip_set_devices(3, (C.c_int * 3)(0, 0, 0)) == 0
    try:
        for name in HOST:
            f = getattr(lib, name)
            for min_r2, max_lag, px, dist, out_len in ((0.2, 2, None, 0.0, ROWS), (NAN, 0, pos.ctypes.data, -1.0, ROWS),
                                                       (0.2, 2, None, 0.0, 1), (0.2, 0, None, 0.0, ROWS)):
                assert f(h, min_r2, max_lag, px, dist, None, k, o, out_len) == -5, name    # ahead of every other check
                assert name.encode() + b":" in lib.STORM_hip_error() and b"ONE device" in lib.STORM_hip_error(), name
            assert f(None, 0.2, 2, None, 0.0, None, k, o, ROWS) == -1, name                # the NULL checks come first
            assert f(h, 0.2, 2, None, 0.0, None, None, o, ROWS) == -2, name
    finally:
        assert lib.STORM_hip_set_devices(1, (C.c_int * 1)(0)) == 0
    for name in HOST:                                                                      # one slot again: the size check answers
        assert getattr(lib, name)(h, 0.2, 2, None, 0.0, None, k, o, 1) == -4, name
    assert untouched(keep, owner)
    lib.STORM_dosage_free(h)


def test_the_device_layer_refuses_a_null_context(lib):
    keep, owner = outputs()
    k, o = keep.ctypes.data + 1, owner.ctypes.data + 4
    assert lib.storm_hip_lag_band_prune_device(None, k, 4, 4, 1, 0.2, None, None, None, k, o) == -1
    assert b"NULL context" in lib.storm_hip_last_error()
    for name in SHIM[1:]:
        assert getattr(lib, name)(None, None, 4, 1, 0.2, None, None, None, k, o) == -1, name
        assert b"NULL context" in lib.storm_hip_last_error()
    assert untouched(keep, owner)


def test_no_cpu_fallback_without_device(lib):
    if lib.storm_hip_device_count() != 0:
        pytest.skip("a GPU is visible; the loud-failure path is exercised on the CPU container")
    S, n = 100, 3
    h = lib.STORM_dosage_new(S)
    rng = np.random.default_rng(1)
    for _ in range(n):
        r = rng.integers(0, 4, size=S, dtype=np.uint8)
        assert lib.STORM_dosage_add(h, r.ctypes.data, S) == 0
    keep, owner = outputs()
    k, o = keep.ctypes.data + 1, owner.ctypes.data + 4
    pos = np.arange(ROWS, dtype=np.float64)
    prio = np.arange(ROWS, dtype=np.float32)
    for name in HOST:
        for px, max_lag in ((None, 2), (pos.ctypes.data, 0), (pos.ctypes.data, 5)):
            for pr in (None, prio.ctypes.data):
                assert getattr(lib, name)(h, 0.2, max_lag, px, 1.0, pr, k, o, n) == -3, name
                assert lib.STORM_hip_error()
    assert untouched(keep, owner)
    lib.STORM_dosage_free(h)
    d = sb.StormDosage(S)
    d.add(np.zeros(S, dtype=np.uint8))
    d.add(np.full(S, 3, dtype=np.uint8))
    for f in (lambda: d.lag_prune(0.2, 1), lambda: d.lag_prune(0.5, 1, priority=[1.0, 2.0], owner=True),
              lambda: d.lag_prune(0.2, complete=True, pos=[0.0, 1.0], max_dist=1.0)):
        with pytest.raises(RuntimeError):
            f()


def test_python_answers_the_small_shapes_and_the_refusals_without_a_device():
    d = sb.StormDosage(10)
    keep = d.lag_prune(0.2, 4, complete=True)
    assert keep.shape == (0,) and keep.dtype == np.uint8
    keep, owner = d.lag_prune(0.2, pos=np.zeros(0), max_dist=3.0, priority=np.zeros(0), owner=True)
    assert keep.shape == (0,) and owner.shape == (0,) and owner.dtype == np.uint32
    d.add(np.ones(10, dtype=np.uint8))
    keep, owner = d.lag_prune(0.2, 4, owner=True)
    assert keep.tolist() == [1] and owner.tolist() == [0]                          # one row is kept and owns itself
    assert d.lag_prune(1.0, pos=[5.0], max_dist=0.0, priority=[-np.inf], complete=True).tolist() == [1]
    d.add(np.ones(10, dtype=np.uint8))
    with pytest.raises(RuntimeError):
        d.lag_prune(0.2)                                                           # neither a lag nor positions
    with pytest.raises(RuntimeError):
        d.lag_prune(float("nan"), 1)
    with pytest.raises(RuntimeError):
        d.lag_prune(0.2, pos=[1.0, 0.0], max_dist=1.0)                             # decreasing
    with pytest.raises(RuntimeError):
        d.lag_prune(0.2, 1, priority=[0.0, np.nan])
    with pytest.raises(ValueError):
        d.lag_prune(0.2, pos=[0.0, 1.0])                                           # positions without a distance
    with pytest.raises(ValueError):
        d.lag_prune(0.2, 1, priority=[1.0, 2.0, 3.0])                              # a priority too many
