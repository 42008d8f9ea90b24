"""The host side of the sparse LD report (storm.h: STORM_dosage_lag_corr_sparse, _complete and their _device forms; storm_hip.h:
storm_hip_lag_band_sparse_device and the four storm_hip_lag_dosage_corr_sparse calls) without a GPU: the exports, the
declarations, the bindings, every refusal code in its documented order with guard elements unchanged around the outputs, the
shim's NULL context, the shapes that need no device (no rows, one row), and, no CPU fallback, compute calls that fail with a
reason when no device is visible. The index helpers are tests/test_lag_sparse_math.py's, what the device computes
tests/test_gpu_lag_sparse.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stormbitmaps_amd as sb
from stormbitmaps_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HOST = ("STORM_dosage_lag_corr_sparse", "STORM_dosage_lag_corr_sparse_device", "STORM_dosage_lag_corr_sparse_complete",
        "STORM_dosage_lag_corr_sparse_complete_device")
SHIM = ("storm_hip_lag_band_sparse_device", "storm_hip_lag_dosage_corr_sparse", "storm_hip_lag_dosage_corr_sparse_device",
        "storm_hip_lag_dosage_corr_sparse_complete", "storm_hip_lag_dosage_corr_sparse_complete_device")
GUARD_R, GUARD_C, GUARD_V = np.uint64(0x7777777777777777), np.uint32(0xDEADBEEF), np.float32(-7.5)
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
    assert {s for s in exported if "sparse" in s and "lag" in s} == set(HOST + SHIM)   # these and no other
    assert not {s for s in exported if "_kernel" in s and not s.startswith("storm_hip_")}   # the kernels' handles stay inside
    header = open(os.path.join(ROOT, "include", "storm.h")).read()
    for name in HOST:
        assert f"int {name}(" in header, name
    assert "exactly at the\n *             threshold is NOT listed (PLINK's filter is >=" in header   # strict, and said so
    assert "nothing is ever written at or beyond" in header
    header = open(os.path.join(ROOT, "include", "storm_hip.h")).read()
    for name in SHIM:
        assert f"int {name}(" in header, name
    for cls, names in ((sb.StormDosage, ("lag_corr_sparse",)), (sb.HipContext, ("lag_band_sparse_device",)),
                       (sb.HipMatrix, ("lag_dosage_corr_sparse", "lag_dosage_corr_sparse_device"))):
        for name in names:
            assert callable(getattr(cls, name)), name


def outputs():
    """row_start, col, val and n_pairs with guard elements before and after what a call may write"""
    return (np.full(ROWS + 3, GUARD_R, dtype=np.uint64), np.full(ROWS + 2, GUARD_C, dtype=np.uint32),
            np.full(ROWS + 2, GUARD_V, dtype=np.float32), np.full(3, GUARD_R, dtype=np.uint64))


def untouched(rows, col, val, total=None):
    return (rows == GUARD_R).all() and (col == GUARD_C).all() and (val == GUARD_V).all() and (total is None or (total == GUARD_R).all())


def call(lib, name, h, min_r2, max_lag, pos, dist, r, out_rows, c, v, cap, t):
    """the host forms take n_pairs, the _device forms do not"""
    f = getattr(lib, name)
    return f(h, min_r2, max_lag, pos, dist, r, out_rows, c, v, cap) if name.endswith("_device") else \
        f(h, min_r2, max_lag, pos, dist, r, out_rows, c, v, cap, t)


def test_every_refusal_code_in_its_order_and_the_shapes_without_a_device(lib):
    S = 40
    h = lib.STORM_dosage_new(S)
    good = np.arange(S, dtype=np.uint8) % 3
    rows, col, val, total = outputs()
    pos = np.arange(ROWS, dtype=np.float64)
    r, c, v, t, x = rows.ctypes.data + 8, col.ctypes.data + 4, val.ctypes.data + 4, total.ctypes.data + 8, pos.ctypes.data
    for name in HOST:
        host = not name.endswith("_device")
        assert call(lib, name, None, 0.2, 1, None, 0.0, r, ROWS, c, v, ROWS, t) == -1, name        # NULL handle
        assert call(lib, name, h, 0.2, 1, None, 0.0, None, ROWS, c, v, ROWS, t) == -2, name        # NULL row_start
        if host:
            assert call(lib, name, h, 0.2, 1, None, 0.0, r, ROWS, c, v, ROWS, None) == -2, name    # NULL n_pairs
        assert call(lib, name, h, 0.2, 1, None, 0.0, r, ROWS, None, v, ROWS, t) == -2, name        # exactly one of col / val
        assert call(lib, name, h, 0.2, 1, None, 0.0, r, ROWS, c, None, ROWS, t) == -2, name
        assert call(lib, name, h, 0.2, 1, None, 0.0, r, ROWS, None, None, 1, t) == -2, name        # a capacity without them
        assert call(lib, name, h, 0.2, 0, None, 0.0, r, ROWS, c, v, ROWS, t) == -3, name           # max_lag 0 without positions
        assert b"max_lag" in lib.STORM_hip_error() and name.encode() + b":" in lib.STORM_hip_error()
        assert call(lib, name, h, 0.2, 3, None, 0.0, r, 0, None, None, 0, t) == 0, name           # no rows, no room: nothing written
    assert untouched(rows, col, val) and total.tolist() == [GUARD_R, 0, GUARD_R]                   # (*n_pairs = 0 alone)
    for name in HOST[::2]:                                                                         # no row, host forms: no device
        one_r, one_c, one_v, one_t = outputs()
        a = (one_r.ctypes.data + 8, ROWS, one_c.ctypes.data + 4, one_v.ctypes.data + 4, ROWS, one_t.ctypes.data + 8)
        assert call(lib, name, h, 0.2, 3, None, 0.0, *a) == 0, name
        assert one_r.tolist() == [GUARD_R, 0] + [GUARD_R] * (ROWS + 1) and one_t.tolist() == [GUARD_R, 0, GUARD_R]
        assert untouched(one_r[2:], one_c, one_v)
        assert call(lib, name, h, 0.2, 0, x, 2.0, *a) == 0, name                                   # max_lag 0 with positions: a request
    assert lib.STORM_dosage_add(h, good.ctypes.data, S) == 0
    for name in HOST[::2]:                                                                         # one row, host forms: no device
        one_r, one_c, one_v, one_t = outputs()
        a = (one_r.ctypes.data + 8, 2, one_c.ctypes.data + 4, one_v.ctypes.data + 4, ROWS, one_t.ctypes.data + 8)
        assert call(lib, name, h, 0.2, 3, None, 0.0, *a) == 0, name
        assert one_r.tolist() == [GUARD_R, 0, 0] + [GUARD_R] * ROWS and one_t.tolist() == [GUARD_R, 0, GUARD_R]
        assert untouched(one_r[3:], one_c, one_v)
        one_r, one_c, one_v, one_t = outputs()
        assert call(lib, name, h, -1.0, 0, x, 1.0, one_r.ctypes.data + 8, 5, None, None, 0, one_t.ctypes.data + 8) == 0, name   # count-only
        assert one_r.tolist() == [GUARD_R, 0, 0] + [GUARD_R] * ROWS and one_t.tolist() == [GUARD_R, 0, GUARD_R]
    for name in HOST:
        assert call(lib, name, h, 0.2, 3, None, 0.0, r, 1, c, v, ROWS, t) == -4, name              # out_rows < n + 1
    for _ in range(4):
        assert lib.STORM_dosage_add(h, good.ctypes.data, S) == 0
    assert lib.STORM_dosage_n_rows(h) == 5
    bad_pos = pos.copy()
    bad_pos[3] = 1.5
    nan_pos = pos.copy()
    nan_pos[2] = np.nan
    total[1] = GUARD_R
    for name in HOST:
        assert call(lib, name, h, 0.2, 3, None, 0.0, r, 5, c, v, ROWS, t) == -4, name              # out_rows < n + 1
        assert call(lib, name, h, NAN, 0, x, -1.0, r, 5, c, v, ROWS, t) == -4, name                # ... ahead of everything behind it
        assert call(lib, name, h, 0.2, 0, None, 0.0, r, 5, c, v, ROWS, t) == -3, name              # max_lag 0 is said before the size
        assert b"max_lag" in lib.STORM_hip_error()
        assert call(lib, name, h, NAN, 3, x, -1.0, r, ROWS, c, v, ROWS, t) == -3, name             # a NaN threshold, before the positions
        assert b"min_r2 is NaN" in lib.STORM_hip_error()
        for dist in (-1.0, NAN, -float("inf")):
            assert call(lib, name, h, 0.2, 3, x, dist, r, ROWS, c, v, ROWS, t) == -3, name
            assert b"max_dist" in lib.STORM_hip_error()
        assert call(lib, name, h, 0.2, 3, nan_pos.ctypes.data, 1.0, r, ROWS, c, v, ROWS, t) == -3, name
        assert b"pos[2] is not finite" in lib.STORM_hip_error()
        assert call(lib, name, h, 0.2, 3, bad_pos.ctypes.data, 1.0, r, ROWS, c, v, ROWS, t) == -3, name
        assert b"pos[3]" in lib.STORM_hip_error() and b"decrease" in lib.STORM_hip_error()
        assert call(lib, name, h, 0.2, 2, x, 3.0, r, ROWS, c, v, ROWS, t) == -3, name              # the windows need 3 rows: never clipped
        assert b"lag of 3 rows, max_lag is 2" in lib.STORM_hip_error() and name.encode() + b":" in lib.STORM_hip_error()
    assert untouched(rows, col, val, total)
    lib.STORM_dosage_free(h)


def test_several_device_slots_in_view_are_refused(lib):
    """-5: the outputs live on ONE device. Three slots in view (the same device three times: nothing is asked of the
    hardware) — every call names itself and writes nothing; one slot again after"""
    S = 40
    h = lib.STORM_dosage_new(S)
    row = np.arange(S, dtype=np.uint8) % 3
    for _ in range(3):
        assert lib.STORM_dosage_add(h, row.ctypes.data, S) == 0
    rows, col, val, total = outputs()
    r, c, v, t = rows.ctypes.data + 8, col.ctypes.data + 4, val.ctypes.data + 4, total.ctypes.data + 8
    pos = np.arange(ROWS, dtype=np.float64)
    assert lib.STORM_hip_set_devices(3, (C.c_int * 3)(0, 0, 0)) == 0
    try:
        for name in HOST:
            for min_r2, max_lag, px, dist, out_rows in ((0.2, 2, None, 0.0, ROWS), (NAN, 0, pos.ctypes.data, -1.0, ROWS),
                                                        (0.2, 2, None, 0.0, 1), (0.2, 0, None, 0.0, ROWS)):
                assert call(lib, name, h, min_r2, max_lag, px, dist, r, out_rows, c, v, ROWS, t) == -5, name   # ahead of every other check
                assert name.encode() + b":" in lib.STORM_hip_error() and b"ONE device" in lib.STORM_hip_error(), name
            assert call(lib, name, None, 0.2, 2, None, 0.0, r, ROWS, c, v, ROWS, t) == -1, name    # the NULL checks come first
            assert call(lib, name, h, 0.2, 2, None, 0.0, None, ROWS, c, v, ROWS, t) == -2, name
            assert call(lib, name, h, 0.2, 2, None, 0.0, r, ROWS, c, None, ROWS, t) == -2, name
    finally:
        assert lib.STORM_hip_set_devices(1, (C.c_int * 1)(0)) == 0
    for name in HOST:                                                                              # one slot again: the size check answers
        assert call(lib, name, h, 0.2, 2, None, 0.0, r, 3, c, v, ROWS, t) == -4, name
    assert untouched(rows, col, val, total)
    lib.STORM_dosage_free(h)


def test_the_device_layer_refuses_a_null_context(lib):
    rows, col, val, total = outputs()
    r, c, v, t = rows.ctypes.data + 8, col.ctypes.data + 4, val.ctypes.data + 4, total.ctypes.data + 8
    assert lib.storm_hip_lag_band_sparse_device(None, v, 4, 4, 1, 0.2, None, None, r, c, v, ROWS) == -1
    assert b"NULL context" in lib.storm_hip_last_error()
    for name in SHIM[1:]:
        args = (None, None, 4, 1, 0.2, None, None, r, c, v, ROWS)
        assert getattr(lib, name)(*args) == -1 if name.endswith("_device") else getattr(lib, name)(*args, t) == -1, name
        assert b"NULL context" in lib.storm_hip_last_error()
    assert untouched(rows, col, val, total)


def test_no_cpu_fallback_without_device(lib):
    if lib.storm_hip_device_count() != 0:
        pytest.skip("a GPU is visible; the loud-failure path is exercised on the CPU container")
    S, n = 100, 3
    h = lib.STORM_dosage_new(S)
    rng = np.random.default_rng(1)
    for _ in range(n):
        row = rng.integers(0, 4, size=S, dtype=np.uint8)
        assert lib.STORM_dosage_add(h, row.ctypes.data, S) == 0
    rows, col, val, total = outputs()
    r, c, v, t = rows.ctypes.data + 8, col.ctypes.data + 4, val.ctypes.data + 4, total.ctypes.data + 8
    pos = np.arange(ROWS, dtype=np.float64)
    for name in HOST:
        for px, max_lag in ((None, 2), (pos.ctypes.data, 0), (pos.ctypes.data, 5)):
            for cc, vv, cap in ((c, v, ROWS), (None, None, 0)):
                assert call(lib, name, h, 0.2, max_lag, px, 1.0, r, n + 1, cc, vv, cap, t) == -3, name
                assert lib.STORM_hip_error()
    assert untouched(rows, col, val) and total.tolist() in ([GUARD_R, 0, GUARD_R], [GUARD_R, GUARD_R, GUARD_R])
    lib.STORM_dosage_free(h)
    d = sb.StormDosage(S)
    d.add(np.zeros(S, dtype=np.uint8))
    d.add(np.full(S, 3, dtype=np.uint8))
    for f in (lambda: d.lag_corr_sparse(0.2, 1), lambda: d.lag_corr_sparse(0.5, 1, capacity=4),
              lambda: d.lag_corr_sparse(0.2, complete=True, pos=[0.0, 1.0], max_dist=1.0)):
        with pytest.raises(RuntimeError):
            f()


def test_python_answers_the_small_shapes_and_the_refusals_without_a_device():
    d = sb.StormDosage(10)
    for kw in ({}, {"capacity": 0}, {"capacity": 3, "complete": True}, {"pos": np.zeros(0), "max_dist": 3.0, "max_lag": None}):
        rows, col, val = d.lag_corr_sparse(0.2, **{"max_lag": 4, **kw})
        assert rows.tolist() == [0] and rows.dtype == np.uint64
        assert col.shape == (0,) and col.dtype == np.uint32 and val.shape == (0,) and val.dtype == np.float32
    d.add(np.ones(10, dtype=np.uint8))
    rows, col, val = d.lag_corr_sparse(0.2, 4)
    assert rows.tolist() == [0, 0] and col.size == 0 and val.size == 0              # one row has no pair
    assert d.lag_corr_sparse(-1.0, pos=[5.0], max_dist=0.0, complete=True)[0].tolist() == [0, 0]
    d.add(np.ones(10, dtype=np.uint8))
    with pytest.raises(RuntimeError):
        d.lag_corr_sparse(0.2)                                                     # neither a lag nor positions
    with pytest.raises(RuntimeError):
        d.lag_corr_sparse(float("nan"), 1)
    with pytest.raises(RuntimeError):
        d.lag_corr_sparse(0.2, pos=[1.0, 0.0], max_dist=1.0)                       # decreasing
    with pytest.raises(ValueError):
        d.lag_corr_sparse(0.2, pos=[0.0, 1.0])                                     # positions without a distance
