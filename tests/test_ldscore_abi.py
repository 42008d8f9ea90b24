"""The host side of the LD-score calls (storm.h: STORM_dosage_lag_ldscore, _ldscore_complete and their _device forms;
storm_hip.h: storm_hip_lag_band_sums_device and the four storm_hip_lag_dosage_ldscore calls) without a GPU: the exports,
the declarations, the bindings, every refusal code in its order with the outputs' guard values unchanged behind it, the
shim's NULL context, and, no CPU fallback, compute calls that fail with a reason when no device is visible. The
reduction's arithmetic is tests/test_ldscore_math.py's, what the device computes tests/test_gpu_ldscore.py's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import stormbitmaps_amd as sb
from stormbitmaps_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HOST = ("STORM_dosage_lag_ldscore", "STORM_dosage_lag_ldscore_device", "STORM_dosage_lag_ldscore_complete",
        "STORM_dosage_lag_ldscore_complete_device")
COMPLETE = HOST[2:]
SHIM = ("storm_hip_lag_band_sums_device", "storm_hip_lag_dosage_ldscore", "storm_hip_lag_dosage_ldscore_device",
        "storm_hip_lag_dosage_ldscore_complete", "storm_hip_lag_dosage_ldscore_complete_device")
R2, ADJ = 0, 1
GUARD_F, GUARD_U = np.float32(-77.5), np.uint32(0xDEADBEEF)


def test_the_library_exports_and_binds_the_calls(lib):
    for name in HOST + SHIM:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "stormbitmaps_amd", "libstorm_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(HOST + SHIM) <= exported
    assert not {s for s in exported if "_kernel" in s and not s.startswith("storm_hip_")}   # the kernel's handle stays inside
    header = open(os.path.join(ROOT, "include", "storm.h")).read()
    for name in HOST:
        assert f"int {name}(" in header, name
    assert "#define STORM_LDSCORE_R2 0" in header and "#define STORM_LDSCORE_R2_ADJ 1" in header
    assert "1 + score" in header                                                   # LDSC's l counts the variant itself
    header = open(os.path.join(ROOT, "include", "storm_hip.h")).read()
    for name in SHIM:
        assert f"int {name}(" in header, name


def outputs(n=8):
    return np.full(n, GUARD_F, dtype=np.float32), np.full(n, GUARD_U, dtype=np.uint32)


def untouched(score, pairs):
    return (score == GUARD_F).all() and (pairs == GUARD_U).all()


def test_every_refusal_code_and_the_empty_shapes(lib):
    S = 40
    h = lib.STORM_dosage_new(S)
    good = np.arange(S, dtype=np.uint8) % 3
    score, pairs = outputs()
    s, p = score.ctypes.data, pairs.ctypes.data
    for name in HOST:
        f = getattr(lib, name)
        assert f(None, R2, 1, s, p, 8) == -1, name                                 # NULL handle
        assert f(h, R2, 1, None, p, 8) == -2, name                                 # NULL score
        assert f(h, R2, 3, s, p, 0) == 0, name                                     # empty: 0, nothing written, no device
        assert f(h, R2, 3, s, None, 0) == 0, name                                  # ... n_pairs may be NULL
        assert f(h, R2, 0, s, p, 8) == -3, name                                    # max_lag 0, even when empty
        assert b"max_lag" in lib.STORM_hip_error()
        assert f(h, R2, 0, s, p, 0) == -3, name
    assert lib.STORM_dosage_add(h, good.ctypes.data, S) == 0
    for name in HOST:
        f = getattr(lib, name)
        assert f(h, ADJ, 3, s, p, 1) == 0, name                                    # one row: nothing written
        assert f(h, R2, 3, s, p, 0) == -4, name                                    # out_len < n
    for _ in range(4):
        assert lib.STORM_dosage_add(h, good.ctypes.data, S) == 0
    assert lib.STORM_dosage_n_rows(h) == 5
    for name in HOST:
        f = getattr(lib, name)
        assert f(h, R2, 3, s, p, 4) == -4, name                                    # out_len < n
        assert f(h, ADJ, 100, s, None, 4) == -4, name
        assert f(h, R2, 0, s, p, 4) == -3, name                                    # max_lag 0 is said before the size
        assert b"max_lag" in lib.STORM_hip_error()
        for stat in (2, -1, 99):                                                   # before any device is asked for
            assert f(h, stat, 3, s, p, 8) == -3, name
            assert b"stat" in lib.STORM_hip_error()
            assert f(h, stat, 3, s, p, 4) == -4, name                              # ... and behind the size check
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
    s, p = score.ctypes.data, pairs.ctypes.data
    assert lib.STORM_hip_set_devices(3, (C.c_int * 3)(0, 0, 0)) == 0
    try:
        for name in HOST:
            f = getattr(lib, name)
            for stat, max_lag, n_pairs, out_len in ((R2, 2, p, 8), (ADJ, 100, None, 8), (R2, 2, p, 1), (7, 2, p, 8), (R2, 0, p, 8)):
                assert f(h, stat, max_lag, s, n_pairs, out_len) == -5, name        # ahead of the size, stat and max_lag checks
                assert name.encode() + b":" in lib.STORM_hip_error() and b"ONE device" in lib.STORM_hip_error(), name
            assert f(None, R2, 2, s, p, 8) == -1 and f(h, R2, 2, None, p, 8) == -2, name   # the NULL checks come first
    finally:
        assert lib.STORM_hip_set_devices(1, (C.c_int * 1)(0)) == 0
    assert untouched(score, pairs)
    for name in HOST:                                                              # one slot again: the size check answers
        assert getattr(lib, name)(h, R2, 2, s, p, 1) == -4, name
    assert untouched(score, pairs)
    lib.STORM_dosage_free(h)


def test_the_adjusted_statistic_needs_three_samples(lib):
    """N - 2 of the complete-case call is n_samples - 2: refused below 3, before any device is asked for; the
    pairwise-complete call has its N per pair and does not refuse here"""
    score, pairs = outputs()
    s, p = score.ctypes.data, pairs.ctypes.data
    for S in (1, 2):
        h = lib.STORM_dosage_new(S)
        row = np.zeros(S, dtype=np.uint8)
        for _ in range(3):
            assert lib.STORM_dosage_add(h, row.ctypes.data, S) == 0
        for name in HOST[:2]:
            assert getattr(lib, name)(h, ADJ, 2, s, p, 8) == -3, name
            assert b"3 samples" in lib.STORM_hip_error()
        lib.STORM_dosage_free(h)
    assert untouched(score, pairs)


def test_the_device_layer_refuses_a_null_context(lib):
    score, pairs = outputs()
    s, p = score.ctypes.data, pairs.ctypes.data
    assert lib.storm_hip_lag_band_sums_device(None, s, 4, 4, 1, R2, 4, None, 0, 0, s, p) == -1
    assert b"NULL context" in lib.storm_hip_last_error()
    for name in SHIM[1:]:
        assert getattr(lib, name)(None, None, R2, 4, 1, s, p) == -1, name
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
    for name in HOST:
        for stat in (R2, ADJ):
            assert getattr(lib, name)(h, stat, 2, score.ctypes.data, pairs.ctypes.data, n) == -3, name
            assert lib.STORM_hip_error()
    assert untouched(score, pairs)
    lib.STORM_dosage_free(h)
    d = sb.StormDosage(S)
    d.add(np.zeros(S, dtype=np.uint8))
    d.add(np.full(S, 3, dtype=np.uint8))
    for f in (lambda: d.lag_ldscore(1), lambda: d.lag_ldscore(1, "r2_adj"), lambda: d.lag_ldscore(1, complete=True),
              lambda: d.lag_ldscore(5, "r2_adj", complete=True)):
        with pytest.raises(RuntimeError):
            f()
    with pytest.raises(KeyError):
        d.lag_ldscore(1, "r")


def test_python_answers_the_empty_shapes_without_a_device():
    d = sb.StormDosage(10)
    for _ in range(2):
        score, pairs = d.lag_ldscore(4, "r2_adj", complete=True)
        assert score.shape == pairs.shape == (d.n_rows,) and score.dtype == np.float32 and pairs.dtype == np.uint32
        d.add(np.ones(10, dtype=np.uint8))
    with pytest.raises(RuntimeError):
        d.lag_ldscore(0)
