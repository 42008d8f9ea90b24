"""The host side of r / r^2 and N between two dosage containers (storm.h: STORM_dosage_square_corr, _square_nobs,
_square_corr_complete and their _device forms) without a GPU: the six symbols are exported and declared, and every refusal
that needs no device returns its code — those of STORM_dosage_square_dot — with nothing written. No CPU fallback: with rows on
both sides and no device visible the calls fail with a reason. What the device computes is tests/test_gpu_dosage_square.py's."""
import os

import numpy as np
import pytest

import stormbitmaps_amd as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORR = ("STORM_dosage_square_corr", "STORM_dosage_square_corr_complete")
NOBS = "STORM_dosage_square_nobs"
SENTINEL = 0xDEADBEEF


def _calls(lib):
    """every one of the six as f(a, b, out, out_rows, out_ld, measure=0)"""
    out = []
    for name in CORR:
        for form in ("", "_device"):
            fn = getattr(lib, name + form)
            out.append((name + form, lambda a, b, o, rows, ld, measure=0, fn=fn: fn(a, b, measure, o, rows, ld)))
    for form in ("", "_device"):
        fn = getattr(lib, NOBS + form)
        out.append((NOBS + form, lambda a, b, o, rows, ld, measure=0, fn=fn: fn(a, b, o, rows, ld)))
    return out


def test_the_six_symbols_are_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "storm.h")).read()
    device_header = open(os.path.join(ROOT, "include", "storm_hip.h")).read()
    for name in CORR + (NOBS,):
        for form in ("", "_device"):
            assert hasattr(lib, name + form), name + form
            assert f"int {name}{form}(STORM_dosage_t* a, STORM_dosage_t* b," in header, name + form
            hip = name.replace("STORM_dosage_square", "storm_hip_square_dosage") + form
            assert hasattr(lib, hip), hip
            assert f"int {hip}(storm_hip_ctx_t* ctx, const storm_hip_matrix_t* a, const storm_hip_matrix_t* b," in device_header, hip


def test_every_refusal_code(lib):
    S = 40
    a, b, wider, empty = (lib.STORM_dosage_new(S), lib.STORM_dosage_new(S), lib.STORM_dosage_new(S + 1), lib.STORM_dosage_new(S))
    good = (np.arange(S, dtype=np.uint8) % 4)
    out = np.full((8, 8), SENTINEL, dtype=np.uint32)
    o = out.ctypes.data
    calls = _calls(lib)
    # NULL handles: -1; NULL out: -2
    for name, call in calls:
        assert call(None, b, o, 8, 8) == -1, name
        assert call(a, None, o, 8, 8) == -1, name
        assert call(None, None, None, 8, 8) == -1, name
        assert call(a, b, None, 8, 8) == -2, name
    # an empty container on either side, or on both: 0, nothing written (no device is needed)
    for _ in range(5):
        assert lib.STORM_dosage_add(a, good.ctypes.data, S) == 0
    for _ in range(6):
        assert lib.STORM_dosage_add(b, good.ctypes.data, S) == 0
    for name, call in calls:
        assert call(empty, empty, o, 8, 8) == 0, name
        assert call(a, empty, o, 8, 8) == 0, name
        assert call(empty, b, o, 8, 8) == 0, name
        assert call(empty, b, o, 0, 6) == 0, name                            # no rows of A: out_rows 0 holds them
    assert (out == SENTINEL).all()
    # too small an output: -4, nothing written
    for name, call in calls:
        assert call(a, b, o, 4, 8) == -4, name                               # out_rows < A's rows
        assert call(a, b, o, 8, 5) == -4, name                               # out_ld < B's rows
        assert call(b, a, o, 5, 8) == -4, name
        assert call(a, empty, o, 4, 8) == -4, name                           # ... checked ahead of the empty side
    assert (out == SENTINEL).all()
    # unequal sample counts: -3, the message names both counts
    zeros = np.zeros(S + 1, dtype=np.uint8)
    assert lib.STORM_dosage_add(wider, zeros.ctypes.data, S + 1) == 0
    for name, call in calls:
        for x, y in ((a, wider), (wider, a)):
            assert call(x, y, o, 8, 8) == -3, name
            msg = lib.STORM_hip_error()
            assert b"samples" in msg and str(S).encode() in msg and str(S + 1).encode() in msg and name.encode() in msg, (name, msg)
    # an unknown measure: -3, STORM_hip_error names it (before any device is asked for)
    for name, call in calls:
        if NOBS in name:
            continue
        for measure in (2, -1, 99):
            assert call(a, b, o, 8, 8, measure) == -3, (name, measure)
            msg = lib.STORM_hip_error()
            assert b"measure" in msg and str(measure).encode() in msg and name.encode() in msg, (name, msg)
            assert call(a, a, o, 8, 8, measure) == -3, (name, measure)       # a == b is allowed, a bad measure is not
    assert (out == SENTINEL).all()
    for d in (a, b, wider, empty):
        lib.STORM_dosage_free(d)


def test_the_device_layer_refuses_a_null_context(lib):
    out = np.zeros(4, dtype=np.uint32)
    o = out.ctypes.data
    for form in ("", "_device"):
        assert getattr(lib, "storm_hip_square_dosage_corr" + form)(None, None, None, 0, 4, o, 4) == -1
        assert getattr(lib, "storm_hip_square_dosage_corr_complete" + form)(None, None, None, 0, 4, o, 4) == -1
        assert getattr(lib, "storm_hip_square_dosage_nobs" + form)(None, None, None, 4, o, 4) == -1
        assert b"NULL context" in lib.storm_hip_last_error()


def test_python_methods_check_their_arguments():
    S = 12
    d, other = sb.StormDosage(S), sb.StormDosage(S)
    assert d.square_corr(other).shape == (0, 0) and d.square_corr(other).dtype == np.float32
    assert d.square_corr(other, "r", complete=True).shape == (0, 0)
    assert d.square_nobs(other).shape == (0, 0) and d.square_nobs(other).dtype == np.uint32
    d.add(np.zeros(S, dtype=np.uint8))
    assert d.square_corr(other).shape == (1, 0) and other.square_nobs(d).shape == (0, 1)
    with pytest.raises(KeyError):
        d.square_corr(other, "pearson")
    with pytest.raises(RuntimeError, match="samples"):
        d.square_corr(sb.StormDosage(S + 1))
    with pytest.raises(RuntimeError, match="samples"):
        d.square_nobs(sb.StormDosage(S + 1))
    d.free()
    other.free()


def test_no_cpu_fallback_without_device(lib):
    if lib.storm_hip_device_count() != 0:
        pytest.skip("a GPU is visible; the loud-failure path is exercised on the CPU container")
    S, n = 100, 3
    h = lib.STORM_dosage_new(S)
    rng = np.random.default_rng(1)
    for _ in range(n):
        r = rng.integers(0, 4, size=S, dtype=np.uint8)
        assert lib.STORM_dosage_add(h, r.ctypes.data, S) == 0
    out = np.full((n, n), SENTINEL, dtype=np.uint32)
    for name, call in _calls(lib):
        assert call(h, h, out.ctypes.data, n, n) == -3, name
        assert lib.STORM_hip_error(), name
    assert (out == SENTINEL).all()
    lib.STORM_dosage_free(h)
    d = sb.StormDosage(S)
    d.add(np.zeros(S, dtype=np.uint8))
    for call in (lambda: d.square_corr(d), lambda: d.square_corr(d, "r", complete=True), lambda: d.square_nobs(d)):
        with pytest.raises(RuntimeError):
            call()
    d.free()
