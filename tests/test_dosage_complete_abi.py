"""The host side of the dosage container's rectangle and of its calls for rows with missing genotypes (storm.h:
STORM_dosage_square_dot, _row_missing, _pairw_nobs, _pairw_corr_complete) without a GPU: every refusal code — those of
STORM_dosage_pairw_corr — and, no CPU fallback, compute calls that fail with a reason when no device is visible. What the
device computes is tests/test_gpu_dosage_complete.py's."""
import numpy as np
import pytest

import stormbitmaps_amd as sb


def test_the_missing_code_is_declared():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "storm.h")).read()
    assert "#define STORM_DOSAGE_MISSING 3" in header


def test_every_refusal_code(lib):
    S = 40
    h, other, wider = lib.STORM_dosage_new(S), lib.STORM_dosage_new(S), lib.STORM_dosage_new(S + 1)
    good = np.arange(S, dtype=np.uint8) % 4
    out = np.full((4, 4), 77, dtype=np.uint32)
    fout = np.zeros((4, 4), dtype=np.float32)
    miss = np.full(8, 77, dtype=np.uint32)
    o, f = out.ctypes.data, fout.ctypes.data
    # NULL handle: -1
    assert lib.STORM_dosage_square_dot(None, h, o, 4, 4) == -1
    assert lib.STORM_dosage_square_dot(h, None, o, 4, 4) == -1
    assert lib.STORM_dosage_square_dot_device(None, h, o, 4, 4) == -1
    assert lib.STORM_dosage_square_dot_device(h, None, o, 4, 4) == -1
    assert lib.STORM_dosage_row_missing(None, miss.ctypes.data) == -1
    assert lib.STORM_dosage_pairw_nobs(None, o, 4, 4) == -1
    assert lib.STORM_dosage_pairw_nobs_device(None, o, 4, 4) == -1
    assert lib.STORM_dosage_pairw_corr_complete(None, 0, f, 4, 4) == -1
    assert lib.STORM_dosage_pairw_corr_complete_device(None, 0, f, 4, 4) == -1
    # NULL out: -2
    assert lib.STORM_dosage_square_dot(h, other, None, 4, 4) == -2
    assert lib.STORM_dosage_square_dot_device(h, other, None, 4, 4) == -2
    assert lib.STORM_dosage_row_missing(h, None) == -2
    assert lib.STORM_dosage_pairw_nobs(h, None, 4, 4) == -2
    assert lib.STORM_dosage_pairw_nobs_device(h, None, 4, 4) == -2
    assert lib.STORM_dosage_pairw_corr_complete(h, 0, None, 4, 4) == -2
    assert lib.STORM_dosage_pairw_corr_complete_device(h, 1, None, 4, 4) == -2
    # empty containers and fewer than two rows: 0, nothing written (no device is needed)
    assert lib.STORM_dosage_square_dot(h, other, o, 4, 4) == 0
    assert lib.STORM_dosage_row_missing(h, miss.ctypes.data) == 0
    assert lib.STORM_dosage_pairw_nobs(h, o, 4, 4) == 0
    assert lib.STORM_dosage_add(h, good.ctypes.data, S) == 0
    assert lib.STORM_dosage_square_dot(h, other, o, 4, 4) == 0              # B is still empty
    assert lib.STORM_dosage_square_dot(other, h, o, 4, 4) == 0              # ... and so is A
    assert lib.STORM_dosage_pairw_nobs(h, o, 4, 4) == 0
    assert lib.STORM_dosage_pairw_corr_complete(h, 1, f, 4, 4) == 0
    assert (out == 77).all() and (fout == 0).all() and (miss == 77).all()
    # too small an output: -4, nothing written
    for _ in range(4):
        assert lib.STORM_dosage_add(h, good.ctypes.data, S) == 0
    for _ in range(6):
        assert lib.STORM_dosage_add(other, good.ctypes.data, S) == 0
    assert lib.STORM_dosage_n_rows(h) == 5 and lib.STORM_dosage_n_rows(other) == 6
    assert lib.STORM_dosage_square_dot(h, other, o, 4, 8) == -4             # out_rows < A's rows
    assert lib.STORM_dosage_square_dot(h, other, o, 8, 5) == -4             # out_ld < B's rows
    assert lib.STORM_dosage_square_dot_device(h, other, o, 5, 5) == -4
    assert lib.STORM_dosage_pairw_nobs(h, o, 4, 8) == -4
    assert lib.STORM_dosage_pairw_nobs(h, o, 8, 4) == -4
    assert lib.STORM_dosage_pairw_nobs_device(h, o, 4, 4) == -4
    assert lib.STORM_dosage_pairw_corr_complete(h, 0, f, 4, 4) == -4
    assert lib.STORM_dosage_pairw_corr_complete_device(h, 0, f, 5, 4) == -4
    assert (out == 77).all() and (fout == 0).all()
    # an unknown measure: -3, before any device is asked for
    big = np.zeros((5, 5), dtype=np.float32)
    for measure in (2, -1, 99):
        assert lib.STORM_dosage_pairw_corr_complete(h, measure, big.ctypes.data, 5, 5) == -3
        assert b"measure" in lib.STORM_hip_error()
        assert lib.STORM_dosage_pairw_corr_complete_device(h, measure, big.ctypes.data, 5, 5) == -3
    # containers of different sample counts: -3, before any device is asked for
    zeros = np.zeros(S + 1, dtype=np.uint8)
    assert lib.STORM_dosage_add(wider, zeros.ctypes.data, S + 1) == 0
    wide = np.full((8, 8), 77, dtype=np.uint32)
    assert lib.STORM_dosage_square_dot(h, wider, wide.ctypes.data, 8, 8) == -3
    assert b"samples" in lib.STORM_hip_error()
    assert lib.STORM_dosage_square_dot_device(wider, h, wide.ctypes.data, 8, 8) == -3
    assert (wide == 77).all() and (big == 0).all()
    for d in (h, other, wider):
        lib.STORM_dosage_free(d)


def test_the_device_layer_refuses_null_arguments(lib):
    """storm_hip_* refusals that need no device: NULL context"""
    out = np.zeros(4, dtype=np.uint32)
    assert lib.storm_hip_square_dosage_matrix(None, None, None, out.ctypes.data, 4) == -1
    assert lib.storm_hip_square_dosage_matrix_device(None, None, None, out.ctypes.data, 4) == -1
    assert lib.storm_hip_dosage_row_missing(None, None, 4, out.ctypes.data) == -1
    assert lib.storm_hip_pairw_dosage_nobs(None, None, 4, out.ctypes.data, 4) == -1
    assert lib.storm_hip_pairw_dosage_nobs_device(None, None, 4, out.ctypes.data, 4) == -1
    assert lib.storm_hip_pairw_dosage_corr_complete(None, None, 0, 4, out.ctypes.data, 4) == -1
    assert lib.storm_hip_pairw_dosage_corr_complete_device(None, None, 0, 4, out.ctypes.data, 4) == -1
    assert b"NULL context" in lib.storm_hip_last_error()


def test_no_cpu_fallback_without_device(lib):
    if lib.storm_hip_device_count() != 0:
        pytest.skip("a GPU is visible; the loud-failure path is exercised on the CPU container")
    S, n = 100, 3
    h = lib.STORM_dosage_new(S)
    rng = np.random.default_rng(1)
    for _ in range(n):
        r = rng.integers(0, 4, size=S, dtype=np.uint8)
        assert lib.STORM_dosage_add(h, r.ctypes.data, S) == 0
    out = np.full((n, n), 77, dtype=np.uint32)
    fout = np.full((n, n), 7.0, dtype=np.float32)
    miss = np.full(n, 77, dtype=np.uint32)
    assert lib.STORM_dosage_square_dot(h, h, out.ctypes.data, n, n) == -3
    assert lib.STORM_hip_error()
    assert lib.STORM_dosage_pairw_nobs(h, out.ctypes.data, n, n) == -3
    assert lib.STORM_dosage_pairw_corr_complete(h, 0, fout.ctypes.data, n, n) == -3
    assert lib.STORM_dosage_pairw_corr_complete(h, 1, fout.ctypes.data, n, n) == -3
    assert lib.STORM_dosage_row_missing(h, miss.ctypes.data) == -3
    assert lib.STORM_hip_error()
    assert (out == 77).all() and (fout == 7.0).all() and (miss == 77).all()
    lib.STORM_dosage_free(h)
    d = sb.StormDosage(S)
    d.add(np.zeros(S, dtype=np.uint8))
    d.add(np.full(S, 3, dtype=np.uint8))
    for call in (lambda: d.square_dot(d), d.pairw_nobs, d.row_missing, lambda: d.pairw_corr_complete("r")):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(KeyError):
        d.pairw_corr_complete("pearson")
