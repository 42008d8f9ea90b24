"""The host side of the dosage containers' top-k calls (storm.h: STORM_dosage_pairw_topk, STORM_dosage_square_topk, their
_complete and _device forms) without a GPU: the eight symbols and their storm_hip_* counterparts are exported and declared,
and every refusal that needs no device returns its code — those of STORM_dosage_square_corr and STORM_square_topk — with the
sentinel-filled outputs untouched. No CPU fallback: with rows and no device visible the calls fail with a reason. What the
device selects is tests/test_gpu_dosage_topk.py's."""
import os

import numpy as np
import pytest

import stormbitmaps_amd as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0xDEADBEEF
R2, R, DOT = 0, 1, 2
TOPK_MAX = 128
FORMS = [(shape, complete, device) for shape in ("pairw", "square") for complete in ("", "_complete") for device in ("", "_device")]


def _name(shape, complete, device):
    return f"STORM_dosage_{shape}_topk{complete}{device}"


def _calls(lib):
    """every one of the eight as (name, complete, f(a, b, score, k, panel_rows, idx, val, out_rows, out_ld)); the pairw forms
    take `a` alone"""
    out = []
    for shape, complete, device in FORMS:
        fn = getattr(lib, _name(shape, complete, device))
        if shape == "pairw":
            out.append((_name(shape, complete, device), bool(complete), False, lambda a, b, *rest, fn=fn: fn(a, *rest)))
        else:
            out.append((_name(shape, complete, device), bool(complete), True, lambda a, b, *rest, fn=fn: fn(a, b, *rest)))
    return out


def test_the_symbols_are_exported_and_declared(lib):
    header = open(os.path.join(ROOT, "include", "storm.h")).read()
    device_header = open(os.path.join(ROOT, "include", "storm_hip.h")).read()
    assert "#define STORM_DOSAGE_TOPK_DOT 2" in header and "#define STORM_HIP_DOSAGE_TOPK_DOT 2" in device_header
    for shape, complete, device in FORMS:
        name = _name(shape, complete, device)
        handles = "STORM_dosage_t* h," if shape == "pairw" else "STORM_dosage_t* a, STORM_dosage_t* b,"
        assert hasattr(lib, name), name
        assert f"int {name}({handles} int score, uint64_t k, uint64_t panel_rows," in header, name
        hip = f"storm_hip_{shape}_dosage_topk{complete}{device}"
        handles = "const storm_hip_matrix_t* m," if shape == "pairw" else "const storm_hip_matrix_t* a, const storm_hip_matrix_t* b,"
        assert hasattr(lib, hip), hip
        assert f"int {hip}(storm_hip_ctx_t* ctx, {handles}" in " ".join(device_header.split()), hip
    assert hasattr(lib, "storm_hip_dosage_topk_rows_device")
    assert "int storm_hip_dosage_topk_rows_device(storm_hip_ctx_t* ctx, const uint32_t* d_dots," in device_header


def test_every_refusal_code(lib):
    S, n, k = 40, 5, 4
    a, b, wider, empty = (lib.STORM_dosage_new(S), lib.STORM_dosage_new(S), lib.STORM_dosage_new(S + 1), lib.STORM_dosage_new(S))
    good = (np.arange(S, dtype=np.uint8) % 4)
    for _ in range(n):
        assert lib.STORM_dosage_add(a, good.ctypes.data, S) == 0
    for _ in range(6):
        assert lib.STORM_dosage_add(b, good.ctypes.data, S) == 0
    assert lib.STORM_dosage_add(wider, np.zeros(S + 1, dtype=np.uint8).ctypes.data, S + 1) == 0
    idx = np.full((8, 8), SENTINEL, dtype=np.uint32)
    val = np.full((8, 8), SENTINEL, dtype=np.uint32)
    p, q = idx.ctypes.data, val.ctypes.data
    for name, complete, square, call in _calls(lib):
        # NULL handles: -1; NULL idx or val: -2
        assert call(None, b, R2, k, 0, p, q, 8, 8) == -1, name
        if square:
            assert call(a, None, R2, k, 0, p, q, 8, 8) == -1, name
        assert call(None, None, R2, k, 0, None, None, 8, 8) == -1, name
        assert call(a, b, R2, k, 0, None, q, 8, 8) == -2 and call(a, b, R2, k, 0, p, None, 8, 8) == -2, name
        # too small an output: -4, ahead of every -3
        assert call(a, b, R2, k, 0, p, q, n - 1, 8) == -4 and call(a, b, R2, k, 0, p, q, 8, k - 1) == -4, name
        assert call(a, b, 7, k, 100, p, q, n - 1, 8) == -4, name
        # a bad score: -3, the dot product in the _complete forms included
        for score in (3, -1, 99) + ((DOT,) if complete else ()):
            assert call(a, b, score, k, 0, p, q, 8, 8) == -3, (name, score)
            msg = lib.STORM_hip_error()
            assert b"score" in msg and name.encode() in msg, (name, msg)
        # k of 0 and above the maximum; panel_rows that is no multiple of 256
        assert call(a, b, R2, 0, 0, p, q, 8, 8) == -3 and b"k must be" in lib.STORM_hip_error(), name
        big = np.full((8, TOPK_MAX + 1), SENTINEL, dtype=np.uint32)
        assert call(a, b, R2, TOPK_MAX + 1, 0, big.ctypes.data, big.ctypes.data, 8, TOPK_MAX + 1) == -3, name
        assert b"k must be" in lib.STORM_hip_error() and (big == SENTINEL).all(), name
        for panel_rows in (100, 255, 257):
            assert call(a, b, R2, k, panel_rows, p, q, 8, 8) == -3 and b"panel_rows" in lib.STORM_hip_error(), (name, panel_rows)
        # unequal sample counts: -3, the message names both counts
        if square:
            for x, y in ((a, wider), (wider, a)):
                assert call(x, y, R2, 1, 0, p, q, 8, 8) == -3, name
                msg = lib.STORM_hip_error()
                assert b"samples" in msg and str(S).encode() in msg and str(S + 1).encode() in msg and name.encode() in msg, (name, msg)
        # an empty a: 0, nothing written (no device is needed); its arguments are checked all the same
        assert call(empty, b, R2, k, 0, p, q, 0, k) == 0 and call(empty, empty, R if complete else DOT, TOPK_MAX, 256, p, q, 0, 128) == 0, name
        assert call(empty, b, R2, 0, 0, p, q, 0, 8) == -3 and call(empty, b, R2, k, 0, p, q, 0, k - 1) == -4, name
    assert (idx == SENTINEL).all() and (val == SENTINEL).all()
    for d in (a, b, wider, empty):
        lib.STORM_dosage_free(d)


def test_the_device_layer_refuses_a_null_context(lib):
    out = np.zeros(4, dtype=np.uint32)
    o = out.ctypes.data
    for complete in ("", "_complete"):
        for device in ("", "_device"):
            assert getattr(lib, f"storm_hip_pairw_dosage_topk{complete}{device}")(None, None, 0, 4, 1, 0, o, o, 1) == -1
            assert getattr(lib, f"storm_hip_square_dosage_topk{complete}{device}")(None, None, None, 0, 4, 1, 0, o, o, 1) == -1
            assert b"NULL context" in lib.storm_hip_last_error()
    assert lib.storm_hip_dosage_topk_rows_device(None, o, 1, 1, 1, o, o, o, o, 4, 0, 0, 1, o, o, 1) == -1
    assert b"NULL context" in lib.storm_hip_last_error()


def test_python_methods_check_their_arguments():
    S = 12
    d, other = sb.StormDosage(S), sb.StormDosage(S)
    idx, val = d.pairw_topk(3)
    assert idx.shape == val.shape == (0, 3) and idx.dtype == np.uint32 and val.dtype == np.float32
    assert d.square_topk(other, 2, "dot")[1].dtype == np.uint32 and d.square_topk(other, 2, "r", complete=True)[0].shape == (0, 2)
    with pytest.raises(KeyError):
        d.pairw_topk(3, "pearson")
    with pytest.raises(RuntimeError, match="score"):
        d.pairw_topk(3, "dot", complete=True)
    with pytest.raises(RuntimeError, match="k must be"):
        d.pairw_topk(0)
    with pytest.raises(RuntimeError, match="panel_rows"):
        d.square_topk(other, 3, panel_rows=100)
    with pytest.raises(RuntimeError, match="samples"):
        d.square_topk(sb.StormDosage(S + 1), 3)
    d.free()
    other.free()


def test_no_cpu_fallback_without_device(lib):
    if lib.storm_hip_device_count() != 0:
        pytest.skip("a GPU is visible; the loud-failure path is exercised on the CPU container")
    S, n, k = 100, 3, 2
    h = lib.STORM_dosage_new(S)
    rng = np.random.default_rng(1)
    for _ in range(n):
        r = rng.integers(0, 4, size=S, dtype=np.uint8)
        assert lib.STORM_dosage_add(h, r.ctypes.data, S) == 0
    idx = np.full((n, k), SENTINEL, dtype=np.uint32)
    val = np.full((n, k), SENTINEL, dtype=np.uint32)
    for name, complete, square, call in _calls(lib):
        assert call(h, h, R2, k, 0, idx.ctypes.data, val.ctypes.data, n, k) == -3, name
        assert lib.STORM_hip_error(), name
    assert (idx == SENTINEL).all() and (val == SENTINEL).all()
    lib.STORM_dosage_free(h)
