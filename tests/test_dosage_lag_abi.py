"""The host side of the dosage container's lag calls (storm.h: STORM_dosage_pairw_lag_dot, _lag_corr, _lag_nobs,
_lag_corr_complete and their _device forms) without a GPU: the exports, every refusal code — those of STORM_pairw_lag_matrix
and of STORM_dosage_pairw_corr — empty shapes, and, no CPU fallback, compute calls that fail with a reason when no device
is visible. The interleaved split of the pairwise-complete call (storm_dosage_math.h: dosage_interleaved_word, the one line
dosage_split_interleaved_kernel runs per word) and the place of the six sums of an entry in the lag layout of the
interleaved rows (dosage_interleaved_entry_bits, the one line of dosage_complete_finish_lag_kernel) are built by a host
compiler here and compared with numpy. What the device computes is tests/test_gpu_dosage_lag.py's."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import stormbitmaps_amd as sb
from stormbitmaps_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DOT = ("STORM_dosage_pairw_lag_dot", "STORM_dosage_pairw_lag_dot_device", "STORM_dosage_pairw_lag_nobs",
       "STORM_dosage_pairw_lag_nobs_device")
CORR = ("STORM_dosage_pairw_lag_corr", "STORM_dosage_pairw_lag_corr_device", "STORM_dosage_pairw_lag_corr_complete",
        "STORM_dosage_pairw_lag_corr_complete_device")
SHIM = ("storm_hip_lag_dosage_plan", "storm_hip_pairw_lag_dosage_matrix", "storm_hip_pairw_lag_dosage_matrix_device",
        "storm_hip_dosage_finish_lag_device", "storm_hip_pairw_lag_dosage_corr", "storm_hip_pairw_lag_dosage_corr_device",
        "storm_hip_pairw_lag_dosage_nobs", "storm_hip_pairw_lag_dosage_nobs_device", "storm_hip_pairw_lag_dosage_corr_complete",
        "storm_hip_pairw_lag_dosage_corr_complete_device")


def test_the_library_exports_and_binds_the_calls(lib):
    for name in DOT + CORR + SHIM:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "stormbitmaps_amd", "libstorm_hip.so")],
                         capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(DOT + CORR + SHIM) <= exported
    assert not {s for s in exported if "interleave" in s or "_kernel" in s and not s.startswith("storm_hip_")}   # stay inside
    header = open(os.path.join(ROOT, "include", "storm.h")).read()
    for name in DOT + CORR:
        assert f"int {name}(" in header, name
    header = open(os.path.join(ROOT, "include", "storm_hip.h")).read()
    for name in SHIM:
        assert f"int {name}(" in header, name


def call(lib, name, h, max_lag, out, rows, ld, measure=0):
    f = getattr(lib, name)
    return f(h, measure, max_lag, out, rows, ld) if name in CORR else f(h, max_lag, out, rows, ld)


def test_every_refusal_code_and_the_empty_shapes(lib):
    S = 40
    h = lib.STORM_dosage_new(S)
    good = np.arange(S, dtype=np.uint8) % 4
    out = np.full((8, 8), 77, dtype=np.uint32)
    o = out.ctypes.data
    for name in DOT + CORR:
        assert call(lib, name, None, 1, o, 8, 8) == -1, name                      # NULL handle
        assert call(lib, name, h, 1, None, 8, 8) == -2, name                      # NULL out
        assert call(lib, name, h, 3, o, 0, 0) == 0, name                          # empty: 0, nothing written, no device
        assert call(lib, name, h, 0, o, 8, 8) == -3, name                         # max_lag 0, even when empty
        assert b"max_lag" in lib.STORM_hip_error()
    assert lib.STORM_dosage_add(h, good.ctypes.data, S) == 0
    for name in DOT + CORR:
        assert call(lib, name, h, 3, o, 1, 0) == 0, name                          # one row: L = 0, nothing written
        assert call(lib, name, h, 3, o, 0, 8) == -4, name                         # out_rows < n
    for _ in range(4):
        assert lib.STORM_dosage_add(h, good.ctypes.data, S) == 0
    assert lib.STORM_dosage_n_rows(h) == 5
    for name in DOT + CORR:
        assert call(lib, name, h, 3, o, 4, 8) == -4, name                         # out_rows < n
        assert call(lib, name, h, 3, o, 8, 2) == -4, name                         # out_ld < L = 3
        assert call(lib, name, h, 100, o, 8, 3) == -4, name                       # out_ld < L = n - 1 = 4
        assert call(lib, name, h, 0, o, 4, 0) == -3, name                         # max_lag 0 is said before the sizes
    for name in CORR:
        for measure in (2, -1, 99):                                               # before any device is asked for
            assert call(lib, name, h, 3, o, 8, 8, measure=measure) == -3, name
            assert b"measure" in lib.STORM_hip_error()
    assert (out == 77).all()
    lib.STORM_dosage_free(h)


def test_the_device_layer_refuses_null_arguments(lib):
    out = np.zeros(4, dtype=np.uint32)
    o = out.ctypes.data
    assert lib.storm_hip_pairw_lag_dosage_matrix(None, None, 1, o, 4) == -1
    assert lib.storm_hip_pairw_lag_dosage_matrix_device(None, None, 1, 0, 4, o, 4) == -1
    assert lib.storm_hip_dosage_finish_lag_device(None, o, 4, 4, 0, 4, 1, o, o, 0, 4) == -1
    assert lib.storm_hip_pairw_lag_dosage_corr(None, None, 0, 4, 1, o, 4) == -1
    assert lib.storm_hip_pairw_lag_dosage_corr_device(None, None, 0, 4, 1, o, 4) == -1
    assert lib.storm_hip_pairw_lag_dosage_nobs(None, None, 4, 1, o, 4) == -1
    assert lib.storm_hip_pairw_lag_dosage_nobs_device(None, None, 4, 1, o, 4) == -1
    assert lib.storm_hip_pairw_lag_dosage_corr_complete(None, None, 0, 4, 1, o, 4) == -1
    assert lib.storm_hip_pairw_lag_dosage_corr_complete_device(None, None, 0, 4, 1, o, 4) == -1
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
    for name in DOT + CORR:
        assert call(lib, name, h, 2, out.ctypes.data, n, n) == -3, name
        assert lib.STORM_hip_error()
    assert (out == 77).all()
    lib.STORM_dosage_free(h)
    d = sb.StormDosage(S)
    d.add(np.zeros(S, dtype=np.uint8))
    d.add(np.full(S, 3, dtype=np.uint8))
    for f in (lambda: d.pairw_lag_dot(1), lambda: d.pairw_lag_corr(1, "r"), lambda: d.pairw_lag_nobs(1),
              lambda: d.pairw_lag_corr_complete(1)):
        with pytest.raises(RuntimeError):
            f()
    with pytest.raises(KeyError):
        d.pairw_lag_corr_complete(1, "pearson")


# ------------------------------------------------------------------------------------------ the interleaved split
SOURCE = r"""
#include "storm_dosage_math.h"
extern "C" void interleave(const uint64_t* x, uint64_t stride_words, uint64_t n_rows, uint32_t n_words, uint64_t n_samples,
                           uint64_t rows_out, uint64_t* t) {
    for (uint64_t r = 0; r < rows_out; ++r)
        for (uint64_t w = 0; w < stride_words; ++w)
            t[r * stride_words + w] = storm::dosage_interleaved_word(x, stride_words, n_rows, n_words, n_samples, r, w);
}
extern "C" void entries(const uint32_t* sums, uint64_t lds, uint64_t n, uint64_t lag, int measure, uint32_t* out) {
    for (uint64_t i = 0; i < n; ++i)
        for (uint64_t d = 0; d < lag && i + 1 + d < n; ++d)
            out[i * lag + d] = storm::dosage_interleaved_entry_bits(sums + 3 * i * lds, sums + (3 * i + 1) * lds,
                                                                    sums + (3 * i + 2) * lds, (uint32_t)d, measure);
}
extern "C" uint32_t complete_bits(uint32_t P, uint32_t N, uint32_t sx, uint32_t sy, uint32_t qx, uint32_t qy, int measure) {
    return storm::dosage_corr_complete_bits(P, N, sx, sy, qx, qy, measure);
}
"""


@pytest.fixture(scope="module")
def math(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "a host C++ compiler"
    d = tmp_path_factory.mktemp("dosagelag")
    src, so = d / "lag.cpp", d / "liblag.so"
    src.write_text(SOURCE)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "stormbitmaps_amd", "csrc"), str(src), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    lib.interleave.restype = lib.entries.restype = None
    lib.interleave.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_void_p]
    lib.entries.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p]
    lib.complete_bits.restype = C.c_uint32
    lib.complete_bits.argtypes = [C.c_uint32] * 6 + [C.c_int]
    return lib


def pack(G, stride_words):
    """[n, S] values 0 .. 3 -> [n, stride_words] uint64, 32 values per word; the words behind ceil(S / 32) hold ones (a
    device matrix's pad is zero, but the split must not depend on it)"""
    n, S = G.shape
    n_words = (S + 31) // 32
    v = np.zeros((n, n_words * 32), dtype=np.uint64)
    v[:, :S] = G
    words = (v.reshape(n, -1, 32) << (np.arange(32, dtype=np.uint64) * np.uint64(2))).sum(axis=2, dtype=np.uint64)
    out = np.full((n, stride_words), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    out[:, :n_words] = words
    return out


def unpack(words, S):
    """[rows, stride] uint64 -> [rows, S] values"""
    v = (words[:, :, None] >> (np.arange(32, dtype=np.uint64) * np.uint64(2))[None, None, :]) & np.uint64(3)
    return v.reshape(words.shape[0], -1)[:, :S].astype(np.int64)


@pytest.mark.parametrize("n,S,stride", [(1, 1, 1), (5, 31, 2), (43, 33, 8), (7, 64, 2), (130, 257, 16)])
def test_interleaved_split_against_a_numpy_restatement_of_the_word_split(math, n, S, stride):
    """row 3 i = G_i (3 -> 0), 3 i + 1 = H_i (1 where 2), 3 i + 2 = M_i (1 where present); zero rows behind 3 n up to a
    multiple of 128 and two more; zero in every word behind ceil(S / 32) and at the tail samples of the last word"""
    rng = np.random.default_rng(100 * n + S)
    X = rng.integers(0, 4, size=(n, S), dtype=np.uint8)
    X[0, :] = 3
    words = pack(X, stride)
    rows_out = (3 * n + 127) // 128 * 128 + 2
    t = np.full((rows_out, stride), 0x1111111111111111, dtype=np.uint64)
    math.interleave(words.ctypes.data, stride, n, (S + 31) // 32, S, rows_out, t.ctypes.data)
    n_words = (S + 31) // 32
    assert (t[:, n_words:] == 0).all() and (t[3 * n:] == 0).all()
    got = unpack(t[:3 * n], n_words * 32)
    assert (got[:, S:] == 0).all()                                                 # the tail samples, M's too
    x = X.astype(np.int64)
    assert np.array_equal(got[0::3, :S], np.where(x == 3, 0, x))
    assert np.array_equal(got[1::3, :S], (x == 2).astype(np.int64))
    assert np.array_equal(got[2::3, :S], (x != 3).astype(np.int64))


@pytest.mark.parametrize("n,L", [(9, 1), (20, 7), (20, 19), (50, 42)])
def test_an_entry_is_made_of_the_six_sums_at_their_skewed_columns(math, n, L):
    """the lag layout (lag 3 L + 2) of the products of the interleaved rows, from numpy; entry (i, d) read out of it equals
    dosage_corr_complete_bits on the six sums of the pair (i, i + 1 + d) computed from the rows themselves"""
    S = 60
    rng = np.random.default_rng(n * 100 + L)
    X = rng.integers(0, 4, size=(n, S), dtype=np.uint8)
    x = X.astype(np.int64)
    g, h, m = np.where(x == 3, 0, x), (x == 2).astype(np.int64), (x != 3).astype(np.int64)
    t = np.empty((3 * n, S), dtype=np.int64)
    t[0::3], t[1::3], t[2::3] = g, h, m
    full = t @ t.T
    lag3 = 3 * L + 2
    lds = (lag3 + 3) // 4 * 4
    sums = np.full((3 * n, lds), 0xDEADBEEF, dtype=np.uint32)                      # the corner and the pitch: never used
    for r in range(3 * n):
        for c in range(r + 1, min(3 * n, r + lag3 + 1)):
            sums[r, c - r - 1] = full[r, c]
    for measure in (0, 1):
        out = np.full((n, L), 0xDEADBEEF, dtype=np.uint32)
        math.entries(sums.ctypes.data, lds, n, L, measure, out.ctypes.data)
        for i in range(n):
            for d in range(L):
                j = i + 1 + d
                if j >= n:
                    assert out[i, d] == 0xDEADBEEF
                    continue
                N, P, sx, sy = m[i] @ m[j], g[i] @ g[j], g[i] @ m[j], m[i] @ g[j]
                qx, qy = (g[i] * g[i]) @ m[j], m[i] @ (g[j] * g[j])
                assert out[i, d] == math.complete_bits(int(P), int(N), int(sx), int(sy), int(qx), int(qy), measure), (i, d)
