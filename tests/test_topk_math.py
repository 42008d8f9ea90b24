"""The order of topk_rows_kernel without a device: storm_topk_math.h holds the key the kernel ranks by, and a host
compiler builds the same lines here. The candidate predicate is false exactly for the one NaN pattern the similarity
measures write; sorting 10^5 random (value bits, column) pairs by key, descending, equals numpy's order by value
descending, then column ascending — for floats (negatives, denormals, +-0, +-inf, many repeated values) and for counts —
and a key gives its column and its value back. What a device adds to this, the sweep, the selection and the calls
around the kernel, is tests/test_gpu_topk.py's."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_BITS = 0x7FC00000
N = 100_000

SOURCE = r"""
#include "storm_topk_math.h"
extern "C" void topk_keys(const uint32_t* bits, const uint32_t* j, uint64_t n, int is_count, uint64_t* keys) {
    for (uint64_t i = 0; i < n; ++i) keys[i] = storm::topk_key(bits[i], j[i], is_count != 0);
}
extern "C" void topk_unkey(const uint64_t* keys, uint64_t n, int is_count, uint32_t* bits, uint32_t* j) {
    for (uint64_t i = 0; i < n; ++i) {
        bits[i] = storm::topk_key_value(keys[i], is_count != 0);
        j[i] = storm::topk_key_index(keys[i]);
    }
}
extern "C" void topk_candidates(const uint32_t* bits, uint64_t n, uint8_t* out) {
    for (uint64_t i = 0; i < n; ++i) out[i] = storm::topk_is_candidate(bits[i]) ? 1 : 0;
}
extern "C" uint32_t topk_nan(void) { return storm::kTopkNaN; }
extern "C" uint32_t topk_no_index(void) { return storm::kTopkNoIndex; }
"""


@pytest.fixture(scope="module")
def math(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "a host C++ compiler"
    d = tmp_path_factory.mktemp("topkmath")
    src, so = d / "topk.cpp", d / "libtopk.so"
    src.write_text(SOURCE)
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "stormbitmaps_amd", "csrc"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    for f in (lib.topk_keys, lib.topk_unkey, lib.topk_candidates):
        f.restype = None
    lib.topk_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    lib.topk_unkey.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p]
    lib.topk_candidates.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    lib.topk_nan.restype = lib.topk_no_index.restype = C.c_uint32
    return lib


def _keys(lib, bits, j, is_count):
    bits, j = np.ascontiguousarray(bits, dtype=np.uint32), np.ascontiguousarray(j, dtype=np.uint32)
    keys = np.empty(bits.size, dtype=np.uint64)
    lib.topk_keys(bits.ctypes.data, j.ctypes.data, bits.size, int(is_count), keys.ctypes.data)
    return keys


def _unkey(lib, keys, is_count):
    bits, j = np.empty(keys.size, dtype=np.uint32), np.empty(keys.size, dtype=np.uint32)
    lib.topk_unkey(keys.ctypes.data, keys.size, int(is_count), bits.ctypes.data, j.ctypes.data)
    return bits, j


def _columns(rng, n):
    """distinct columns, the ends of the range among them (the largest column is 2^32 - 2: 2^32 - 1 marks a padding)"""
    j = rng.choice(1 << 20, size=n, replace=False).astype(np.uint32)
    j[:4] = (0, 1, (1 << 32) - 2, (1 << 32) - 3)
    return j


def test_candidate_predicate_is_false_exactly_for_the_nan_pattern(math):
    assert math.topk_nan() == NAN_BITS and math.topk_no_index() == 0xFFFFFFFF
    rng = np.random.default_rng(7)
    bits = np.concatenate([rng.integers(0, 1 << 32, size=N, dtype=np.uint64).astype(np.uint32),
                           # the pattern, its neighbours, the other NaNs and special values
                           np.array([NAN_BITS, NAN_BITS - 1, NAN_BITS + 1, 0xFFC00000, 0x7FC00001, 0x7F800001, 0x7FFFFFFF,
                                     0xFFFFFFFF, 0x7F800000, 0xFF800000, 0, 0x80000000, 1], dtype=np.uint32)])
    out = np.empty(bits.size, dtype=np.uint8)
    math.topk_candidates(bits.ctypes.data, bits.size, out.ctypes.data)
    assert np.array_equal(out.astype(bool), bits != NAN_BITS)
    assert not out[N] and out[N + 1:].all()


def test_float_keys_sort_like_value_descending_then_column_ascending(math):
    rng = np.random.default_rng(11)
    pool = np.concatenate([
        rng.standard_normal(300).astype(np.float32),                                       # negatives and positives
        (rng.random(200) * 1e-40).astype(np.float32) * rng.choice([-1, 1], 200).astype(np.float32),   # denormals
        np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 0.5, 1e-45, -1e-45, 3.4e38, -3.4e38], dtype=np.float32)])
    assert (np.abs(pool[300:500]) < np.finfo(np.float32).tiny).all() and (pool[300:500] != 0).any()
    values = pool[rng.integers(0, pool.size, size=N)]        # 10^5 draws of 511 values: many repeats
    values[:11] = pool[-11:]
    bits, j = values.view(np.uint32), _columns(rng, N)
    assert (bits == 0x80000000).any() and (bits == 0).any() and not np.isnan(values).any()
    keys = _keys(math, bits, j, False)
    assert np.unique(keys).size == N and (keys != 0).all()
    got = np.argsort(keys, kind="stable")[::-1]
    want = np.lexsort((j, -values.astype(np.float64)))      # value descending (-0 == +0), then column ascending
    assert np.array_equal(got, want)
    back_bits, back_j = _unkey(math, keys, False)
    assert np.array_equal(back_j, j)
    assert np.array_equal(back_bits, np.where(bits == 0x80000000, 0, bits))      # -0 comes back as +0, all else as it was


def test_count_keys_sort_like_count_descending_then_column_ascending(math):
    rng = np.random.default_rng(13)
    counts = rng.integers(0, 400, size=N, dtype=np.uint64).astype(np.uint32)     # many repeats
    counts[:6] = (0, 1, (1 << 32) - 1, (1 << 31), (1 << 31) - 1, NAN_BITS)           # a count is never "undefined"
    j = _columns(rng, N)
    keys = _keys(math, counts, j, True)
    assert np.unique(keys).size == N and (keys != 0).all()
    got = np.argsort(keys, kind="stable")[::-1]
    want = np.lexsort((j, -counts.astype(np.int64)))
    assert np.array_equal(got, want)
    back_counts, back_j = _unkey(math, keys, True)
    assert np.array_equal(back_j, j) and np.array_equal(back_counts, counts)
