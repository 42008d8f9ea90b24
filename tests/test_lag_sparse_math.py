"""storm_lag_sparse_math.h — the pitch of a row's forward mask, the slot of a set bit in the list and the block plan of the scan
of lag_band_sparse_*_kernel — built by the host C++ compiler and compared with numpy at the word and block boundaries; and the
numpy reference of the GPU tests (tests/_lag_sparse.py) against the adjacency of the pruning tests (tests/_prune.py). No
device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _lag_sparse, _prune

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SOURCE = r"""
#include "storm_lag_sparse_math.h"
extern "C" uint64_t mask_pitch(uint64_t L) { return storm::sparse_mask_pitch(L); }
extern "C" uint32_t bits_below(uint64_t word, uint32_t lane) { return storm::sparse_bits_below(word, lane); }
extern "C" uint64_t slot(uint64_t row_start, uint64_t before, uint64_t word, uint32_t lane) {
    return storm::sparse_slot(row_start, before, word, lane);
}
extern "C" uint64_t scan_rows(void) { return storm::kSparseScanRows; }
extern "C" uint64_t scan_blocks(uint64_t n) { return storm::sparse_scan_blocks(n); }
extern "C" uint64_t scan_block_of(uint64_t row) { return storm::sparse_scan_block_of(row); }
extern "C" uint64_t scan_block_rows(uint64_t n, uint64_t b) { return storm::sparse_scan_block_rows(n, b); }
extern "C" uint64_t scratch_words(uint64_t n, uint64_t L, int windows) { return storm::sparse_scratch_words(n, L, windows != 0); }
extern "C" int edge(float rho, float min_r2) { return storm::prune_edge(rho, min_r2) ? 1 : 0; }
"""

LAGS = (1, 31, 32, 33, 63, 64, 65, 129, 4096)


@pytest.fixture(scope="module")
def math(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "a host C++ compiler"
    d = tmp_path_factory.mktemp("lag_sparse")
    src, so = d / "lag_sparse.cpp", d / "liblag_sparse.so"
    src.write_text(SOURCE)
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "stormbitmaps_amd", "csrc"), str(src), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    u64, u32 = C.c_uint64, C.c_uint32
    for name, res, args in (("mask_pitch", u64, [u64]), ("bits_below", u32, [u64, u32]), ("slot", u64, [u64, u64, u64, u32]),
                            ("scan_rows", u64, []), ("scan_blocks", u64, [u64]), ("scan_block_of", u64, [u64]),
                            ("scan_block_rows", u64, [u64, u64]), ("scratch_words", u64, [u64, u64, C.c_int]),
                            ("edge", C.c_int, [C.c_float, C.c_float])):
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    return lib


def test_the_mask_pitch_covers_every_lag_in_whole_words(math):
    for L in LAGS + (2, 127, 128, 4095, 4097, (1 << 32) - 1):
        pitch = math.mask_pitch(L)
        assert pitch == -(-L // 64)
        assert 64 * (pitch - 1) < L <= 64 * pitch                                  # the last lag has a bit, no word is spare


def test_the_slot_of_a_bit_is_its_rank_in_the_row(math):
    """a row's mask of L random bits, word by word as the fill kernel walks it: the slots of the set bits are row_start,
    row_start + 1, .. in ascending lag order, exactly numpy's flatnonzero"""
    rng = np.random.default_rng(11)
    for L in LAGS:
        for density in (0.0, 0.03, 0.5, 1.0):
            bits = rng.random(L) < density
            words = np.zeros(math.mask_pitch(L), dtype=np.uint64)
            for d in np.flatnonzero(bits):
                words[d // 64] |= np.uint64(1) << np.uint64(d % 64)
            row_start = int(rng.integers(0, 1 << 40))
            before, got = 0, []
            for c, word in enumerate(words.tolist()):
                for lane in range(64):
                    assert math.bits_below(word, lane) == bin(word & ((1 << lane) - 1)).count("1")
                    if (word >> lane) & 1:
                        got.append((64 * c + lane, math.slot(row_start, before, word, lane)))
                before += bin(word).count("1")
            want = np.flatnonzero(bits)
            assert [d for d, _ in got] == want.tolist()
            assert [s for _, s in got] == list(range(row_start, row_start + want.size))
            assert before == int(bits.sum())
    assert math.bits_below((1 << 64) - 1, 63) == 63 and math.bits_below((1 << 64) - 1, 0) == 0
    assert math.slot((1 << 33) + 5, (1 << 32) + 1, 1 << 63, 63) == (1 << 33) + (1 << 32) + 6   # 64-bit offsets


def test_the_scan_blocks_partition_the_rows(math):
    R = math.scan_rows()
    assert R == 1024
    for n in (0, 1, 2, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 1, 70001, (1 << 20) + 3):
        blocks = math.scan_blocks(n)
        assert blocks == -(-n // R)
        rows = [math.scan_block_rows(n, b) for b in range(blocks + 2)]
        assert sum(rows) == n and rows[blocks:] == [0, 0]
        assert all(r == R for r in rows[:max(blocks - 1, 0)]) and (blocks == 0 or 1 <= rows[blocks - 1] <= R)
        for row in {0, n // 2, max(n - 1, 0)} if n else ():
            b = math.scan_block_of(row)
            assert b * R <= row < b * R + math.scan_block_rows(n, b)
    # the offsets the three launches produce, replayed with numpy at the block size +- 1: sums per block, their exclusive
    # scan, every block's own scan behind its sum
    rng = np.random.default_rng(5)
    for n in (R - 1, R, R + 1, 2 * R + 1):
        counts = rng.integers(0, 3, size=n).astype(np.uint32)
        blocks = math.scan_blocks(n)
        sums = np.array([counts[b * R:b * R + math.scan_block_rows(n, b)].sum() for b in range(blocks)], dtype=np.uint64)
        base = np.concatenate([[0], np.cumsum(sums)[:-1]]).astype(np.uint64)
        offsets = np.concatenate([base[b] + np.concatenate([[0], np.cumsum(counts[b * R:(b + 1) * R])[:-1]]).astype(np.uint64)
                                  for b in range(blocks)])
        assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64))


def test_the_scratch_keeps_its_64_bit_part_first(math):
    for n in (2, 63, 1025, 70001):
        for L in LAGS:
            for windows in (0, 1):
                words = math.scratch_words(n, L, windows)
                assert words == 2 * (n * math.mask_pitch(L) + math.scan_blocks(n)) + n + (2 * n if windows else 0)


def test_the_predicate_is_prunings(math):
    f32 = np.float32
    t = f32(0.5)
    assert math.edge(t, t) == 0 and math.edge(np.nextafter(t, f32(1)), t) == 1 and math.edge(f32(np.nan), t) == 0
    assert math.edge(f32(0.0), f32(-0.0)) == 0 and math.edge(f32(-0.0), f32(0.0)) == 0 and math.edge(f32(np.inf), t) == 1
    assert math.edge(f32(0.0), f32(-1.0)) == 1 and math.edge(f32(np.nan), f32(-1.0)) == 0


@pytest.mark.parametrize("n,max_lag", [(2, 1), (33, 31), (64, 64), (65, 200), (130, 63)])
def test_the_numpy_reference_symmetrised_is_the_pruning_tests_adjacency(n, max_lag):
    rng = np.random.default_rng(100 * n + max_lag)
    L = min(max_lag, n - 1)
    t = np.float32(0.5)
    band = rng.choice(np.float32([0.1, 0.9, t, np.nan, np.nextafter(t, np.float32(1)), np.inf, 0.0]), size=(n, L + 2))
    pos = np.cumsum(rng.integers(1, 5, size=n)).astype(np.float64)
    lo, hi, _ = _prune.window_bounds(pos, 9.0)
    one_sided = (np.zeros(n, np.uint32), hi)                                       # windows narrower than the lag ahead only
    for windows in ((None, None), (lo, hi), one_sided):
        row_start, col, val = _lag_sparse.sparse_list(band, n, max_lag, t, *windows)
        assert row_start.dtype == np.uint64 and col.dtype == np.uint32 and val.dtype == np.float32
        assert row_start[0] == 0 and row_start[n] == col.size == val.size
        nb = _prune.neighbours(band, n, max_lag, t, *windows)
        assert _lag_sparse.symmetrised(row_start, col, n) == [sorted(x) for x in nb]
        for i in range(n):
            mine = col[int(row_start[i]):int(row_start[i + 1])]
            assert (np.diff(mine.astype(np.int64)) > 0).all() and (mine > i).all() and (mine < n).all()
            assert np.array_equal(val[int(row_start[i]):int(row_start[i + 1])].view(np.uint32),
                                  band[i, mine.astype(np.int64) - i - 1].view(np.uint32))
    assert _lag_sparse.sparse_list(band, n, max_lag, np.float32(-1.0))[0][n] == int(
        np.isfinite(band[:, :L])[np.arange(n)[:, None] + 1 + np.arange(L)[None, :] < n].sum()
        + np.isinf(band[:, :L])[np.arange(n)[:, None] + 1 + np.arange(L)[None, :] < n].sum())   # every pair that is a number
