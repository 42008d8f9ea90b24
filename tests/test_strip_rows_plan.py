"""The third strip form (strip_plan form 2: K2b with 128 A rows per wave, strip16_rows_kernel — A tiles of 512 rows = 8 own
64-row blocks, k-slices of 128 bits) on the host: its lists cover every (row pair, slice) exactly once over the ranks of a
world, and evaluated with numpy by the kernel's diagonal rule they add up to the oracle's total. The option that selects
the form is validated. No device is touched."""
import ctypes as C
import functools

import numpy as np
import pytest

from stormbitmaps_amd import _lib, dist

ROWS = (2, 513, 1100, 1600)
WORDS = (1, 3, 130)
SHAPINGS = ({}, {"max_run": 3, "tail_run": 2})


@functools.lru_cache(maxsize=None)
def _matrix(rows, words):
    rng = np.random.default_rng(rows * 131 + words)
    mat = rng.integers(0, 1 << 63, size=(rows, words), dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, size=(rows, words), dtype=np.uint64)
    mat[rows // 2] = 0
    mat.setflags(write=False)
    return mat


@functools.lru_cache(maxsize=None)
def _want(rows, words):
    from tests._orc import Oracle
    return Oracle().wrapper_diag_blocked(_matrix(rows, words), 31)


def _bits(cols):
    """[rows, 2] words -> [rows, 128] of 0 / 1 as float32 (a pair's count in a slice is at most 128: exact; the sums are taken in float64)."""
    return np.unpackbits(np.ascontiguousarray(cols).view(np.uint8), axis=1).astype(np.float32)


def _evaluate(items, mat):
    """The total of a list by the kernel's rule. Wave w of an item keeps blocks w and w + 4 of the 512-row A tile; at own-tile
    stage d a half (block b) skips d < b, keeps the strict upper triangle (A row < B row) at d == b and takes d > b whole;
    behind them the B blocks [j0, j1) whole. Rows beyond the matrix are zero, as is the second word of an odd row's last slice."""
    rows, words = mat.shape
    blocks = (rows + 63) // 64
    pad = np.zeros((max(blocks * 64, (rows + 511) // 512 * 512) + 512, words + (words & 1)), dtype=np.uint64)
    pad[:rows, :words] = mat
    upper = np.triu(np.ones((64, 64), dtype=np.float32), k=1)
    by_slice = {}
    total = 0
    for a_row0, diag, j0, j1, ks in items.tolist():
        if ks not in by_slice:
            by_slice[ks] = _bits(dist.slice_columns(pad, ks, 2))
        x = by_slice[ks]
        a = x[a_row0:a_row0 + 512]
        if j1 > j0:
            total += int((a @ x[64 * j0:64 * j1].T).sum(dtype=np.float64))
        if diag:
            for wave in range(4):
                for b in (wave, wave + 4):
                    ab = a[64 * b:64 * b + 64]
                    for d in range(8):
                        if d < b:
                            continue
                        c = ab @ a[64 * d:64 * d + 64].T
                        total += int((c * upper).sum(dtype=np.float64)) if d == b else int(c.sum(dtype=np.float64))
    return total


def _cover(items, blocks, n_slices, cover):
    """+1 for every (slice, A block, B block) an item multiplies; blocks beyond the matrix hold zero rows and are not counted."""
    for a_row0, diag, j0, j1, ks in items.tolist():
        assert a_row0 % 512 == 0 and ks < n_slices and j1 - j0 <= 4096
        a0 = a_row0 // 64
        assert j0 >= a0 + 8 or j1 == j0
        for b in range(a0, min(a0 + 8, blocks)):
            cover[ks, b, j0:min(j1, blocks)] += 1
            if diag:
                cover[ks, b, b:min(a0 + 8, blocks)] += 1
        assert j1 <= blocks or j1 == j0


@pytest.mark.parametrize("rows", ROWS)
def test_form2_covers_every_pair_and_slice_once_and_adds_up_to_the_oracle(rows):
    blocks = (rows + 63) // 64
    expect = np.triu(np.ones((blocks, blocks), dtype=np.int32))
    for words in WORDS:
        mat = _matrix(rows, words)
        n_slices = (words + 1) // 2
        for shaping in SHAPINGS:
            for world in (1, 2, 3):
                for pair_space in (0, 1):
                    cover = np.zeros((n_slices, blocks, blocks), dtype=np.int32)
                    total = 0
                    runs = set()
                    for rank in range(world):
                        items, run = dist.strip_plan(rows, words, rank, world, 2, pair_space, return_run=True, **shaping)
                        runs.add(run)
                        _cover(items, blocks, n_slices, cover)
                        total += _evaluate(items, mat)
                    case = (rows, words, shaping, world, pair_space)
                    assert len(runs) == 1, case   # every rank cuts the slices at the same run length
                    assert np.array_equal(cover, np.broadcast_to(expect, cover.shape)), case
                    assert total == _want(rows, words), case


def test_form2_cuts_runs_and_keeps_the_diagonal_on_the_first_item_of_a_tile():
    items = dist.strip_plan(1600, 3, 0, 1, 2, 0, max_run=3, tail_run=2)
    assert max(int(j1 - j0) for _, _, j0, j1, _ in items) <= 3
    assert any(diag == 0 for _, diag, _, _, _ in items)   # continuation items without a diagonal
    first = {}
    for a_row0, diag, j0, j1, ks in items.tolist():
        first.setdefault((a_row0, ks), []).append((j0, diag))
    for runs in first.values():
        assert sum(d for _, d in runs) == 1 and min(runs)[1] == 1


def test_forms_0_and_1_are_what_they_were_beside_form_2():
    """(tests/test_plan_golden.py pins their digests; here: form 2 is a list of its own and an unknown form is refused)"""
    a = dist.strip_plan(1100, 130, 0, 1, 1)
    b = dist.strip_plan(1100, 130, 0, 1, 2)
    assert a[:, 0].max() % 256 == 0 and b[:, 0].max() % 512 == 0
    assert a[:, 4].max() + 1 == 2 * ((130 + 7) // 8) and b[:, 4].max() + 1 == 65
    lib = _lib.load()
    n = C.c_uint64(0)
    assert lib.storm_hip_strip_plan3(1100, 130, 0, 1, 3, 0, 0, 32, 3, 6, 256, None, 0, C.byref(n), None) != 0


def test_the_option_that_selects_the_form():
    lib = _lib.load()
    lib.storm_hip_option_check.argtypes = [C.c_char_p, C.c_int64]
    for value in (0, 64, 128):
        assert lib.storm_hip_option_check(b"k2_strip_rows", value) == 0, value
    for value in (-1, 1, 32, 63, 65, 127, 129, 256, 512):
        assert lib.storm_hip_option_check(b"k2_strip_rows", value) != 0, value
    assert lib.storm_hip_option_check(b"k2_strip_rows_used", 128) != 0   # read-only
    assert lib.storm_hip_option_check(b"k2_strip_operands", 7) != 0
    assert lib.storm_hip_option_check(b"k2_strip_operands", 6) == 0
