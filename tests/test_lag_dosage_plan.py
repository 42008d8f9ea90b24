"""CPU tests of the host-only planner of the dosage form in the lag layout (storm_hip_lag_dosage_plan): the K2h item list
for the pairs i < j with j - i <= L = min(max_lag, n_rows - 1) of rows of 2-bit values. Two rules meet here and both are
stated from their definitions: the tiles are exactly those that hold a wanted pair (tests/test_lag_plan.py's enumeration of
the pairs, with the lone-row tile it names), and the parts obey the dosage weight of 9 x 256 a chunk — an item's chunks x
2304 <= 2^24, 16-bit windows only while a part's chunks x 2304 <= 65535 (tests/test_dosage_plan.py's two cuts). The
interleaved layout of the pairwise-complete call (3 n rows at lag 3 L + 2) is planned by the same call; its cover of the
nine products of every wanted row pair is checked here from the pairs themselves."""
import ctypes as C

import numpy as np
import pytest

from stormbitmaps_amd import _lib, dist
from tests.test_lag_plan import T, _lone_row_tile, _wanted_tiles

WEIGHT = 9 * 256


def tiles_and_cover(plan, n_chunks):
    """the plan's tiles; a tile's parts tile [0, n_chunks) exactly once, within both limits of the dosage weight"""
    by_tile = {}
    for I, J, c0, n, tile, part, n_parts, narrow in plan.tolist():
        by_tile.setdefault(tile, []).append((part, c0, n, n_parts, I, J, narrow))
    seen = []
    for parts in by_tile.values():
        parts.sort()
        assert [p[0] for p in parts] == list(range(len(parts))) and all(p[3] == len(parts) for p in parts)
        assert len({(p[4], p[5]) for p in parts}) == 1
        assert len({p[6] for p in parts}) == 1
        pos = 0
        for _, c0, n, _, _, _, narrow in parts:
            assert c0 == pos and n >= 1 and n * WEIGHT <= 1 << 24
            assert not narrow or (len(parts) > 1 and n * WEIGHT <= 65535)
            pos += n
        assert pos == n_chunks
        seen.append((parts[0][4], parts[0][5]))
    assert len(seen) == len(set(seen)), "a tile listed twice: its pairs would be covered twice"
    return set(seen), by_tile


@pytest.mark.parametrize("n_rows", [2, 129, 300, 1500])
@pytest.mark.parametrize("n_words", [1, 464, 65536])
@pytest.mark.parametrize("n_cus", [1, 256])
def test_lag_dosage_plans_list_exactly_the_tiles_with_a_wanted_pair(n_rows, n_words, n_cus):
    n_chunks = (n_words + 7) // 8
    triangle, _ = tiles_and_cover(dist.dosage_plan(n_rows, n_words, n_cus=n_cus), n_chunks)
    for max_lag in (1, 127, 128, 129, n_rows - 1, 10 * n_rows):
        lag = min(max_lag, n_rows - 1)
        plan = dist.lag_dosage_plan(n_rows, n_words, max_lag, n_cus=n_cus)
        tiles, by_tile = tiles_and_cover(plan, n_chunks)
        assert tiles == _wanted_tiles(n_rows, lag) | _lone_row_tile(n_rows), (n_rows, max_lag)
        # the same tiles as the bit form's list: the rule does not ask what a word holds
        assert tiles == {(int(I), int(J)) for I, J in dist.lag_plan(n_rows, n_words, max_lag, n_cus=n_cus)[:, :2]}
        assert (np.diff(plan[:, 3].astype(np.int64)) <= 0).all()           # longest first
        if n_words == 65536:   # 8192 chunks x 2304 > 2^24: every tile is cut, whatever the lag
            assert all(len(parts) >= 2 for parts in by_tile.values())
        if max_lag >= n_rows - 1:
            assert tiles == triangle


@pytest.mark.parametrize("n_rows,max_lag,band", [(700, 200, (0, 130)), (700, 200, (130, 512)), (700, 200, (512, 700)),
                                                 (1500, 129, (1279, 1281))])
def test_a_row_band_lists_exactly_the_tiles_of_its_rows(n_rows, max_lag, band):
    lag = min(max_lag, n_rows - 1)
    plan = dist.lag_dosage_plan(n_rows, 64, max_lag, band_row0=band[0], band_rows=band[1] - band[0])
    tiles, _ = tiles_and_cover(plan, 8)
    rows = range(band[0] // T, (band[1] + T - 1) // T)
    assert tiles == {t for t in _wanted_tiles(n_rows, lag) | _lone_row_tile(n_rows, band) if t[0] in rows}
    assert _wanted_tiles(n_rows, lag, band) <= tiles


def test_the_two_cuts_of_the_dosage_weight_fall_where_the_triangle_s_do():
    # an item covers at most 7281 chunks (x 2304 <= 2^24): two rows, one CU, lag 1
    for n_chunks, parts in ((7281, 1), (7282, 2)):
        plan = dist.lag_dosage_plan(2, 8 * n_chunks, 1, n_cus=1, slots_per_cu=1, min_chunks=4096)
        assert len(plan) == parts, (n_chunks, plan.tolist())
        tiles_and_cover(plan, n_chunks)
    assert len(dist.lag_plan(2, 8 * 7282, 1, n_cus=1, slots_per_cu=1, min_chunks=4096)) == 1   # as bits: one item
    # windows are narrow up to 28 chunks a part and wide from 29: 130 rows on 256 CUs, every tile cut down to min_chunks
    for n_chunks, min_chunks, narrow in ((56, 28, 1), (58, 29, 0), (28 * 3, 28, 1), (29 * 3, 29, 0)):
        for max_lag in (1, 129):
            plan = dist.lag_dosage_plan(130, 8 * n_chunks, max_lag, n_cus=256, min_chunks=min_chunks)
            tiles_and_cover(plan, n_chunks)
            assert (plan[:, 6] >= 2).all() and int(plan[:, 3].max()) == min_chunks
            assert (plan[:, 7] == narrow).all(), (n_chunks, min_chunks, max_lag)
            # the bit-weighted list of the same shape keeps narrow windows at 29 chunks: the weight is what differs
            assert (dist.lag_plan(130, 8 * n_chunks, max_lag, n_cus=256, min_chunks=min_chunks)[:, 7] == 1).all()


@pytest.mark.parametrize("n,L", [(50, 1), (50, 41), (50, 42), (50, 43), (200, 85), (200, 86), (130, 129)])
def test_the_interleaved_rows_at_lag_3L_plus_2_hold_all_nine_products_of_every_wanted_pair(n, L):
    """rows 3 i + a, 3 j + b of the interleaved split for 0 < j - i <= L are at most 3 L + 2 apart, so the list of 3 n rows
    at that lag holds a tile for each of them; and column 3 d + 2 + b - a of the lag layout is where
    dosage_complete_finish_lag_kernel looks for them"""
    plan = dist.lag_dosage_plan(3 * n, 8, 3 * L + 2)
    tiles, _ = tiles_and_cover(plan, 1)
    i = np.arange(n)[:, None]
    j = i + np.arange(1, L + 1)[None, :]
    ok = j < n
    i, j = np.broadcast_to(i, j.shape)[ok], j[ok]
    for a in range(3):
        for b in range(3):
            r, c = 3 * i + a, 3 * j + b
            assert ((c - r >= 1) & (c - r <= 3 * L + 2)).all()
            assert np.array_equal(c - r - 1, 3 * (j - i - 1) + 2 + b - a)
            assert set(zip((r // T).tolist(), (c // T).tolist())) <= tiles


def test_bad_arguments_and_the_count_query(lib):
    n = C.c_uint64(7)
    f = lib.storm_hip_lag_dosage_plan
    assert f(300, 16, 0, 0, 0, 256, 0, 8, 80, None, 0, C.byref(n)) == -1          # max_lag 0
    assert b"lag_dosage_plan" in lib.storm_hip_last_error()
    assert f(0, 16, 5, 0, 0, 256, 0, 8, 80, None, 0, C.byref(n)) == -1
    assert f(300, 16, 5, 0, 0, 256, 0, 8, 80, None, 0, None) == -1
    assert f(300, 16, 5, 0, 0, 256, 0, 0, 80, None, 0, C.byref(n)) == -1          # min_chunks 0
    assert f(300, 16, 5, 0, 0, 256, 0, 8, 80, None, 0, C.byref(n)) == 0 and n.value == len(dist.lag_dosage_plan(300, 16, 5))
    out = np.zeros((int(n.value) - 1, 8), dtype=np.uint32)
    assert f(300, 16, 5, 0, 0, 256, 0, 8, 80, out.ctypes.data_as(C.c_void_p), n.value - 1, C.byref(n)) == -1   # capacity
    assert f(1, 16, 5, 0, 0, 256, 0, 8, 80, None, 0, C.byref(n)) == 0 and n.value == 0   # one row: no pairs
    assert f(300, 16, 5, 300, 0, 256, 0, 8, 80, None, 0, C.byref(n)) == 0 and n.value == 0   # a band behind the rows
    assert "storm_hip_lag_dosage_plan" in _lib.SIGNATURES
