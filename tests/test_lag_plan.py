"""CPU tests of the host-only planner of the lag layout (storm_hip_lag_plan): the K2h item list for the pairs i < j with
j - i <= L = min(max_lag, n_rows - 1). What is wanted is stated here from the definition alone — a tile (I, J) of 128 x 128
rows is wanted exactly when one of its pairs has a lag within L, found by enumerating the pairs — and the plan must cover
every (wanted pair, 512-bit chunk) exactly once, list no tile without a wanted pair, and equal the triangle's tiles once
the lag spans the matrix.

One tile is listed without a wanted pair: the last diagonal tile when it holds a single row (n_rows % 128 == 1). The tile
rule (I <= J <= (128 I + 127 + L) / 128) lists it, as the triangle's own list always has — it multiplies one row with
itself and writes nothing — and the lag list must equal the triangle's once the lag spans the matrix, so it stays; the
tests name it (`_lone_row_tile`) instead of hiding it."""
import ctypes as C

import numpy as np
import pytest

from stormbitmaps_amd import _lib, dist

T = 128


def _wanted_tiles(n_rows, lag, band=None):
    """the tiles that hold a pair i < j < n_rows, j - i <= lag, i in the band: from the pairs themselves"""
    i0, i1 = band if band else (0, n_rows)
    i = np.arange(i0, i1)[:, None]
    j = i + np.arange(1, lag + 1)[None, :]
    ok = j < n_rows
    return set(zip((np.broadcast_to(i, j.shape)[ok] // T).tolist(), (j[ok] // T).tolist()))


def _lone_row_tile(n_rows, band=None):
    """the last diagonal tile if it holds one row (and the band reaches it): listed, though a single row has no pair"""
    if n_rows % T != 1 or (band and band[1] < n_rows):
        return set()
    return {(n_rows // T, n_rows // T)}


def _tiles_and_cover(plan, n_chunks):
    """the plan's tiles; asserts that a tile's parts tile its chunk range [0, n_chunks) exactly once"""
    by_tile = {}
    for I, J, c0, n, tile, part, n_parts, narrow in plan.tolist():
        by_tile.setdefault(tile, []).append((part, c0, n, n_parts, I, J, narrow))
    seen = []
    for parts in by_tile.values():
        parts.sort()
        assert [p[0] for p in parts] == list(range(len(parts))) and all(p[3] == len(parts) for p in parts)
        assert len({(p[4], p[5]) for p in parts}) == 1
        pos = 0
        for _, c0, n, _, _, _, narrow in parts:
            assert c0 == pos and n >= 1 and n * 512 < (1 << 24)
            assert not narrow or (len(parts) > 1 and n <= 127)
            pos += n
        assert pos == n_chunks
        seen.append((parts[0][4], parts[0][5]))
    assert len(seen) == len(set(seen)), "a tile listed twice: its pairs would be covered twice"
    return set(seen)


@pytest.mark.parametrize("n_rows", [2, 129, 300, 1500])
@pytest.mark.parametrize("n_words", [16, 1024])
@pytest.mark.parametrize("n_cus", [1, 256])
def test_lag_plans_cover_every_wanted_pair_and_chunk_once(n_rows, n_words, n_cus):
    n_chunks = (n_words + 7) // 8
    triangle = _tiles_and_cover(dist.matrix_plan(n_rows, n_words, n_cus=n_cus), n_chunks)
    for max_lag in (1, 127, 128, 129, n_rows - 1, 10 * n_rows):
        lag = min(max_lag, n_rows - 1)
        plan = dist.lag_plan(n_rows, n_words, max_lag, n_cus=n_cus)
        tiles = _tiles_and_cover(plan, n_chunks)
        # every wanted pair lies in a listed tile (once: no tile twice, parts cover the chunks once), and every listed tile
        # holds a wanted pair
        assert tiles == _wanted_tiles(n_rows, lag) | _lone_row_tile(n_rows), (n_rows, max_lag)
        # the rule as the issue states it
        nt = (n_rows + T - 1) // T
        assert tiles == {(I, J) for I in range(nt) for J in range(I, min(nt - 1, (T * I + T - 1 + lag) // T) + 1)}
        assert (np.diff(plan[:, 3].astype(np.int64)) <= 0).all()           # longest first, as the triangle's list
        if max_lag >= n_rows - 1:
            assert tiles == triangle


@pytest.mark.parametrize("n_rows,max_lag,band", [(700, 200, (0, 257)), (700, 200, (257, 700)), (1500, 70, (300, 1000)),
                                                 (1500, 129, (1279, 1281)), (300, 1000, (299, 300))])
def test_a_row_band_lists_exactly_the_tiles_of_its_rows(n_rows, max_lag, band):
    lag = min(max_lag, n_rows - 1)
    plan = dist.lag_plan(n_rows, 64, max_lag, band_row0=band[0], band_rows=band[1] - band[0])
    tiles = _tiles_and_cover(plan, 8)
    # the tile rows that hold the band, each with its columns of the whole-matrix list (a tile row is listed whole)
    rows = range(band[0] // T, (band[1] + T - 1) // T)
    assert tiles == {t for t in _wanted_tiles(n_rows, lag) | _lone_row_tile(n_rows, band) if t[0] in rows}
    assert _wanted_tiles(n_rows, lag, band) <= tiles


def test_bad_arguments_and_the_count_query(lib):
    n = C.c_uint64(7)
    f = lib.storm_hip_lag_plan
    assert f(300, 16, 0, 0, 0, 256, 0, 8, 80, None, 0, C.byref(n)) == -1          # max_lag 0
    assert f(0, 16, 5, 0, 0, 256, 0, 8, 80, None, 0, C.byref(n)) == -1
    assert f(300, 16, 5, 0, 0, 256, 0, 8, 80, None, 0, None) == -1
    assert f(300, 16, 5, 0, 0, 256, 0, 8, 80, None, 0, C.byref(n)) == 0 and n.value == len(dist.lag_plan(300, 16, 5))
    out = np.zeros((int(n.value) - 1, 8), dtype=np.uint32)
    assert f(300, 16, 5, 0, 0, 256, 0, 8, 80, out.ctypes.data_as(C.c_void_p), n.value - 1, C.byref(n)) == -1   # capacity
    assert f(1, 16, 5, 0, 0, 256, 0, 8, 80, None, 0, C.byref(n)) == 0 and n.value == 0   # one row: no pairs
    assert f(300, 16, 5, 300, 0, 256, 0, 8, 80, None, 0, C.byref(n)) == 0 and n.value == 0   # a band behind the rows


LAG_SYMBOLS = ("storm_hip_lag_plan", "storm_hip_pairw_lag_matrix_device", "storm_hip_pairw_lag_matrix",
               "storm_hip_similarity_finish_lag_device", "storm_hip_pairw_lag_similarity_device",
               "storm_hip_pairw_lag_similarity", "STORM_contig_pairw_lag_matrix", "STORM_contig_pairw_lag_matrix_device",
               "STORM_contig_pairw_lag_similarity", "STORM_contig_pairw_lag_similarity_device", "STORM_pairw_lag_matrix",
               "STORM_pairw_lag_matrix_device", "STORM_pairw_lag_similarity", "STORM_pairw_lag_similarity_device")


def test_the_library_exports_and_binds_the_lag_calls(lib):
    for name in LAG_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_host_conventions_of_the_container_forms_without_a_device(lib):
    """what the storm.h forms answer before any device is touched: NULL handle, NULL out"""
    out = np.zeros(4, dtype=np.uint32)
    p = out.ctypes.data_as(C.c_void_p)
    c = lib.STORM_contig_new(4096)
    s = lib.STORM_new()
    try:
        for f, h in ((lib.STORM_contig_pairw_lag_matrix, c), (lib.STORM_contig_pairw_lag_matrix_device, c),
                     (lib.STORM_pairw_lag_matrix, s), (lib.STORM_pairw_lag_matrix_device, s)):
            assert f(None, 0, 1, p, 2, 2) == -1 and f(h, 0, 1, None, 2, 2) == -2
        for f, h in ((lib.STORM_contig_pairw_lag_similarity, c), (lib.STORM_contig_pairw_lag_similarity_device, c),
                     (lib.STORM_pairw_lag_similarity, s), (lib.STORM_pairw_lag_similarity_device, s)):
            assert f(None, 0, 0, 1, p, 2, 2) == -1 and f(h, 0, 0, 1, None, 2, 2) == -2
    finally:
        lib.STORM_contig_free(c)
        lib.STORM_free(s)
