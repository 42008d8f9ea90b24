"""CPU tests of the K2h planner for the RECTANGLE of the dosage form (storm_hip_dosage_square_plan, what
storm_hip_square_dosage_matrix_device launches): every 128 x 128 tile of n_a x n_b exactly once per k-part, under the two
limits of a chunk that weighs 9 x 256 — an item's chunks x 2304 <= 2^24 (at most 7281 chunks), 16-bit windows only while a
part's chunks x 2304 <= 65535 (at most 28). The triangle's planner (storm_hip_dosage_plan) keeps refusing a second matrix;
the plans of the bit form are held to their committed digests by tests/test_plan_golden.py."""
import ctypes as C

import numpy as np
import pytest

import stormbitmaps_amd as sb
from stormbitmaps_amd import dist

WEIGHT = 9 * 256


def check(plan, n_a, n_b, n_words):
    n_chunks = (n_words + 7) // 8
    ta, tb = (n_a + 127) // 128, (n_b + 127) // 128
    j0 = (n_a + 255) // 256 * 2                   # B's tiles count on behind A's rows padded to 256
    tiles = {}
    for I, J, c0, n, tile, part, n_parts, narrow in plan.tolist():
        tiles.setdefault(tile, []).append((part, c0, n, n_parts, I, J, narrow))
    seen = []
    for tile, parts in tiles.items():
        parts.sort()
        assert [p[0] for p in parts] == list(range(len(parts)))
        assert all(p[3] == len(parts) for p in parts)
        assert len({(p[4], p[5]) for p in parts}) == 1
        assert len({p[6] for p in parts}) == 1                    # a tile's windows are all narrow or all wide
        seen.append((parts[0][4], parts[0][5]))
        pos = 0
        for _, c0, n, _, _, _, narrow in parts:
            assert c0 == pos and n >= 1                            # the parts tile the chunk range exactly once
            assert n <= 7281 and n * WEIGHT <= 1 << 24             # an item's sums stay exact in f32
            assert not narrow or (len(parts) > 1 and n <= 28 and n * WEIGHT <= 65535)
            pos += n
        assert pos == n_chunks
    assert len(seen) == len(set(seen))                             # no tile is listed twice
    assert set(seen) == {(i, j0 + j) for i in range(ta) for j in range(tb)}   # exactly the rectangle's tiles
    return tiles


@pytest.mark.parametrize("n_cus", [1, 256])
@pytest.mark.parametrize("n_words", [1, 8, 464, 65536])
@pytest.mark.parametrize("n_a,n_b", [(1, 1), (2, 129), (129, 2), (257, 130), (300, 1500), (1500, 300)])
def test_rectangle_plans_cover_every_tile_and_chunk_once_within_both_limits(n_a, n_b, n_words, n_cus):
    plan = dist.dosage_square_plan(n_a, n_b, n_words, n_cus=n_cus)
    tiles = check(plan, n_a, n_b, n_words)
    assert (np.diff(plan[:, 3].astype(np.int64)) <= 0).all()      # longest first
    if n_words == 65536:
        # S = 2^21: 8192 chunks x 2304 > 2^24, so even a lone tile on a lone CU is cut
        assert all(len(parts) >= 2 for parts in tiles.values())


def test_a_lone_tile_of_long_rows_is_cut_at_the_exactness_limit():
    for n_chunks, parts in ((7281, 1), (7282, 2)):
        plan = dist.dosage_square_plan(3, 3, 8 * n_chunks, n_cus=1, slots_per_cu=1, min_chunks=4096)
        assert len(plan) == parts, (n_chunks, plan.tolist())
        check(plan, 3, 3, 8 * n_chunks)


def test_windows_are_narrow_up_to_28_chunks_a_part_and_wide_from_29():
    # 130 x 130 rows = 4 tiles on 256 CUs: every tile is cut down to min_chunks
    for n_chunks, min_chunks, narrow in ((56, 28, 1), (58, 29, 0), (28 * 3, 28, 1), (29 * 3, 29, 0)):
        plan = dist.dosage_square_plan(130, 130, 8 * n_chunks, n_cus=256, min_chunks=min_chunks)
        check(plan, 130, 130, 8 * n_chunks)
        assert (plan[:, 6] >= 2).all()
        assert int(plan[:, 3].max()) == min_chunks
        assert (plan[:, 7] == narrow).all(), (n_chunks, min_chunks)


def test_bad_arguments_are_refused_and_the_triangle_planner_still_refuses_a_second_matrix():
    lib = sb.load()
    n = C.c_uint64(0)

    def square(n_a, n_b, n_words, n_cus, min_chunks=8):
        return lib.storm_hip_dosage_square_plan(n_a, n_b, n_words, n_cus, 0, min_chunks, 80, None, 0, C.byref(n))
    assert square(100, 100, 8, 256) == 0 and n.value >= 1
    assert square(0, 100, 8, 256) == -1
    assert b"dosage_square_plan" in lib.storm_hip_last_error()
    assert square(100, 0, 8, 256) == -1
    assert square(100, 100, 0, 256) == -1
    assert square(100, 100, 8, 0) == -1
    assert square(100, 100, 8, 256, min_chunks=0) == -1
    assert lib.storm_hip_dosage_square_plan(100, 100, 8, 256, 0, 8, 80, None, 0, None) == -1
    # too small a capacity
    out = np.zeros((1, 8), dtype=np.uint32)
    assert lib.storm_hip_dosage_square_plan(300, 300, 8, 256, 0, 8, 80, out.ctypes.data, 1, C.byref(n)) == -1
    # the triangle's planner: n_rows_b must stay 0
    assert lib.storm_hip_dosage_plan(100, 100, 8, 0, 0, 256, 0, 8, 80, None, 0, C.byref(n)) == -1
    assert b"dosage_plan" in lib.storm_hip_last_error()
