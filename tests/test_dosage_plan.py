"""CPU tests of the K2h planner in its dosage form (storm_hip_dosage_plan): rows of 2-bit values, where one 512-bit chunk
(256 values of 0 .. 3 on either side) can add 9 x 256 = 2304 to an accumulator instead of 512. The two limits that follow
from that weight — an item's chunks x 2304 <= 2^24 (exact f32 accumulation: at most 7281 chunks), 16-bit windows only
while a part's chunks x 2304 <= 65535 (at most 28 chunks) — and the cover of every tile and chunk exactly once. The plans
of the bit form (storm_hip_matrix_plan) are held to their committed digests by tests/test_plan_golden.py."""
import ctypes as C

import numpy as np
import pytest

import stormbitmaps_amd as sb

WEIGHT = 9 * 256


def dosage_plan(n_rows, n_words, n_cus, slots_per_cu=0, min_chunks=8, diag_cost_pct=80, n_rows_b=0):
    lib = sb.load()
    n = C.c_uint64(0)
    args = (n_rows, n_rows_b, n_words, 0, 0, n_cus, slots_per_cu, min_chunks, diag_cost_pct)
    rc = lib.storm_hip_dosage_plan(*args, None, 0, C.byref(n))
    if rc != 0:
        return rc
    out = np.zeros((max(n.value, 1), 8), dtype=np.uint32)
    assert lib.storm_hip_dosage_plan(*args, out.ctypes.data, n.value, C.byref(n)) == 0
    return out[:n.value]


def check(plan, n_rows, n_words):
    n_chunks = (n_words + 7) // 8
    nt = (n_rows + 127) // 128
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
            assert n * WEIGHT <= 1 << 24                           # an item's sums stay exact in f32
            assert not narrow or (len(parts) > 1 and n * WEIGHT <= 65535)
            pos += n
        assert pos == n_chunks
    assert len(seen) == len(set(seen))                             # no tile is listed twice
    assert set(seen) == {(i, j) for i in range(nt) for j in range(i, nt)}   # exactly the triangle's tiles
    return tiles


@pytest.mark.parametrize("n_cus", [1, 256])
@pytest.mark.parametrize("n_words", [1, 8, 464, 65536])
@pytest.mark.parametrize("n_rows", [2, 129, 300, 1500])
def test_dosage_plans_cover_every_tile_and_chunk_once_within_both_limits(n_rows, n_words, n_cus):
    plan = dosage_plan(n_rows, n_words, n_cus)
    tiles = check(plan, n_rows, n_words)
    assert (np.diff(plan[:, 3].astype(np.int64)) <= 0).all()      # longest first
    if n_words == 65536:
        # S = 2^21: 8192 chunks x 2304 > 2^24, so even a lone tile on a lone CU is cut
        assert all(len(parts) >= 2 for parts in tiles.values())


def test_a_lone_tile_of_long_rows_is_cut_at_the_exactness_limit():
    plan = dosage_plan(2, 65536, 1)
    assert len(plan) >= 2 and int(plan[:, 3].max()) <= 7281 and int(plan[:, 3].sum()) == 8192
    # the longest rows one item may still cover, and the first that it may not
    for n_chunks, parts in ((7281, 1), (7282, 2)):
        plan = dosage_plan(2, 8 * n_chunks, 1, slots_per_cu=1, min_chunks=4096)
        assert len(plan) == parts, (n_chunks, plan.tolist())
        check(plan, 2, 8 * n_chunks)
    # the same rows as bits: one item up to 32767 chunks
    from stormbitmaps_amd import dist
    assert len(dist.matrix_plan(2, 8 * 7282, n_cus=1, slots_per_cu=1, min_chunks=4096)) == 1


def test_windows_are_narrow_up_to_28_chunks_a_part_and_wide_from_29():
    # 130 rows = 3 tiles on 256 CUs: every tile is cut down to min_chunks
    for n_chunks, min_chunks, narrow in ((56, 28, 1), (58, 29, 0), (28 * 3, 28, 1), (29 * 3, 29, 0)):
        plan = dosage_plan(130, 8 * n_chunks, 256, min_chunks=min_chunks)
        check(plan, 130, 8 * n_chunks)
        assert (plan[:, 6] >= 2).all()
        assert int(plan[:, 3].max()) == min_chunks
        assert (plan[:, 7] == narrow).all(), (n_chunks, min_chunks)


def test_bad_arguments_are_refused():
    lib = sb.load()
    assert dosage_plan(0, 8, 256) == -1
    assert dosage_plan(100, 0, 256) == -1
    assert dosage_plan(100, 8, 0) == -1
    assert dosage_plan(100, 8, 256, n_rows_b=100) == -1      # the rectangle has no dosage form
    assert b"dosage_plan" in lib.storm_hip_last_error()
    assert dosage_plan(100, 8, 256, min_chunks=0) == -1
