"""CPU side of tests/test_gpu_dense_edges.py: the shapes of its limit cases, re-derived with the host-only planners (no
device is touched), and the input families' closed forms against the plain numpy product. What keeps the GPU cases
meaningful when somebody retunes a planner: a shape that no longer sits on its limit fails HERE, on any machine."""
import numpy as np
import pytest

from stormbitmaps_amd import dist
from tests import _dense_edges as de

N_CUS = (256, 304, 64)     # MI355X, MI300X, and a small part: whatever the GPU file may meet


@pytest.mark.parametrize("n_cus", N_CUS)
def test_k2h_parts_sit_on_the_16_bit_window_limit(n_cus):
    """Case 1: with 254 chunks and k2_part_min_chunks 127 every tile is cut into two `narrow` parts of exactly 127 chunks
    (127 x 512 = 65024 < 2^16), with 256 chunks and min_chunks 128 into two WIDE parts of 128 (65536: one more than a 16-bit
    count holds) — for triangles, the band that starts inside a tile and the rectangle, one and two slots per CU."""
    for slots in de.K2H_SLOTS:
        de.assert_k2h_on_limit(dist, de.K2H_NARROW, n_cus, slots)
        de.assert_k2h_on_limit(dist, de.K2H_WIDE, n_cus, slots)
    assert de.K2H_NARROW["part_chunks"] * 512 < (1 << 16) <= de.K2H_WIDE["part_chunks"] * 512


def test_k2h_never_plans_a_narrow_part_beyond_127_chunks():
    """... and whatever the shape, a part flagged `narrow` has at most 127 chunks (rows of 1 .. 1200 chunks, every slot rule)."""
    for n_rows, n_rows_b in ((130, 0), (300, 0), (1000, 0), (200, 257)):
        for chunks in (1, 126, 127, 128, 129, 253, 254, 255, 256, 257, 381, 382, 1016, 1200):
            for slots in de.K2H_SLOTS:
                for min_chunks in (1, 8, 127, 128):
                    p = dist.matrix_plan(n_rows, 8 * chunks, n_rows_b=n_rows_b, slots_per_cu=slots, min_chunks=min_chunks)
                    narrow = p[p[:, 7] == 1]
                    assert len(narrow) == 0 or narrow[:, 3].max() <= 127, (n_rows, chunks, slots, min_chunks)
                    for t in np.unique(p[:, 4]):     # a tile's parts are all narrow or all wide, and cover [0, chunks)
                        parts = p[p[:, 4] == t]
                        assert len(set(parts[:, 7].tolist())) == 1 and int(parts[:, 3].sum()) == chunks


@pytest.mark.parametrize("n_cus", (256, 304))
def test_k2h_whole_tiles_end_at_two_to_the_24_bits(n_cus):
    """Case 2: 2945 rows are 300 tiles of 128 x 128 — at least one whole round on 256 and 304 CUs — so at 2^24 - 512 bits the
    plan holds whole tiles of 32767 chunks, the longest item whose f32 sums stay exact; from 2^24 bits on every tile is cut."""
    de.assert_k2h_whole_tiles_on_limit(dist, n_cus)


def test_few_tiles_are_cut_for_load_balance_long_before_the_exactness_cut():
    """Why case 2 needs 2945 rows (and why the older 70-row test cannot see a missing cut): with few tiles the planner cuts
    every tile into many short parts whatever the row length."""
    for bits in (de.EXACT - 512, de.EXACT + 512):
        p = dist.matrix_plan(130, bits // 64)
        assert p[:, 3].max() * 512 < de.EXACT // 16


@pytest.mark.parametrize("n_cus", (256, 304))
def test_strip_items_reach_a_run_of_4096_stages(n_cus):
    """Case 3: with k2_max_run = k2_tail_run = 4096 a matrix of 4100 blocks of 64 rows holds items whose run of later blocks
    is exactly 4096 (the longest a strip accumulator is sized for); with either knob at its default it does not."""
    for n_rows in de.STRIP_LONG_ROWS:
        for form in (0, 1):
            assert de.longest_run(dist, n_rows, de.STRIP_LONG_WORDS, form, 4096, 4096, n_cus) == 4096, (n_rows, form)
        assert de.longest_run(dist, n_rows, de.STRIP_LONG_WORDS, 1, 4096, 32, n_cus) <= 32
        assert de.longest_run(dist, n_rows, de.STRIP_LONG_WORDS, 1, 0, 4096, n_cus) <= 128
    for n_rows in de.STRIP_RAGGED_ROWS:
        for bits in de.STRIP_RAGGED_BITS:
            for max_run, tail_run in de.STRIP_RUNS:
                assert de.longest_run(dist, n_rows, de.n_words_of(bits), 1, max_run, tail_run, n_cus) <= max(128, max_run)


def test_default_stream_shares_are_nowhere_near_the_limit():
    """Case 4: by default the K2q stream is cut into shares of ~80 stages (so no default run comes near kBsMaxStages = 8192
    — the GPU case forces one workgroup per CU); a CU's share of the case's streams is beyond 2048 stages."""
    segs, groups = dist.stream_plan(8192, 8192)
    per_group = np.bincount(segs[:, 0], weights=segs[:, 7], minlength=groups)
    assert per_group.max() <= 128 and groups > 20000
    for n_rows in de.STREAM_ROWS:
        segs, groups = dist.stream_plan(n_rows, de.STREAM_BITS // 64)
        assert 2048 < int(segs[:, 7].sum()) // 256 and (int(segs[:, 7].sum()) + 303) // 304 > 2048, n_rows


def test_input_families_against_the_numpy_product():
    """The references themselves: closed forms == every bit unpacked and an int64 matrix product, at small sizes with the
    same edges (last word masked, lengths around words / stages / chunks, suffix rows, every periodic phase)."""
    for M in (512, 1000, 2050):
        sat = de.saturated(5, M)
        assert (de.numpy_counts(sat) == M).all() and (de.numpy_counts(sat, op="or") == M).all()
        assert (de.numpy_counts(sat, op="xor") == 0).all()
        assert int(sat[:, -1].max()) == (1 << ((M - 1) % 64 + 1)) - 1
        for bit in (0, M - 1):
            odd = de.saturated(4, M, clear=(bit,))
            assert (de.numpy_counts(odd) == M - 1).all() and (de.numpy_counts(odd, op="xor") == 0).all()
        L = de.staircase_lengths(M, cut_chunks=(1, 2))
        S = [s for s in (0, 1, 64, 65, 511, 513, M - 1, M) if s <= M]
        mat = de.staircase(M, L, S)
        na, nb, cnt = de.staircase_counts(M, L, S)
        for op in ("and", "or", "xor"):
            assert np.array_equal(de.numpy_counts(mat, op=op), de.op_counts(na, nb, cnt, op)), (M, op)
        assert np.array_equal(de.numpy_counts(mat).diagonal(), na)
        b = de.staircase(M, L[::3], S[::2])
        _, nb2, cnt2 = de.staircase_counts(M, L, S, L[::3], S[::2])
        assert np.array_equal(de.numpy_counts(mat, b), cnt2) and np.array_equal(de.numpy_counts(b).diagonal(), nb2)
    per = de.periodic(2048, de.PERIODIC_SPECS)
    cnt = de.numpy_counts(per)
    for i, (p, t) in enumerate(de.PERIODIC_SPECS):
        assert cnt[i, i] == len(range(t, 2048, p))
        for j, (q, u) in enumerate(de.PERIODIC_SPECS):     # nested periods: (q | p) the finer row holds the coarser one or misses it
            if p % q == 0:
                assert cnt[i, j] == (cnt[i, i] if t % q == u else 0), (p, t, q, u)
    assert {t for p, t in de.PERIODIC_SPECS if p == 4} == {0, 1, 2, 3}     # K2b's class pairs split bits by (b % 4) // 2


def test_an_odd_count_beyond_two_to_the_24_is_what_an_uncut_f32_sum_loses():
    """Why the exactness cases use ODD-saturated rows: an f32 accumulator fed 128 per step stays exact past 2^24 on all-ones
    rows (every partial sum is even) and loses the one odd step otherwise."""
    M, step = de.EXACT + 512, 128

    def f32_sum(first):
        acc = np.float32(first)
        for _ in range(M // step - 1):
            acc = np.float32(acc + np.float32(step))
        return int(acc)

    assert f32_sum(step) == M                       # all ones: correct by luck
    assert f32_sum(step - 1) != M - 1               # bit 0 cleared: the uncut sum is wrong
    assert (M - 1) % 2 == 1
    for bits in de.EXACT_BITS:
        assert bits % 512 == 0 and (bits - 1) % 2 == 1 and bits < (1 << 25)
