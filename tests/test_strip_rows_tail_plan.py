"""The tail of strip16_rows_kernel's work list chosen with its run length (strip_plan form 2, tail_run = 0: neither tail
option set, which is what a context that was given no options launches), without a device.

  * The scheduling model behind the choice (storm_hip_plan.h: strip_rows_makespan, strip_rows_item_cost), answered by
    tests/strip_rows_tail/driver.cpp on lists made by hand, against schedules worked out by hand (below, case by case);
    the same driver under AddressSanitizer + UBSan (a stand-alone program) answers the same and is clean.
  * The chosen lists at 2048, 2560, 4096, 10000 and 20000 rows x 1024 words and at 2048 x 1094: every (slice, A block,
    B block) of the upper triangle exactly once, runs of at most 4096 stages, one diagonal item per (tile, slice), the
    shaping one of the candidates; at the two smallest shapes the list adds up to the oracle's total by the kernel's rule.
  * What does not move: explicit options give the list they always gave (14520 items at the headline shape), and the
    ranks of a world of 2 or 3 get the lists of the explicit defaults byte for byte."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from stormbitmaps_amd import dist
from tests.test_strip_rows_plan import _cover, _evaluate

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCE = os.path.join(HERE, "strip_rows_tail", "driver.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "stormbitmaps_amd", "csrc")]

# kStripRowsShapings (storm_hip_plan.h): the three run lengths x {the tail as it was, a long tail, a tail of shorter runs}
CANDIDATES = {(run, tail_run, tail_slices) for run in (96, 64, 128) for tail_run, tail_slices in ((32, 3), (32, 12), (24, 8))}
SHAPES = ((2048, 1024), (2560, 1024), (4096, 1024), (10000, 1024), (20000, 1024), (2048, 1094))

needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

# (query, answer in stages). A list on n_cus x slots_per_cu slots; a group waits `latency`, then shares its unit's pipe.
HAND = [
    # one item: its start, then its 7 stages alone on a pipe
    ("s 32 4 0 7", 7.0),
    ("s 32 4 2.5 7", 9.5),
    # a tile's first item with nothing behind the diagonal: 528 MFMAs = 4 1/8 stages
    ("s 32 4 0 d0", 4.125),
    ("s 1 1 0 d3 5", 12.125),
    # 129 items of 3 stages on 128 slots: four to a pipe, all of them end at 12; the last one then runs alone to 15.
    # With a start of 2: the 128 end at 2 + 12, the last one starts at 14, works from 16 and ends at 19.
    ("s 32 4 0 " + " ".join(["3"] * 129), 15.0),
    ("s 32 4 2 " + " ".join(["3"] * 129), 19.0),
    # 2 units x 2 slots, the long item last: the four short ones share two pipes until 4, then 10 stages alone: 14
    ("s 2 2 0 2 2 2 2 10", 14.0),
    # ... the long item first: unit 0 holds 10 and 2, unit 1 holds 2 and 2; at 4 three groups end, the last item goes to
    # the empty unit 1 (ends at 6) and the long one has 8 stages left alone: 12
    ("s 2 2 0 10 2 2 2 2", 12.0),
    # one unit of 3 slots, start 1, items 4 8 8 2: all three work from 1 at a third each, the 4 ends at 13 (8s: 4 left);
    # the 2 arrives at 13 and waits until 14 while TWO work at a half each (3.5 left); from 14 three work at a third: the
    # 2 ends at 20 (1.5 left), then two at a half: 23
    ("s 1 3 1 4 8 8 2", 23.0),
    # one unit of 2 slots, start 1: 2 2 2 -> both from 1, end at 5; the third waits until 6, ends at 8
    ("s 1 2 1 2 2 2", 8.0),
    # ... 1 3 1 -> the first ends at 3 (the 3 has 2 left), the third waits until 4 while the 3 works alone (1 left), then
    # both share: both end at 6
    ("s 1 2 1 1 3 1", 6.0),
    # no start latency, the same lists: 6; and 1 3 1: the first ends at 2 (3: 2 left), then 3 and 1 share, the 1 ends at 4
    # (3: 1 left), alone to 5
    ("s 1 2 0 2 2 2", 6.0),
    ("s 1 2 0 1 3 1", 5.0),
    # what an item costs: 128 MFMAs a stage; a diagonal 528; a run whose top block holds rows in 1 of its 4 fragments
    # (n_rows 10000: block 156 holds rows 9984 .. 9999) is multiplied in that fragment alone; a last tile of 5 blocks
    ("c 4294967295 0 0 8 104", 96.0),
    ("c 4294967295 0 1 8 104", 96.0 + 528 / 128),
    ("c 10000 0 0 125 157", 31.0 + 0.25),
    ("c 10000 9728 1 160 160", (10 * 5 + 16 * 10) / 128),
]


def build_driver(exe, sanitize=False):
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] \
        if sanitize else ["-O2"]
    return subprocess.run(["g++", "-std=c++17", "-Wall", *flags, *INCLUDES, SOURCE, "-o", str(exe)],
                          capture_output=True, text=True)


def ask(exe, queries):
    run = subprocess.run([str(exe)], input="".join(q + "\n" for q in queries), capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-3000:])
    lines = run.stdout.split("\n")[:-1]
    assert len(lines) == len(queries)
    return [float(ln) for ln in lines], run.stderr


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("strip_rows_tail") / "tail"
    build = build_driver(exe)
    assert build.returncode == 0, build.stderr
    return exe


@needs_gxx
def test_the_model_on_lists_made_by_hand(driver):
    got, _ = ask(driver, [q for q, _ in HAND])
    wrong = [(q[:40], g, w) for (q, w), g in zip(HAND, got) if abs(g - w) > 1e-6]
    assert not wrong, wrong


@needs_gxx
def test_the_model_keeps_the_pipes_busy_and_orders_lists_as_expected(driver):
    """Bounds that hold for any list: no shorter than the work over the units, no shorter than the longest item with its
    start; and the longest item LAST is never better than the same list longest first."""
    rng = np.random.default_rng(5)
    queries, bounds = [], []
    for _ in range(40):
        n_cus, slots = int(rng.integers(1, 6)), int(rng.integers(1, 5))
        latency = float(rng.integers(0, 4)) * 0.5
        runs = rng.integers(1, 40, size=int(rng.integers(1, 60))).tolist()
        for order in (sorted(runs, reverse=True), sorted(runs)):
            queries.append("s %d %d %g %s" % (n_cus, slots, latency, " ".join(str(r) for r in order)))
        bounds.append(max(sum(runs) / n_cus, max(runs) + latency))
    got, _ = ask(driver, queries)
    for k, bound in enumerate(bounds):
        first, last = got[2 * k], got[2 * k + 1]
        assert first >= bound - 1e-6 and last >= bound - 1e-6, (queries[2 * k], first, last, bound)
    assert sum(got[0::2]) < sum(got[1::2])   # longest first is the better order over the lot


@needs_gxx
def test_the_model_under_asan_ubsan(driver, tmp_path):
    exe = tmp_path / "tail_sanitized"
    build = build_driver(exe, sanitize=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan not installed")
    assert build.returncode == 0, build.stderr
    queries = [q for q, _ in HAND] + ["s 3 2 1.5 " + " ".join(str(1 + (7 * k) % 23) for k in range(200)), "s 32 4 8 d96 96 64 d32 5"]
    got, stderr = ask(exe, queries)
    assert "Sanitizer" not in stderr and "runtime error" not in stderr, stderr[-3000:]
    assert got == ask(driver, queries)[0]


def _chosen(rows, words):
    return dist.strip_plan(rows, words, 0, 1, 2, tail_run=0, return_run=True)


@pytest.mark.parametrize("rows,words", SHAPES)
def test_the_chosen_list_covers_every_block_pair_and_slice_once(rows, words):
    items, shaping = _chosen(rows, words)
    assert shaping in CANDIDATES, shaping
    blocks, n_slices = (rows + 63) // 64, (words + 1) // 2
    assert int((items[:, 3] - items[:, 2]).max()) <= 4096
    assert set(np.unique(items[:, 4]).tolist()) == set(range(n_slices))
    # exactly one diagonal item per (tile, slice)
    diag = items[items[:, 1] == 1]
    pairs = np.unique(diag[:, [0, 4]], axis=0)
    assert len(pairs) == len(diag) == n_slices * ((rows + 511) // 512)
    # the cover, slice by slice; slices cut alike (the same items but for the slice number) are covered once
    expect = np.triu(np.ones((blocks, blocks), dtype=np.int32))
    order = np.lexsort((items[:, 3], items[:, 2], items[:, 1], items[:, 0], items[:, 4]))
    by_slice = items[order]
    bounds = np.searchsorted(by_slice[:, 4], np.arange(n_slices + 1))
    seen = set()
    for ks in range(n_slices):
        one = by_slice[bounds[ks]:bounds[ks + 1]].copy()
        one[:, 4] = 0
        key = one.tobytes()
        if key in seen:
            continue
        seen.add(key)
        cover = np.zeros((1, blocks, blocks), dtype=np.int32)
        _cover(one, blocks, 1, cover)
        assert np.array_equal(cover[0], expect), (rows, words, ks)
    assert 1 <= len(seen) <= 3   # the main slices, the tail's, and an odd last slice is cut no differently


@pytest.mark.parametrize("rows,words", sorted(SHAPES, key=lambda s: s[0] * s[1])[:2])
def test_the_chosen_list_adds_up_to_the_oracle(rows, words):
    from tests._orc import Oracle
    rng = np.random.default_rng(rows * 131 + words)
    mat = rng.integers(0, 1 << 63, size=(rows, words), dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, size=(rows, words), dtype=np.uint64)
    mat[rows // 2] = 0
    items, _ = _chosen(rows, words)
    assert _evaluate(items, mat) == Oracle().wrapper_diag_blocked(mat, 31)


@needs_gxx
def test_the_chosen_headline_list_issues_the_mfmas_of_the_explicit_one(driver):
    """However a slice is cut it holds the same work: 195 682 MFMAs per slice at 10000 rows (tests/test_strip_rows_trim.py),
    16 x 512 x that in the kernel's SQ_VALU_MFMA_BUSY_CYCLES. (A cost is a multiple of 1 / 128: the sums are exact.)"""
    items, _ = _chosen(10000, 1024)
    got, _ = ask(driver, ["c 10000 %d %d %d %d" % (a_row0, diag, j0, j1) for a_row0, diag, j0, j1, _ in items.tolist()])
    assert sum(got) * 128 == 195682 * 512


def test_explicit_options_and_the_ranks_of_a_world_keep_their_lists():
    assert len(dist.strip_plan(10000, 1024, 0, 1, 2, max_run=0, tail_run=32, tail_slices=3, lpt_rounds=6, n_cus=256)) == 14520
    for rows, words in ((10000, 1024), (2560, 1024)):
        for world in (2, 3):
            for rank in range(world):
                for pair_space in (0, 1):
                    unset, shaping = dist.strip_plan(rows, words, rank, world, 2, pair_space, tail_run=0, return_run=True)
                    explicit, run = dist.strip_plan(rows, words, rank, world, 2, pair_space, tail_run=32, tail_slices=3, return_run=True)
                    assert shaping == (run, 32, 3)
                    assert unset.tobytes() == explicit.tobytes(), (rows, words, world, rank, pair_space)
    # where the choice stays with the shaping the pass always had, so does the list, byte for byte
    for rows, words in ((2048, 1024), (2560, 1024), (20000, 1024), (2048, 1094)):
        unset, shaping = dist.strip_plan(rows, words, 0, 1, 2, tail_run=0, return_run=True)
        explicit, run = dist.strip_plan(rows, words, 0, 1, 2, return_run=True)
        if shaping == (run, 32, 3):
            assert unset.tobytes() == explicit.tobytes(), (rows, words)
        else:
            assert rows > 2560, (rows, words)   # (up to 40 blocks no run is longer than a tail's: a list that is all tail gains nothing)
    # forms 0 and 1 take the defaults where no tail is set
    for form in (0, 1):
        unset, shaping = dist.strip_plan(3000, 64, 0, 1, form, tail_run=0, return_run=True)
        explicit, run = dist.strip_plan(3000, 64, 0, 1, form, return_run=True)
        assert shaping == (run, 32, 3) and unset.tobytes() == explicit.tobytes()


def test_a_set_run_length_is_kept_and_the_choice_is_the_same_every_time():
    items, shaping = dist.strip_plan(10000, 1024, 0, 1, 2, max_run=80, tail_run=0, return_run=True)
    assert shaping[0] == 80 and shaping[1:] in {(32, 3), (32, 12), (24, 8)}
    assert int((items[:, 3] - items[:, 2]).max()) <= 80
    again, shaping2 = dist.strip_plan(10000, 1024, 0, 1, 2, max_run=80, tail_run=0, return_run=True)
    assert shaping2 == shaping and again.tobytes() == items.tobytes()
