"""The sparse arena's host-only planners (storm_hip_plan.cpp): the block-column layout, K4's element layout and its two
work lists, the per-launch view of them and K1's segment table, run by tests/arena_plan/driver.cpp without a device.

  * every output array answers what it answered when the code had only been moved out of build_arena
    (tests/golden/arena_plan_digests.json, written by tests/golden/make_arena_digests.py);
  * K4 counts every list x list pair of a column exactly once: per (probe column, octant) stream the items' near and far
    ranges are checked against group bounds computed here from the case's rows;
  * the same driver under AddressSanitizer + UBSan (a stand-alone program) is clean on every case."""
import importlib.util
import json
import os
import shutil

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_arena_digests", os.path.join(HERE, "golden", "make_arena_digests.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

with open(gen.DIGEST_FILE) as f:
    GOLDEN = json.load(f)

EINVAL = -1
ROWS, OCTANTS, BUNDLE = 128, 8, 4   # kProbeRows, kProbeOctants, kFatGroups


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """case name -> the driver's output (every case is planned once)."""
    tmp = tmp_path_factory.mktemp("arena_plan")
    exe = tmp / "arena_plan"
    build = gen.build_driver(exe)
    assert build.returncode == 0, build.stderr
    out = {name: gen.run_case(exe, gen.case_text(gen.case_rows(name)), tmp, name)[0] for name in gen.VALID_CASES}
    for name, (text, _) in gen.invalid_cases().items():
        out["H_" + name] = gen.run_case(exe, text, tmp, name)[0]
    return out


def test_planner_output_is_unchanged(plans):
    got = {f"{name}/{section}": digest for name, doc in plans.items() for section, digest in gen.digests_of(doc).items()}
    assert set(got) == set(GOLDEN)
    wrong = sorted(key for key in GOLDEN if got[key] != GOLDEN[key])
    assert not wrong, wrong


@pytest.mark.parametrize("name", sorted(gen.invalid_cases()))
def test_invalid_descriptions_are_refused(plans, name):
    status = plans["H_" + name]["status"]
    assert status == {"rc": EINVAL, "error": gen.invalid_cases()[name][1]}


def test_eligibility_and_layout_of_the_small_cases(plans):
    a, b, c = (plans[k]["columns"] for k in "ABC")
    assert a["col_probe"] == [1] and a["pool_rows"] == [0, 512] and a["census"] == [1, 0, 0, 1]
    assert b["col_probe"] == [0] and b["census"] == [0, 3, 3, 1] and plans["B"]["probe"]["items"] == []
    # C: 5 bitmap rows, the 300 lists from row 512 on; the dense pass takes the bitmap rows as A rows only
    assert c["col_probe"] == [1] and c["col_list0"] == [512] and c["cols_r0"] == [0] and c["cols_r1"] == [812]
    assert c["pool_rows"] == [1024, 1024]   # a mixed column owns its pool rows from the start


def _streams(name, doc):
    """(column entry, octant) -> (group bounds of the stream, its end), from the case's rows alone."""
    rows = gen.case_rows(name)
    ids = sorted({bid for row in rows for bid, _, _, _ in row})
    cols = doc["columns"]
    regions = {(r[2], r[3]): (r[0], r[1]) for r in doc["probe"]["probe_regions"]}
    out = {}
    for e, cid in enumerate(ids):
        if not cols["col_probe"][e]:
            continue
        lists = [pos for row in rows for bid, kind, pos, _ in row if bid == cid and kind == 0]
        for o in range(OCTANTS):
            counts = [int(np.count_nonzero((pos >= o * 8192) & (pos < (o + 1) * 8192))) for pos in lists]
            if sum(counts) == 0:
                assert (cols["col_list0"][e], o) not in regions
                continue
            begin, end = regions[(cols["col_list0"][e], o)]
            assert end - begin == sum(counts) and begin % 8 == 0
            starts = begin + np.concatenate(([0], np.cumsum(counts)))
            bounds = [int(starts[min(g, len(lists))]) for g in range(0, len(lists) + ROWS, ROWS)]
            out[(e, o)] = (bounds, end)
    assert len(out) == len(regions)
    return out


def _tiles(pieces, begin, end):
    """Non-empty pieces [b0, b1) are disjoint and their union is [begin, end)."""
    at = begin
    for b0, b1 in sorted(p for p in pieces if p[1] > p[0]):
        if b0 != at:
            return False
        at = b1
    return at == end


@pytest.mark.parametrize("name", gen.PROBE_CASES)
def test_every_pair_of_a_stream_is_counted_once(plans, name):
    doc = plans[name]
    streams = _streams(name, doc)
    assert streams
    thin, fat = doc["probe"]["items"], doc["probe"]["fat_items"]
    seen_thin = seen_fat = 0
    for (e, o), (bounds, end) in streams.items():
        begin = bounds[0]
        # ---- one group per item ----
        mine = [it for it in thin if it[7] == e and begin <= it[0] < end]
        seen_thin += len(mine)
        with_elements = {g * ROWS for g in range(len(bounds) - 1) if bounds[g + 1] > bounds[g]}
        assert {it[6] for it in mine} == with_elements   # a group without elements has no item
        for a0 in with_elements:
            g = a0 // ROWS
            items = [it for it in mine if it[6] == a0]
            assert all((it[0], it[1]) == (bounds[g], bounds[g + 1]) for it in items)
            near = [it for it in items if (it[2], it[3]) == (it[0], it[1])]
            assert len(near) == 1 and all(it[2] == it[3] for it in items if it is not near[0])
            assert _tiles([(it[4], it[5]) for it in items], bounds[g + 1], end)
        # ---- bundles of four groups ----
        mine = [it for it in fat if it[8] == e and begin <= it[0] < end]
        seen_fat += len(mine)
        n_groups = len(bounds) - 1
        for g0 in range(0, n_groups, BUNDLE):
            at = [bounds[min(g0 + k, n_groups)] for k in range(BUNDLE + 1)]
            items = [it for it in mine if it[0] == at[0] and it[4] > it[0]] if at[4] > at[0] else []
            if at[4] == at[0]:
                continue
            assert items and all(it[:5] == at for it in items)   # at[] = the thin list's group bounds
            assert sum(it[7] for it in items) == 1
            assert _tiles([(it[5], it[6]) for it in items], at[4], end)
        bundles_with_elements = sum(1 for g0 in range(0, n_groups, BUNDLE) if bounds[min(g0 + BUNDLE, n_groups)] > bounds[g0])
        assert len({it[0] for it in mine}) == bundles_with_elements
    assert seen_thin == len(thin) and seen_fat == len(fat)   # no item outside the streams


def test_case_e_has_streams_of_several_chunks(plans):
    thin = plans["E"]["probe"]["items"]
    per_group = {}
    for it in thin:
        per_group[(it[0], it[6])] = per_group.get((it[0], it[6]), 0) + 1
    assert max(per_group.values()) >= 2


@pytest.mark.parametrize("name", gen.PROBE_CASES)
def test_the_ranks_of_a_world_partition_the_launch(plans, name):
    doc = plans[name]
    launch = doc["launch"]
    n_cols = len(doc["columns"]["col_probe"])
    for bundle, all_items in ((1, doc["probe"]["items"]), (BUNDLE, doc["probe"]["fat_items"])):
        for mask in ("all", "alt"):
            use, seen = [], 0
            for probe in doc["columns"]["col_probe"]:
                use.append(1 if probe and (mask == "all" or seen % 2 == 0) else 0)
                seen += probe
            filtered = [it[:-1] for it in all_items if use[it[-1]]]
            whole = launch[f"b{bundle}/w1/r0/{mask}"]
            assert whole["records"] == filtered and whole["counts"][:2] == [len(filtered), sum(use)]
            assert len(use) == n_cols
            for world in (2, 3):
                ranks = [launch[f"b{bundle}/w{world}/r{r}/{mask}"] for r in range(world)]
                assert all(r["records"] == filtered for r in ranks)   # every rank holds the list, item k belongs to rank k % world
                assert [r["counts"][0] for r in ranks] == [len(filtered[r::world]) for r in range(world)]
                assert sum(r["counts"][2] for r in ranks) == whole["counts"][2]


@pytest.mark.parametrize("name", ("C", "F"))
def test_the_segments_cover_every_row_pair_of_a_column_once(plans, name):
    doc = plans[name]
    cols = list(zip(doc["columns"]["cols_r0"], doc["columns"]["cols_r1"]))
    want = sum((r1 - r0) * (r1 - r0 - 1) // 2 for r0, r1 in cols)
    for seg_len in (1, 256):
        for world in (1, 3):
            pairs = 0
            for rank in range(world):
                plan = doc["segments"][f"len{seg_len}/w{world}/r{rank}"]
                assert plan["row_sum"] == [sum(j1 - j0 for _, _, j0, j1 in plan["segs"])]
                for a0, a_end, j0, j1 in plan["segs"]:
                    n_a = a_end - a0
                    pairs += n_a * (n_a - 1) // 2 if j0 == a0 else n_a * (j1 - j0)
            assert pairs == want


def _dense_segments(n_rows, seg_len, rank, world, block=128):
    """The loop that stood in storm_hip.hip's ensure_segments (the dense matrix's own planner), transcribed: full segments
    first (A-block major), the short diagonal segments last; a shard takes every world-th entry of each list."""
    full, diag = [], []
    for a0 in range(0, n_rows, block):
        a_end = min(a0 + block, n_rows)
        if a_end - a0 > 1:
            diag.append([a0, a_end, a0, a_end])
        for j in range(a0 + block, n_rows, seg_len):
            full.append([a0, a_end, j, min(j + seg_len, n_rows)])
    mine = full[rank::world] + diag[rank::world]
    return mine, sum(j1 - j0 for _, _, j0, j1 in mine)


def test_the_dense_matrix_is_the_single_column_from_row_0(tmp_path):
    """plan_sparse_segments over the column {0, n} is what the dense container's own loop planned."""
    import subprocess
    exe = tmp_path / "arena_plan"
    build = gen.build_driver(exe)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe), "--single-column"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-3000:]
    doc = json.loads(run.stdout)
    cases = [(n, seg_len, world, rank) for n in (1, 2, 128, 129, 600) for seg_len in (256, 100) for world in (1, 3)
             for rank in range(world)]
    assert len(doc) == len(cases)
    for n, seg_len, world, rank in cases:
        segs, row_sum = _dense_segments(n, seg_len, rank, world)
        assert doc[f"n{n}/len{seg_len}/w{world}/r{rank}"] == {"segs": segs, "row_sum": [row_sum]}, (n, seg_len, world, rank)
    assert doc["n1/len256/w1/r0"]["segs"] == [] and len(doc["n600/len100/w1/r0"]["segs"]) == 13 + 5


def test_planners_under_asan_ubsan(tmp_path):
    exe = tmp_path / "arena_plan_sanitized"
    build = gen.build_driver(exe, sanitize=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan not installed")
    assert build.returncode == 0, build.stderr
    cases = {name: gen.case_text(gen.case_rows(name)) for name in gen.VALID_CASES}
    cases.update({"H_" + name: text for name, (text, _) in gen.invalid_cases().items()})
    for name, text in cases.items():
        doc, stderr = gen.run_case(exe, text, tmp_path, name)
        assert "Sanitizer" not in stderr and "runtime error" not in stderr, (name, stderr[-3000:])
        for section, digest in gen.digests_of(doc).items():
            assert digest == GOLDEN[f"{name}/{section}"], (name, section)
