"""The schedule of strip16_rows_kernel's diagonal phase without a device (storm_hip_plan.h: strip_rows_block,
strip_rows_role, strip_rows_diag_begin / _end), printed by tests/strip_rows_diag/driver.cpp.

The A tile's 8 blocks of 64 rows among themselves: block b against every later block whole and against itself as a
triangle. Wave w of 4 keeps two blocks (its halves) and walks the blocks d of [begin, end) upwards; at d a half skips,
multiplies its own triangle or multiplies whole. Checked here from the driver's table alone:
  * over the 4 waves every unordered pair of the 8 blocks is multiplied exactly once, inside the steps the wave walks;
  * every block is owned by exactly one half, and its triangle is multiplied exactly once;
  * every wave issues the same number of MFMAs (16 per whole product, 10 per triangle);
  * no half is multiplied before its own block — the in-place mask of the kernel needs the own block to be the first
    thing a half's accumulators see — and the low half's own block comes in front of the high half's (the kernel's four
    runs: low own | low whole | low whole + high own | both whole);
  * the same driver under AddressSanitizer + UBSan (a stand-alone program) prints the same table and is clean."""
import json
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCE = os.path.join(HERE, "strip_rows_diag", "driver.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "stormbitmaps_amd", "csrc")]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def build_driver(exe, sanitize=False):
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] \
        if sanitize else ["-O2"]
    return subprocess.run(["g++", "-std=c++17", "-Wall", *flags, *INCLUDES, SOURCE, "-o", str(exe)],
                          capture_output=True, text=True)


def run_driver(exe):
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-3000:])
    return json.loads(run.stdout), run.stderr


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = tmp_path_factory.mktemp("strip_rows_diag") / "schedule"
    build = build_driver(exe)
    assert build.returncode == 0, build.stderr
    return run_driver(exe)[0]


def test_the_tile_is_8_blocks_among_4_waves(table):
    assert (table["blocks"], table["waves"]) == (8, 4) and len(table["wave"]) == 4
    assert len({table["skip"], table["own"], table["whole"]}) == 3
    assert table["mfmas"][table["skip"]] == 0 and table["mfmas"][table["own"]] == 10 and table["mfmas"][table["whole"]] == 16
    for w in table["wave"]:
        assert len(w["role"]) == 2 and all(len(r) == 8 for r in w["role"])
        assert 0 <= w["begin"] < w["end"] <= 8


def test_every_block_is_owned_once(table):
    owned = [b for w in table["wave"] for b in w["block"]]
    assert sorted(owned) == list(range(8))
    triangles = []
    for w in table["wave"]:
        for half in range(2):
            at = [d for d in range(8) if w["role"][half][d] == table["own"]]
            assert at == [w["block"][half]]                      # a half's own step is the step of its block
            assert w["begin"] <= at[0] < w["end"]                # ... and the wave walks it
            triangles.append(at[0])
    assert sorted(triangles) == list(range(8))


def test_every_pair_of_blocks_is_multiplied_exactly_once(table):
    count = {}
    for w in table["wave"]:
        for half in range(2):
            for d in range(8):
                if w["role"][half][d] == table["whole"]:
                    assert w["begin"] <= d < w["end"], (w, half, d)   # not outside the steps the wave walks
                    assert d != w["block"][half]
                    pair = frozenset((w["block"][half], d))
                    count[pair] = count.get(pair, 0) + 1
    assert len(count) == 28 and set(count.values()) == {1}
    assert set(count) == {frozenset((a, b)) for a in range(8) for b in range(a + 1, 8)}


def test_a_block_is_multiplied_against_later_blocks_only(table):
    """The strict upper triangle: A block b meets B block d whole only for d > b (rows i < j), so the pair's count lands
    once and on the side the mask of the own block expects."""
    for w in table["wave"]:
        for half in range(2):
            for d in range(8):
                if w["role"][half][d] == table["whole"]:
                    assert d > w["block"][half]


def test_the_waves_issue_the_same_number_of_mfmas(table):
    per_wave = [sum(table["mfmas"][w["role"][half][d]] for half in range(2) for d in range(w["begin"], w["end"]))
                for w in table["wave"]]
    assert per_wave == [7 * 16 + 2 * 10] * 4
    # nothing is lost in front of `begin` or behind `end`
    for w in table["wave"]:
        outside = [d for d in range(8) if not w["begin"] <= d < w["end"]]
        assert all(w["role"][half][d] == table["skip"] for half in range(2) for d in outside)
        # and no step the wave walks is empty
        assert all(any(w["role"][half][d] != table["skip"] for half in range(2)) for d in range(w["begin"], w["end"]))


def test_no_half_is_multiplied_before_its_own_block(table):
    order = {table["skip"]: 0, table["own"]: 1, table["whole"]: 2}
    for w in table["wave"]:
        for half in range(2):
            seq = [order[r] for r in w["role"][half]]
            assert seq == sorted(seq) and seq.count(1) == 1, (w, half)   # skip*, own, whole*
        assert w["block"][0] < w["block"][1]
        assert w["begin"] == w["block"][0]
        # the high half has seen nothing when its own block comes: the steps in front of it are the low half's alone
        assert all(w["role"][1][d] == table["skip"] for d in range(w["block"][1]))


def test_schedule_under_asan_ubsan(table, tmp_path):
    exe = tmp_path / "schedule_sanitized"
    build = build_driver(exe, sanitize=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan not installed")
    assert build.returncode == 0, build.stderr
    got, stderr = run_driver(exe)
    assert "Sanitizer" not in stderr and "runtime error" not in stderr, stderr[-3000:]
    assert got == table
