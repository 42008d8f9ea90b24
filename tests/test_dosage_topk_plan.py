"""The row panels of the dosage top-k calls without a device: how many rows of `a` have their integer sums on the device at a
time (storm_hip_plan.cpp: dosage_topk_plane_words, dosage_topk_panel_rows), run by tests/dosage_topk_plan/driver.cpp.

The rule, as storm_hip.h states it: panel_rows as the caller gives it (a multiple of 256), or for 0 the largest multiple of
256 whose planes hold at most 256 MiB, at least 256; never more than the rows there are, rounded up to 256. A panel row holds
1 word per row of b (up to the next multiple of 4) in the plain forms and `ld + 2 ld + (2 rows128_b + ld)` words — about 6
per row of b — in the pairwise-complete forms."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCES = [os.path.join(HERE, "dosage_topk_plan", "driver.cpp"), os.path.join(ROOT, "stormbitmaps_amd", "csrc", "storm_hip_plan.cpp")]
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "stormbitmaps_amd", "csrc")]
PANEL_BYTES = 256 << 20

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def up(x, m):
    return (x + m - 1) // m * m


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dosage_topk_plan")
    exe = tmp / "driver"
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                            *INCLUDES, *SOURCES, "-o", str(exe)], capture_output=True, text=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        build = subprocess.run(["g++", "-std=c++17", "-Wall", "-O2", *INCLUDES, *SOURCES, "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    rng = np.random.default_rng(256)
    rows = [1, 2, 255, 256, 257, 511, 512, 513, 600, 32768, 65408, 100000, 1 << 20, 1 << 24, (1 << 31) - 1]
    cases = [(p, na, nb, c) for p in (0, 256, 512, 1 << 20) for na in rows for nb in [0] + rows for c in (0, 1)]
    cases += [(int(256 * rng.integers(0, 40)), int(rng.integers(1, 1 << 22)), int(rng.integers(0, 1 << 22)), int(rng.integers(0, 2)))
              for _ in range(2000)]
    path = tmp / "cases.txt"
    path.write_text(f"{len(cases)}\n" + "\n".join(" ".join(map(str, c)) for c in cases) + "\n")
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    out = json.loads(run.stdout)
    assert out["panel_bytes"] == PANEL_BYTES and len(out["cases"]) == len(cases)
    return [(c, tuple(a)) for c, a in zip(cases, out["cases"])]


def test_words_of_a_panel_row(answers):
    for (_, _, nb, complete), (words, _) in answers:
        ld = up(nb, 4)
        assert words == (ld + 2 * ld + 2 * up(nb, 128) + ld if complete else ld), (nb, complete)


def test_a_multiple_of_256_at_least_256_and_no_more_than_the_rows(answers):
    for (panel_rows, na, nb, complete), (_, rows) in answers:
        assert rows % 256 == 0 and rows >= 256, (panel_rows, na, nb, complete, rows)
        assert rows <= up(na, 256), (panel_rows, na, nb, complete, rows)
        if panel_rows:
            assert rows == min(panel_rows, up(na, 256)), (panel_rows, na, nb, complete, rows)


def test_the_planes_hold_at_most_256_mib_wherever_256_rows_allow_it(answers):
    seen_floor = seen_budget = 0
    for (panel_rows, na, nb, complete), (words, rows) in answers:
        if panel_rows:
            continue
        words = max(words, 1)                                               # (an empty b: counted as one word per row)
        if 256 * words * 4 > PANEL_BYTES:                                   # 256 rows alone are over the budget: the floor
            assert rows == 256, (na, nb, complete, rows)
            seen_floor += 1
            continue
        assert rows * words * 4 <= PANEL_BYTES, (na, nb, complete, rows)
        # the largest such multiple of 256, unless the rows end first
        assert rows == up(na, 256) or (rows + 256) * words * 4 > PANEL_BYTES, (na, nb, complete, rows)
        seen_budget += rows < up(na, 256)
    assert seen_floor >= 10 and seen_budget >= 10


def test_the_plain_form_allows_about_six_times_the_rows(answers):
    by_key = {c: a for c, a in answers}
    checked = 0
    for (panel_rows, na, nb, complete), (_, rows) in answers:
        if panel_rows or complete or (0, na, nb, 1) not in by_key:
            continue
        rows_c = by_key[(0, na, nb, 1)][1]
        # not where the rows cap either, nor below 20 panels of 256 (the rounding down is 5 % there), nor below 512 rows of b:
        # the words are 6 ld + 2 (rows128_b - ld) against ld, 6 to 6.5 from 512 rows on, and the rounding adds up to 5 %
        if rows == up(na, 256) or rows_c < 20 * 256 or nb < 512:
            continue
        assert 6.0 * 0.95 <= rows / rows_c <= 6.5 * 1.05, (na, nb, rows, rows_c)
        checked += 1
    assert checked >= 5
