"""What strip16_rows_kernel skips behind the matrix's last row, without a device (storm_hip_plan.h: strip_rows_real_frags,
strip_rows_real_blocks, strip_rows_top_trimmed, strip_rows_item_mfmas), answered by tests/strip_rows_trim/driver.cpp.

The kernel is told where the rows end (n_rows; 0xFFFFFFFF = nothing is trimmed). The top B block of a run that has rows in
only 1 or 2 of its four 16-row fragments is multiplied last and only in those fragments; the diagonal phase of a tile stops
at its last 64-row block that holds a row. Checked here:
  * the fragment and block counts against a direct numpy count of "holds a row < n_rows";
  * an item's MFMAs against counts made here from the rows alone (a stage = 4 waves x 4 fragments x 8 A fragments, a
    diagonal of nb blocks = 10 per triangle + 16 per pair of blocks), over a grid of (n_rows, tile, diag, j0, j1);
  * the headline list dist.strip_plan(10000, 1024, 0, 1, 2) adds up to 197 824 MFMAs per slice untrimmed, 196 000 with the
    top block trimmed and 195 682 with the diagonal phase trimmed as well — the kernel's SQ_VALU_MFMA_BUSY_CYCLES is 16 x;
  * the same driver under AddressSanitizer + UBSan (a stand-alone program) answers the same and is clean."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from stormbitmaps_amd import dist

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCE = os.path.join(HERE, "strip_rows_trim", "driver.cpp")
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "stormbitmaps_amd", "csrc")]
NO_TRIM = 0xFFFFFFFF

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

N_ROWS = (1, 15, 16, 17, 32, 33, 48, 49, 63, 64, 65, 500, 512, 513, 528, 529, 544, 545, 560, 561, 575, 576, 577, 1000, 1024,
          1040, 1296, 2064, 10000, NO_TRIM)


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
    return [tuple(int(v) for v in ln.split()) for ln in lines], run.stderr


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("strip_rows_trim") / "trim"
    build = build_driver(exe)
    assert build.returncode == 0, build.stderr
    return exe


def _frags(n_rows, blk):
    rows = 64 * blk + np.arange(64).reshape(4, 16)
    return int((rows < n_rows).any(axis=1).sum())


def _blocks(n_rows, a_row0):
    rows = a_row0 + np.arange(512).reshape(8, 64)
    return int((rows < n_rows).any(axis=1).sum())


def _item_counts(n_rows, a_row0, diag, j0, j1):
    """(untrimmed, top block alone, top block and diagonal, top block trimmed?) from the rows alone."""
    T = j1 - j0
    F = _frags(n_rows, j1 - 1) if T else 4
    flip = T > 0 and F in (1, 2)
    run = 128 * (T - 1) + 32 * F if flip else 128 * T
    nb = _blocks(n_rows, a_row0)
    return (128 * T + 528 * diag, run + 528 * diag, run + diag * (10 * nb + 16 * nb * (nb - 1) // 2), int(flip))


def _grid():
    grid = []
    for n_rows in N_ROWS:
        top = min((n_rows + 63) // 64, 1 << 20)   # blocks that hold a row
        for j1 in sorted({max(top - 1, 0), top, top + 1, top + 9}):
            for run in (0, 1, 2, 3, 4, 7):
                if run > j1:
                    continue
                last_tile = (n_rows - 1) // 512 * 512
                for a_row0 in sorted({0, last_tile, min(last_tile + 512, 0xFFFFFE00)}):   # (a_row0 is a uint32)
                    for diag in (0, 1):
                        grid.append((n_rows, a_row0, diag, j1 - run, j1))
    return grid


def test_fragments_and_blocks_that_hold_a_row(driver):
    frag_q = [(n, blk) for n in N_ROWS for blk in sorted({0, 1, max((min(n, 1 << 26) + 63) // 64 - 1, 0), (min(n, 1 << 26) + 63) // 64, 8, 157})]
    got, _ = ask(driver, [f"f {n} {blk}" for n, blk in frag_q])
    assert [g[0] for g in got] == [_frags(n, blk) for n, blk in frag_q]
    tile_q = [(n, a) for n in N_ROWS for a in sorted({0, 512, 1024, (min(n, 1 << 30) - 1) // 512 * 512, 9728, 10240})] + \
        [(a + 64 * k + one, a) for a in (0, 9728) for k in range(9) for one in (0, 1)]   # the matrix ends at a block's edge, one row on
    got, _ = ask(driver, [f"b {n} {a}" for n, a in tile_q])
    assert [g[0] for g in got] == [_blocks(n, a) for n, a in tile_q]
    # every value of both ranges is reached
    assert {_frags(n, blk) for n, blk in frag_q} == {0, 1, 2, 3, 4} and {_blocks(n, a) for n, a in tile_q} == set(range(9))


def test_an_items_mfmas_over_a_grid(driver):
    grid = _grid()
    got, _ = ask(driver, ["m %d %d %d %d %d" % g for g in grid])
    want = [_item_counts(*g) for g in grid]
    wrong = [(g, a, b) for g, a, b in zip(grid, got, want) if a != b]
    assert not wrong, wrong[:5]
    assert any(w[3] for w in want) and any(w[1] != w[2] for w in want) and any(w[0] == w[2] for w in want)
    # a trimmed item saves 2 or 3 fragments of its top block, never more
    assert {w[0] - w[1] for w in want} == {0, 64, 96}


def test_the_headline_list_adds_up(driver):
    items = dist.strip_plan(10000, 1024, 0, 1, 2)
    assert len(items) == 14520
    queries = ["m 10000 %d %d %d %d" % (a_row0, diag, j0, j1) for a_row0, diag, j0, j1, _ in items.tolist()]
    got, _ = ask(driver, queries)
    off, top, both, _ = (sum(col) for col in zip(*got))
    assert off == 197824 * 512
    assert top == 196000 * 512
    assert both == 195682 * 512
    # ... and told nothing, the kernel's rule is the untrimmed count
    got, _ = ask(driver, [q.replace("m 10000 ", "m %d " % NO_TRIM) for q in queries])
    assert all(g[0] == g[1] == g[2] and g[3] == 0 for g in got)


def test_trim_under_asan_ubsan(driver, tmp_path):
    exe = tmp_path / "trim_sanitized"
    build = build_driver(exe, sanitize=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan not installed")
    assert build.returncode == 0, build.stderr
    queries = ["m %d %d %d %d %d" % g for g in _grid()] + [f"f {n} {blk}" for n in N_ROWS for blk in (0, 8, 156, (1 << 26) - 1)] + \
        [f"b {n} {a}" for n in N_ROWS for a in (0, 9728, 0xFFFFFE00)]
    got, stderr = ask(exe, queries)
    assert "Sanitizer" not in stderr and "runtime error" not in stderr, stderr[-3000:]
    assert got == ask(driver, queries)[0]
