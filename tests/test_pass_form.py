"""Which kernel an all-pairs pass runs, on which strip form: choose_pass and the StripForm table (storm_hip_plan.*), asked
through tests/pass_form/driver.cpp without a device, against the same rules written down in tests/_pass_forms.py.

  * every strip form's numbers — A tile, waves, threads, slices for a width, the report's words per slice, XCD group, the
    fold's bound, what the k2_*_used options report, the strip_plan form — against the table;
  * the choice over the full product of the selecting options, both builds, both shard counts, the three callers and shapes
    at which every predicate flips (the 256- and 512-row padding in fresh and in resized allocations, 2048 rows, 1024 words,
    the 32-bit pitch limit, the pool's rows);
  * the same driver under AddressSanitizer + UBSan (a stand-alone program) answers the same and is clean;
  * dist.strip_plan's forms 0 / 1 / 2 still plan over the table's slices and tiles (tests/test_plan_golden.py and
    tests/test_strip_rows_plan.py pin the lists themselves)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from stormbitmaps_amd import dist
from tests import _pass_forms as pf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SOURCES = [os.path.join(HERE, "pass_form", "driver.cpp"), os.path.join(ROOT, "stormbitmaps_amd", "csrc", "storm_hip_plan.cpp")]
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "stormbitmaps_amd", "csrc")]

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

# the driver's numbers (the order of the enums in storm_hip_plan.h)
FORM_NUMBER = {"fp4": 0, "bits": 1, "bits_wide": 2, "rows": 3}
FAMILY_NUMBER = {"popcount": 0, "fp4_tiles": 1, "fp4_strips": 2, "fp4_strips_wide": 3, "k2q": 4, "k2b": 5, "tools_stripbits": 6,
                 "tools_bitwave": 7}
CALLERS = ("dense", "upload", "pool")
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 8192)

OPTIONS = [pf.Options(variant, operands, rows, ring, shape, persistent, debug, tools)
           for variant in (-1, 0, 2, 3, 4, 5) for operands in range(7) for rows in (0, 64, 128)
           for ring, shape in ((4, 16), (3, 16), (4, 32)) for persistent in (0, 1) for debug in (0, 1) for tools in (False, True)]
SHARDS = (1, 2)


def _dense_shapes():
    rows = [(n, pf.allocation(n)) for n in (0, 1, 2, 256, 257, 512, 513, 2047, 2048, 2049, 2305)] + [(2064, 2560), (2049, 2560)]
    out = [pf.Shape(n, pad, w, pf.stride(w)) for n, pad in rows for w in (1, 8, 1023, 1024)]
    # rows of 2^26 bytes: a B stage of 64 of them is 2^32 bytes — and the last pitch below that
    out += [pf.Shape(2048, 2048, 1 << 23, 1 << 23), pf.Shape(2048, 2048, (1 << 23) - 64, (1 << 23) - 64)]
    return out


def _pool_shapes():
    # the pool's rows: rows_dst at pool_rows_ready + 512 and one row block above it; a widest column on either side of 64
    return [pf.Shape(rows_dst=ready + over, pool_rows_ready=ready, widest=widest)
            for ready in (512, 4096) for over in (0, 512, 1024) for widest in (63, 64)]


DENSE_SHAPES, POOL_SHAPES = _dense_shapes(), _pool_shapes()


def build_driver(exe, sanitize=False):
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] \
        if sanitize else ["-O2"]
    return subprocess.run(["g++", "-std=c++17", "-Wall", *flags, *INCLUDES, *SOURCES, "-o", str(exe)], capture_output=True, text=True)


def ask(exe, lines):
    run = subprocess.run([str(exe)], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr[-3000:])
    return run.stdout.split("\n")[:-1], run.stderr


def _shape_lines():
    return ["s d %d %d %d %d 0 0 0" % s[:4] for s in DENSE_SHAPES] + \
           ["s p 0 0 0 0 %d %d %d" % (s.rows_dst, s.pool_rows_ready, s.widest) for s in POOL_SHAPES]


def _queries():
    """(the driver's query, caller, options, shard count), in the order asked"""
    return [("q %d %d %d %d %d %d %d %d %d %d" % (CALLERS.index(caller), *o[:7], int(o.tools), shards), caller, o, shards)
            for caller in CALLERS for o in OPTIONS for shards in SHARDS]


def _answer(c):
    strip_mode = {"fp4_strips": 1, "fp4_strips_wide": 2}.get(c.family, 0)
    return "%d %d %d %d %d %d" % (FAMILY_NUMBER[c.family], FORM_NUMBER[c.form] if c.form else -1, c.variant_used, c.operands_used or 0,
                                  strip_mode, int(c.in_panels))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("pass_form") / "pass_form"
    build = build_driver(exe)
    assert build.returncode == 0, build.stderr
    return exe


@pytest.fixture(scope="module")
def answers(driver):
    """the driver's lines for the whole product, asked once"""
    got, _ = ask(driver, _shape_lines() + [q for q, _, _, _ in _queries()])
    return got


def test_every_form_has_the_tables_numbers(driver):
    got, _ = ask(driver, ["f %d %s" % (FORM_NUMBER[name], " ".join(str(w) for w in WIDTHS)) for name in pf.FORMS] +
                 ["p %d" % form for form in (-1, 0, 1, 2, 3)])
    for line, (name, f) in zip(got, pf.FORMS.items()):
        a_tile, waves, threads, slice_words, xcd_group, wave_sum_max, operands, rows, plan, *slices = (int(x) for x in line.split())
        assert (a_tile, waves, threads, xcd_group, operands) == (f.a_tile, f.waves, f.threads, f.xcd_group, f.operands), name
        assert threads == 64 * waves and plan == (-1 if f.plan is None else f.plan), name
        assert slices == [f.slices(w) for w in WIDTHS], name
        if f.slice_words is not None:    # (the FP4 strips report by words and never fold inline)
            assert (slice_words, wave_sum_max, rows) == (f.slice_words, f.wave_sum_max, f.rows), name
    assert [int(x) for x in got[len(pf.FORMS):]] == [-1, FORM_NUMBER["fp4"], FORM_NUMBER["bits"], FORM_NUMBER["rows"], -1]
    # the sparse pool's rows are 1024 words wide: 256 slices of the bits form
    assert pf.FORMS["bits"].slices(1024) == 256


def test_the_choice_over_the_full_product(answers):
    at, wrong, seen, text = 0, [], set(), {}
    shapes = {(caller, shards): [s._replace(shard_count=shards) for s in (POOL_SHAPES if caller == "pool" else DENSE_SHAPES)]
              for caller in CALLERS for shards in SHARDS}
    for _, caller, o, shards in _queries():
        for s in shapes[caller, shards]:
            c = pf.choose(caller, o, s)
            seen.add((caller, c.family, c.form, c.in_panels))
            want = text.get(c) or text.setdefault(c, _answer(c))
            if answers[at] != want and len(wrong) < 10:
                wrong.append((caller, o, s, answers[at], want))
            at += 1
    assert at == len(answers) and not wrong, wrong
    # every family and form is reached by the product, from every caller that can reach it
    dense = {("popcount", None), ("fp4_tiles", None), ("fp4_strips", None), ("fp4_strips_wide", None), ("k2q", None),
             ("tools_stripbits", None), ("tools_bitwave", None), ("k2b", "bits"), ("k2b", "bits_wide"), ("k2b", "rows")}
    assert {(f, form) for caller, f, form, _ in seen if caller == "dense"} == dense
    assert {(f, form) for caller, f, form, panels in seen if caller == "upload" and not panels} == dense
    assert {(f, form) for caller, f, form, panels in seen if panels} == {("k2b", "bits")}
    assert {(f, form) for caller, f, form, _ in seen if caller == "pool"} == \
        {("popcount", None), ("fp4_tiles", None), ("fp4_strips", None), ("fp4_strips_wide", None), ("k2b", "bits")}


def test_every_predicate_flips_inside_the_product():
    """the shapes are worth their place: each rule's two sides are both taken, everything else equal"""
    o = pf.Options()
    form = lambda n, pad, w=1024, shards=1, **kw: pf.choose("dense", o._replace(**kw), pf.Shape(n, pad, w, pf.stride(w), shards)).form
    assert form(2048, 2048) == "rows" and form(2047, 2048) == "bits" and form(2048, 2048, 1023) == "bits"
    assert form(2048, 2048, shards=2) == "bits" and form(2048, 2048, k2_strip_rows=64) == "bits"
    assert form(2049, 2304) == "bits" and form(2049, 2560) == "rows" and form(2064, 2560) == "rows"
    assert form(513, 768, 8, k2_strip_rows=128) == "bits" and form(512, 512, 8, k2_strip_rows=128) == "rows"
    assert form(512, 512, 8, k2_strip_operands=6) == "bits_wide" and form(513, 768, 8, k2_strip_operands=6) == "bits"
    assert form(512, 512, 8, k2_strip_operands=6, k2_strip_rows=128) == "bits_wide"
    family = lambda s, **kw: pf.choose("dense", o._replace(**kw), s).family
    assert family(pf.Shape(257, 256, 8, 64)) == "fp4_strips" and family(pf.Shape(256, 256, 8, 64)) == "k2b"
    assert family(pf.Shape(2048, 2048, 1 << 23, 1 << 23)) == "fp4_strips"
    assert family(pf.Shape(2048, 2048, (1 << 23) - 64, (1 << 23) - 64)) == "k2b"
    assert family(pf.Shape(2, 256), k2_ring=3) == "fp4_strips" and family(pf.Shape(2, 256), k2_ring=3, k2_strip_operands=5) == "k2b"
    panels = lambda n, **kw: pf.choose("upload", o._replace(**kw), pf.Shape(n, pf.allocation(n), 8, 64)).in_panels
    assert panels(2048) and not panels(2047) and panels(2048, k2_strip_operands=6, k2_strip_rows=128)
    assert not panels(2048, variant=3) and not panels(2048, k2_strip_operands=2)
    pool = lambda over, **kw: pf.choose("pool", o._replace(**kw), pf.Shape(rows_dst=512 + over, pool_rows_ready=512, widest=64))
    assert pool(512).form == "bits" and pool(1024).family == "fp4_strips" and pool(512, k2_strip_operands=6).form == "bits"
    assert pool(512, k2_strip_rows=128).form == "bits" and pool(512, k2_strip_operands=4).family == "fp4_strips"


def test_the_driver_under_asan_ubsan(driver, answers, tmp_path):
    exe = tmp_path / "pass_form_sanitized"
    build = build_driver(exe, sanitize=True)
    if build.returncode != 0 and "asan" in build.stderr.lower() and "cannot find" in build.stderr.lower():
        pytest.skip("libasan not installed")
    assert build.returncode == 0, build.stderr
    got, stderr = ask(exe, _shape_lines() + [q for q, _, _, _ in _queries()])
    assert "Sanitizer" not in stderr and "runtime error" not in stderr, stderr[-3000:]
    assert got == answers


@pytest.mark.parametrize("form,name", ((0, "fp4"), (1, "bits"), (2, "rows")))
def test_strip_plan_plans_over_the_tables_slices_and_tiles(form, name):
    f = pf.FORMS[name]
    for rows, words in ((600, 5), (1100, 9), (2048, 33)):
        items = dist.strip_plan(rows, words, 0, 1, form)
        assert set(np.unique(items[:, 4]).tolist()) == set(range(f.slices(words))), (form, rows, words)
        assert (items[:, 0] % f.a_tile == 0).all() and len(np.unique(items[:, 0])) == (rows + f.a_tile - 1) // f.a_tile
        diag = items[items[:, 1] == 1]
        assert len(diag) == f.slices(words) * ((rows + f.a_tile - 1) // f.a_tile)
