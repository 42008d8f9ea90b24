"""What an all-pairs pass reports after a call against the table of tests/_pass_forms.py (the rules of choose_pass,
storm_hip_plan.cpp, written down a second time), through public calls alone: set_option, pairw, pairw_upload, get_option,
last_pass_report, last_launch_info, column_identity and dist.strip_plan. Nothing here reads the library's internals, so the
file passes unchanged against any build that keeps the rules (STORM_HIP_LIB).

Dense: nine shapes at which the rules' predicates flip (the 256- and 512-row padding in fresh and in resized allocations,
2048 rows, 1024 words) x variant x k2_strip_operands x k2_strip_rows x worlds 1 and 2. Every case: the total equals the
column identity (summed over a world's ranks); variant_used and k2_operands_used are the table's; k2_strip_rows_used is the
table's where a K2b launch ran and what it was where none did; the pass report names the table's kernel; for the strip forms
that dist.strip_plan plans, the launch's item count is the length of that plan. pairw_upload at 2047 and 2048 rows: the same,
and panels in the launch info exactly where the table says "in panels". One small sparse container (two bitmap columns and a
list column): K2b on the pool rows for k2_strip_operands 0 and 6, the FP4 strips for 4."""
import ctypes as C
import functools

import numpy as np
import pytest

import stormbitmaps_amd as sb
from stormbitmaps_amd import dist
from tests import _pass_forms as pf
from tests.conftest import shipped
from tests.test_gpu_stage_edges import NONE, Desc, _p

pytestmark = pytest.mark.gpu

# (rows, rows the matrix is created with, words): None = created as it is
SHAPES = ((2, None, 1), (257, None, 8), (513, None, 8), (2048, None, 1024), (2047, None, 1024), (2048, None, 1023),
          (2049, None, 1024), (2049, 2560, 1024), (2064, 2560, 1024))
VARIANTS, OPERANDS, STRIP_ROWS = (-1, 2, 3, 4), (0, 2, 4, 5, 6), (0, 64, 128)


@pytest.fixture(scope="module")
def ctx():
    c = sb.HipContext(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _rows(n_rows, n_words):
    mat = np.random.default_rng([n_rows, n_words]).integers(0, 1 << 64, size=(n_rows, n_words), dtype=np.uint64)
    mat.setflags(write=False)
    return mat


@functools.lru_cache(maxsize=None)
def _plan_len(n_rows, n_words, rank, world, form, n_cus):
    # tail_run 0: no tail option is set on the context
    return len(dist.strip_plan(n_rows, n_words, rank, world, form, tail_run=0, n_cus=n_cus))


def _matrix(ctx, n_rows, created, n_words):
    m = ctx.matrix(created or n_rows, n_words)
    if created:
        m.resize(n_rows)
    m.upload(_rows(n_rows, n_words))
    return m


def _options(ctx):
    tools = ctx.get_option("probes_build") == 1
    return [pf.Options(variant, operands, rows, tools=tools) for variant in shipped(ctx, "variant", VARIANTS)
            for operands in shipped(ctx, "k2_strip_operands", OPERANDS) for rows in STRIP_ROWS]


def _set(ctx, o):
    for key in ("variant", "k2_strip_operands", "k2_strip_rows"):
        ctx.set_option(key, getattr(o, key))


def _check_report(ctx, choice, rows_used_before, n_rows, n_words, rank, world, case):
    """what the context says after a pass that `choice` describes; returns the kernels the pass report names"""
    assert ctx.get_option("variant_used") == choice.variant_used, case
    if choice.operands_used is not None:
        assert ctx.get_option("k2_operands_used") == choice.operands_used, case
    rows_used = ctx.get_option("k2_strip_rows_used")
    assert rows_used == (pf.FORMS[choice.form].rows if choice.family == "k2b" else rows_used_before), case
    form = pf.FORMS[choice.form] if choice.form else pf.FORMS["fp4"] if choice.family == "fp4_strips" else None
    if form is not None and form.plan is not None and not choice.in_panels:
        n_items = _plan_len(n_rows, n_words, rank, world, form.plan, ctx.get_option("n_cus"))
        assert ctx.last_launch_info()["items"] == n_items, case
    kernels = ctx.last_pass_report()["kernels"]
    assert set(kernels) <= {pf.REPORTED[choice.family]}, case    # (a rank without an item launches no kernel)
    return kernels


@pytest.mark.parametrize("n_rows,created,n_words", SHAPES)
def test_a_dense_pass_reports_the_tables_choice(ctx, n_rows, created, n_words):
    m = _matrix(ctx, n_rows, created, n_words)
    shape = pf.Shape(n_rows, pf.allocation(created or n_rows), n_words, pf.stride(n_words))
    try:
        want = m.column_identity()
        for o in _options(ctx):
            _set(ctx, o)
            for world in (1, 2):
                choice = pf.choose("dense", o, shape._replace(shard_count=world))
                total, kernels = 0, set()
                for rank in range(world):
                    case = (n_rows, created, n_words, o[:3], rank, world)
                    before = ctx.get_option("k2_strip_rows_used")
                    total += m.pairw(rank, world)
                    kernels |= set(_check_report(ctx, choice, before, n_rows, n_words, rank, world, case))
                assert total == want, (n_rows, created, n_words, o[:3], world, total, want)
                assert kernels == {pf.REPORTED[choice.family]}, (n_rows, created, n_words, o[:3], world)
    finally:
        m.close()
        _set(ctx, pf.Options())


@pytest.mark.parametrize("n_rows", (2047, 2048))
def test_an_upload_pass_runs_in_panels_where_the_table_says_so(ctx, n_rows):
    n_words = 8
    mat = _rows(n_rows, n_words)
    m = ctx.matrix(n_rows, n_words)
    shape = pf.Shape(n_rows, pf.allocation(n_rows), n_words, pf.stride(n_words))
    try:
        m.upload(mat)
        want = m.column_identity()
        for o in _options(ctx):
            _set(ctx, o)
            choice = pf.choose("upload", o, shape)
            case = (n_rows, o[:3])
            before = ctx.get_option("k2_strip_rows_used")
            assert m.pairw_upload(mat) == want, case
            assert _check_report(ctx, choice, before, n_rows, n_words, 0, 1, case) == [pf.REPORTED[choice.family]], case
            if choice.family not in ("popcount", "k2q"):    # (these two count their own segments in that word)
                assert (ctx.last_launch_info()["segments"] > 0) == choice.in_panels, case
            assert choice.in_panels == (n_rows >= 2048 and o.variant in (-1, 4) and o.k2_strip_operands in (0, 5, 6)), case
    finally:
        m.close()
        _set(ctx, pf.Options())


def _sparse_case():
    """40 rows x 3 block columns: bitmaps in columns 0 and 2 (column 2: the first 9 rows only), short lists in column 1.
    Returns (description, total): the total is the sum over every position of every column of C(rows that hold it, 2)."""
    rng = np.random.default_rng(77)
    d, total = Desc(), 0
    counts = np.zeros((3, 65536), dtype=np.int64)
    for row in range(40):
        bitmap = rng.integers(0, 1 << 64, size=1024, dtype=np.uint64) & rng.integers(0, 1 << 64, size=1024, dtype=np.uint64)
        d.block(0, 1, bitmap, NONE)
        counts[0] += np.unpackbits(bitmap.view(np.uint8), bitorder="little")
        positions = np.sort(rng.choice(65536, size=30, replace=False)).astype(np.uint16)
        d.block(1, 0, positions, NONE)
        counts[1, positions] += 1
        if row < 9:
            d.block(2, 1, bitmap[::-1].copy(), NONE)
            counts[2] += np.unpackbits(bitmap[::-1].copy().view(np.uint8), bitorder="little")
        d.end_row()
    total = int((counts * (counts - 1) // 2).sum())
    return d, total


def test_a_sparse_pool_takes_the_256_row_form_whatever_was_asked_for(ctx):
    lib = ctx._lib
    d, want = _sparse_case()
    n_rows, n_blocks, off, ids, kinds, lens, ptrs, _ = d.arrays()
    h = C.c_void_p()
    sb._lib.check(lib.storm_hip_sparse_create_blocks(ctx._h, n_rows, n_blocks, _p(off), _p(ids), _p(kinds), _p(lens), _p(ptrs),
                                                     C.byref(h)), "storm_hip_sparse_create_blocks")
    try:
        ctx.set_option("variant", 4)
        for operands, strip_rows in ((0, 0), (6, 0), (0, 128), (4, 0)):
            o = pf.Options(4, operands, strip_rows)
            _set(ctx, o)
            choice = pf.choose("pool", o, pf.Shape(rows_dst=512, pool_rows_ready=512, widest=40))
            out = C.c_uint64()
            sb._lib.check(lib.storm_hip_pairw_sparse(ctx._h, h, 0, 1, C.byref(out)), "storm_hip_pairw_sparse")
            assert out.value == want, (operands, strip_rows, out.value, want)
            kernels = ctx.last_pass_report()["kernels"]
            assert pf.REPORTED[choice.family] in kernels and "probe_lists_kernel" in kernels, (operands, kernels)
            assert ctx.get_option("variant_used") == 4
            if operands != 4:
                assert choice.form == "bits" and "strip16_bits_kernel" in kernels and "strip16_fp4_kernel" not in kernels
                assert ctx.get_option("k2_operands_used") == 5 and ctx.get_option("k2_strip_rows_used") == 64, operands
            else:
                assert "strip16_fp4_kernel" in kernels and "strip16_bits_kernel" not in kernels
    finally:
        lib.storm_hip_sparse_destroy(ctx._h, h)
        _set(ctx, pf.Options())
