"""strip16_rows_kernel on the work list whose tail the planner chose (no shaping option set: a fresh context) against the
CPU oracle, at the smallest shapes the default rule gives to the form: 2048 x 65536; 2560 rows, and 2064 rows in a
2560-row allocation that was resized (a ragged top block: one 16-row fragment of block 32 holds rows); 2048 x 65600 (an
odd last slice). The three fold modes once each; what the context says it used (k2_*_used, the item count) is the host
planner's choice for the shape; and with k2_tail_run / k2_tail_slices set the list is the explicit plan's."""
import functools

import numpy as np
import pytest

import stormbitmaps_amd as sb
from stormbitmaps_amd import dist

pytestmark = pytest.mark.gpu

# (rows, bits, rows of the allocation the matrix is created with, or None: as the rows ask)
SHAPES = ((2048, 65536, None), (2560, 65536, None), (2064, 65536, 2560), (2048, 65600, None))
USED = ("k2_max_run_used", "k2_tail_run_used", "k2_tail_slices_used")


@functools.lru_cache(maxsize=None)
def _case(rows, n_bits):
    words = n_bits // 64
    rng = np.random.default_rng(rows * 7 + n_bits)
    mat = rng.integers(0, 1 << 63, size=(rows, words), dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, size=(rows, words), dtype=np.uint64)
    mat[rows // 2] = 0
    from tests._orc import Oracle
    want = Oracle().wrapper_diag_blocked(mat, 31)
    mat.setflags(write=False)
    return mat, want


def _matrix(ctx, rows, n_bits, alloc_rows):
    mat, want = _case(rows, n_bits)
    if alloc_rows is None:
        return ctx.matrix_from_host(mat), want
    m = ctx.matrix(alloc_rows, mat.shape[1])
    m.resize(rows)
    m.upload(mat)
    return m, want


@pytest.fixture(scope="module")
def fresh_ctx():
    """A context on which no shaping option was ever set (the session's shared one has had k2_tail_run set by other tests)."""
    ctx = sb.HipContext(0)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("rows,n_bits,alloc_rows", SHAPES)
def test_the_chosen_list_against_the_oracle(fresh_ctx, rows, n_bits, alloc_rows):
    ctx = fresh_ctx
    m, want = _matrix(ctx, rows, n_bits, alloc_rows)
    try:
        plan, shaping = dist.strip_plan(rows, n_bits // 64, 0, 1, 2, tail_run=0, n_cus=ctx.get_option("n_cus"), return_run=True)
        for fold in (-1, 0, 1):
            ctx.set_option("k2_fold_inline", fold)
            got = m.pairw()
            assert got == want, (rows, n_bits, fold, got, want)
            assert ctx.get_option("k2_strip_rows_used") == 128
            assert tuple(ctx.get_option(key) for key in USED) == shaping, (rows, n_bits)
            assert ctx.last_launch_info()["items"] == len(plan), (rows, n_bits)
    finally:
        ctx.set_option("k2_fold_inline", -1)
        m.close()


def test_a_list_too_long_to_be_all_tail_against_the_column_identity(fresh_ctx):
    """4096 x 65536: more than the 6 rounds that are ordered as one tail, so the candidates differ there (the lists above
    are all tail and every candidate cuts them alike). Total against the column identity of the synthetic matrix."""
    ctx = fresh_ctx
    rows, n_bits = 4096, 65536
    m = ctx.matrix(rows, n_bits // 64)
    try:
        m.fill_synthetic(n_bits, n_bits // 3, seed=rows)
        plan, shaping = dist.strip_plan(rows, n_bits // 64, 0, 1, 2, tail_run=0, n_cus=ctx.get_option("n_cus"), return_run=True)
        assert m.pairw() == m.column_identity()
        assert ctx.get_option("k2_strip_rows_used") == 128
        assert tuple(ctx.get_option(key) for key in USED) == shaping
        assert ctx.last_launch_info()["items"] == len(plan)
    finally:
        m.close()


def test_a_set_tail_is_taken_as_it_is():
    rows, n_bits = 2048, 65536
    ctx = sb.HipContext(0)
    m, want = _matrix(ctx, rows, n_bits, None)
    try:
        ctx.set_option("k2_tail_run", 32)
        ctx.set_option("k2_tail_slices", 3)
        plan, run = dist.strip_plan(rows, n_bits // 64, 0, 1, 2, tail_run=32, tail_slices=3, n_cus=ctx.get_option("n_cus"), return_run=True)
        assert m.pairw() == want
        assert ctx.last_launch_info()["items"] == len(plan)
        assert tuple(ctx.get_option(key) for key in USED) == (run, 32, 3)
        assert ctx.get_option("k2_tail_run") == 32 and ctx.get_option("k2_tail_slices") == 3
        # ... and a tail of another length, which no candidate has
        ctx.set_option("k2_tail_slices", 5)
        plan5 = dist.strip_plan(rows, n_bits // 64, 0, 1, 2, tail_run=32, tail_slices=5, n_cus=ctx.get_option("n_cus"))
        assert m.pairw() == want
        assert ctx.last_launch_info()["items"] == len(plan5)
        assert tuple(ctx.get_option(key) for key in USED)[1:] == (32, 5)
    finally:
        m.close()
        ctx.close()
