"""strip16_rows_kernel (K2b, 128 A rows per wave, option k2_strip_rows = 128) where the matrix ends inside a 64-row block,
through the C-ABI against the CPU oracle. The kernel is told the row count of a dense pass and issues no MFMA for zero rows
in whole units (storm_hip_plan.h: strip_rows_top_trimmed, strip_rows_real_blocks; tests/test_strip_rows_trim.py checks the
rules and the counts on the host): a run's top block with rows in 1 or 2 of its 4 fragments (F) becomes the run's LAST
stage, behind Tl = T - 1 whole stages, and multiplies those fragments alone; the diagonal phase stops at the tile's last
block that holds a row.

Rows, in an allocation that was resized so that zero rows reach the next multiple of 512:
  in 1024 rows: 528, 592, 656, 720 (T = 1 .. 4 with F = 1: Tl = 0 .. 3, every exit site of the loop and the prologue's),
  784 (Tl = 4: the second lap), 544, 608 (F = 2), 560 (F = 3: untrimmed), 576 (no ragged block), 513 (one real row), 529
  (F = 2 with a fragment of one row), 545 (F = 3);
  in 1536 rows: 1040 (tile 0 has a run of 9 stages that ends ragged, tile 1 a run of the ragged block only; also as two
  shards), 1296 (the last tile holds 5 blocks, as at 10000 rows, F = 1).
720 and 1040 rows run again with k2_max_run = 2: the ragged block sits in a short item, the other items are untrimmed.
Bits: 128 (one slice), 192 (a half-empty last slice), 8192. Data: all-ones rows, one-bit rows, density 0.5, and rows whose
popcount is (row mod 64) + 1 — a fragment that is skipped, doubled or mapped to the wrong rows changes the total. Every case
runs in the three fold modes, twice in a row on one context: the second run shows that the slots came back zeroed."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IN_1024 = (528, 592, 656, 720, 784, 544, 608, 560, 576, 513, 529, 545)
IN_1536 = (1040, 1296)
BITS = (128, 192, 8192)
KINDS = ("ones", "single", "half", "rowid")


def _pack(bits):
    """[rows, n_bits] of 0 / 1 -> [rows, words] uint64, bit b of a row in word b // 64 at position b % 64."""
    rows, n_bits = bits.shape
    words = (n_bits + 63) // 64
    full = np.zeros((rows, words * 64), dtype=np.uint8)
    full[:, :n_bits] = bits
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view(np.uint64).reshape(rows, words)


@functools.lru_cache(maxsize=None)
def _case(kind, rows, n_bits):
    rng = np.random.default_rng(rows * 13 + n_bits)
    if kind == "ones":
        bits = np.ones((rows, n_bits), dtype=np.uint8)
    elif kind == "single":
        bits = np.zeros((rows, n_bits), dtype=np.uint8)
        bits[np.arange(rows), np.arange(rows) % n_bits] = 1
    elif kind == "half":
        bits = rng.integers(0, 2, size=(rows, n_bits), dtype=np.uint8)
    else:
        bits = (np.arange(n_bits)[None, :] < (np.arange(rows) % 64 + 1)[:, None]).astype(np.uint8)
    mat = _pack(bits)
    from tests._orc import Oracle
    want = Oracle().wrapper_diag_blocked(mat, 31)
    mat.setflags(write=False)
    return mat, want


def _reset(ctx):
    for key, value in (("k2_strip_rows", 0), ("k2_fold_inline", -1), ("k2_max_run", 0)):
        ctx.set_option(key, value)


def _check(ctx, kind, rows, n_bits, alloc_rows, shards=(), max_run=0):
    mat, want = _case(kind, rows, n_bits)
    case = (kind, rows, n_bits, max_run)
    m = ctx.matrix(alloc_rows, mat.shape[1])
    try:
        m.resize(rows)
        m.upload(mat)
        ctx.set_option("k2_strip_rows", 128)
        ctx.set_option("k2_max_run", max_run)
        for fold in (-1, 0, 1):
            ctx.set_option("k2_fold_inline", fold)
            for rep in range(2):
                got = m.pairw()
                assert ctx.get_option("k2_strip_rows_used") == 128, case
                assert got == want, (case, fold, rep, got, want)
        ctx.set_option("k2_fold_inline", -1)
        for world in shards:
            assert sum(m.pairw(rank, world) for rank in range(world)) == want, (case, world)
            assert ctx.get_option("k2_strip_rows_used") == 128, case
    finally:
        m.close()
        _reset(ctx)


@pytest.mark.parametrize("rows", IN_1024)
def test_ragged_top_block_in_a_1024_row_allocation(hip_ctx, rows):
    for n_bits in BITS:
        for kind in KINDS:
            _check(hip_ctx, kind, rows, n_bits, 1024)


@pytest.mark.parametrize("rows", IN_1536)
def test_ragged_top_block_behind_a_long_run_and_a_short_last_tile(hip_ctx, rows):
    for n_bits in BITS:
        for kind in KINDS:
            _check(hip_ctx, kind, rows, n_bits, 1536, shards=(2,) if rows == 1040 else ())


@pytest.mark.parametrize("rows,alloc_rows", ((720, 1024), (1040, 1536)))
def test_ragged_top_block_in_a_short_item_of_a_cut_run(hip_ctx, rows, alloc_rows):
    for n_bits in BITS:
        for kind in KINDS:
            _check(hip_ctx, kind, rows, n_bits, alloc_rows, max_run=2)
