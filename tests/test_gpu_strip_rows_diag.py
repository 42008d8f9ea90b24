"""The diagonal phase of K2b's 128-rows-per-wave form (strip16_rows_kernel, option k2_strip_rows = 128) through the C-ABI
against the CPU oracle: wave w keeps blocks w and 7 - w of the 512-row A tile, the tile is published as eight resident FP4
images behind one barrier, and every wave walks the blocks from its own one upwards without a barrier
(storm_hip_plan.h: strip_rows_role; tests/test_strip_rows_diag_schedule.py checks the schedule itself on the host).

Rows: 512 (one tile, the diagonal only: no pipelined stage), 1024 (one tile with a run behind its diagonal, one without),
1536, 2048 (also as two shards), and 513, 600, 1000 rows in a 1024-row allocation that was resized, so that blocks of the
last tile are zero rows. Bits: 128 (one slice), 192 (a half-empty last slice), 8192, and 65536 once at 1024 rows (the padded
pitch). Data: all-ones rows (every mask error shows), one-bit rows (the k order and the row mapping), density 0.5, and
block-identifying rows — every row of 64-row block b of a tile has its first 8 (b + 1) bits set, so a block pair that is
skipped, doubled or handed to the wrong half changes the total. Every case runs in the three fold modes, twice in a row on
one context: the second run shows that the slots came back zeroed."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WHOLE = (512, 1024, 1536, 2048)      # allocated as they are
RESIZED = (513, 600, 1000)           # in a 1024-row allocation
BITS = (128, 192, 8192)
KINDS = ("ones", "single", "half", "blockid")


def _pack(bits):
    """[rows, n_bits] of 0 / 1 -> [rows, words] uint64, bit b of a row in word b // 64 at position b % 64."""
    rows, n_bits = bits.shape
    words = (n_bits + 63) // 64
    full = np.zeros((rows, words * 64), dtype=np.uint8)
    full[:, :n_bits] = bits
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view(np.uint64).reshape(rows, words)


@functools.lru_cache(maxsize=None)
def _case(kind, rows, n_bits):
    rng = np.random.default_rng(rows * 11 + n_bits)
    if kind == "ones":
        bits = np.ones((rows, n_bits), dtype=np.uint8)
    elif kind == "single":
        bits = np.zeros((rows, n_bits), dtype=np.uint8)
        bits[np.arange(rows), np.arange(rows) % n_bits] = 1
    elif kind == "half":
        bits = rng.integers(0, 2, size=(rows, n_bits), dtype=np.uint8)
    else:
        block = (np.arange(rows) % 512) // 64
        bits = (np.arange(n_bits)[None, :] < 8 * (block[:, None] + 1)).astype(np.uint8)
    mat = _pack(bits)
    from tests._orc import Oracle
    want = Oracle().wrapper_diag_blocked(mat, 31)
    mat.setflags(write=False)
    return mat, want


def _reset(ctx):
    for key, value in (("k2_strip_rows", 0), ("k2_fold_inline", -1)):
        ctx.set_option(key, value)


def _check(ctx, kind, rows, n_bits, alloc_rows=None, shards=()):
    mat, want = _case(kind, rows, n_bits)
    case = (kind, rows, n_bits)
    if alloc_rows is None:
        m = ctx.matrix_from_host(mat)
    else:
        m = ctx.matrix(alloc_rows, mat.shape[1])
    try:
        if alloc_rows is not None:
            m.resize(rows)
            m.upload(mat)
        ctx.set_option("k2_strip_rows", 128)
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


@pytest.mark.parametrize("rows", WHOLE)
def test_diagonal_phase_against_the_oracle(hip_ctx, rows):
    for n_bits in BITS:
        for kind in KINDS:
            _check(hip_ctx, kind, rows, n_bits, shards=(2,) if rows == 2048 else ())


@pytest.mark.parametrize("rows", RESIZED)
def test_diagonal_phase_with_zero_blocks_in_the_last_tile(hip_ctx, rows):
    for n_bits in BITS:
        for kind in KINDS:
            _check(hip_ctx, kind, rows, n_bits, alloc_rows=1024)


def test_diagonal_phase_at_512_slices_and_a_padded_pitch(hip_ctx):
    for kind in ("ones", "half", "blockid"):
        _check(hip_ctx, kind, 1024, 65536)
