"""K2b with 128 A rows per wave (strip16_rows_kernel, option k2_strip_rows = 128) through the C-ABI against the CPU oracle.

The form runs only where the zero rows of the allocation (a multiple of 256, at least 256) reach the next multiple of its
512-row A tile; everywhere else the 256-row form runs and `k2_strip_rows_used` says 64. Of the row counts below that means
128 at 512, 1536 (and 300, 770, 1000, 1500, 2000: ragged last blocks, a second tile of a few rows, cut runs — added so that
the new kernel itself meets those shapes) and 64 at 2, 65, 130, 513, 600, 1100, 1600. A second tile of ONE row reaches the
new kernel through a 1024-row matrix resized to 513 rows; the last test pins the rule of k2_strip_rows = 0."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = (2, 65, 130, 300, 512, 513, 770, 1100, 1500, 1536, 1600, 2000)
BITS = (64, 128, 192, 8256)
KINDS = ("half", "sparse", "ones", "single")
CUT_RUNS = (1536, 1600, 2000)   # k2_max_run 3: cut runs, continuation items without a diagonal, the rings wrap several times


def _used(rows):
    # the allocation rule of storm_hip_matrix_create (kRowPad, storm_hip_internal.h): rows padded to a multiple of 256, at
    # least 256 — restated here; if kRowPad changes, this line and the row lists above change with it
    pad = max(256, (rows + 255) // 256 * 256)
    return 128 if (rows + 511) // 512 * 512 <= pad else 64


def _pack(bits):
    """[rows, n_bits] of 0 / 1 -> [rows, words] uint64, bit b of a row in word b // 64 at position b % 64."""
    rows, n_bits = bits.shape
    words = (n_bits + 63) // 64
    full = np.zeros((rows, words * 64), dtype=np.uint8)
    full[:, :n_bits] = bits
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view(np.uint64).reshape(rows, words)


@functools.lru_cache(maxsize=None)
def _case(kind, rows, n_bits):
    rng = np.random.default_rng(rows * 7 + n_bits)
    if kind == "half":
        bits = rng.integers(0, 2, size=(rows, n_bits), dtype=np.uint8)
    elif kind == "sparse":
        bits = (rng.random((rows, n_bits)) < 0.02).astype(np.uint8)
    elif kind == "ones":       # every triangle-mask error shows
        bits = np.ones((rows, n_bits), dtype=np.uint8)
    else:                      # row i = the single bit i mod M: any disagreement on the k order or the row mapping shows
        bits = np.zeros((rows, n_bits), dtype=np.uint8)
        bits[np.arange(rows), np.arange(rows) % n_bits] = 1
    if rows > 2:
        bits[rows // 2] = 0    # one all-zero row in the middle
    mat = _pack(bits)
    from tests._orc import Oracle
    want = Oracle().wrapper_diag_blocked(mat, 31)
    mat.setflags(write=False)
    return mat, want


def _reset(ctx):
    for key, value in (("k2_strip_rows", 0), ("k2_fold_inline", -1), ("k2_max_run", 0)):
        ctx.set_option(key, value)


def _check(ctx, kind, rows, n_bits):
    mat, want = _case(kind, rows, n_bits)
    m = ctx.matrix_from_host(mat)
    case = (kind, rows, n_bits)
    try:
        ctx.set_option("k2_strip_rows", 128)
        ctx.set_option("k2_max_run", 3 if rows in CUT_RUNS else 0)
        for fold in (-1, 0, 1):
            ctx.set_option("k2_fold_inline", fold)
            for rep in range(3):   # (again: the slots must have come back zeroed)
                got = m.pairw()
                assert ctx.get_option("k2_strip_rows_used") == _used(rows), case
                assert ctx.get_option("k2_operands_used") == 5, case
                assert got == want, (case, fold, rep, got, want)
        ctx.set_option("k2_fold_inline", -1)
        for world in (2, 3):
            assert sum(m.pairw(rank, world) for rank in range(world)) == want, (case, world)
            assert ctx.get_option("k2_strip_rows_used") == _used(rows), case
        for form in (0, 64):
            ctx.set_option("k2_strip_rows", form)
            assert m.pairw() == want, (case, form)
        assert ctx.get_option("k2_strip_rows_used") == 64, case
    finally:
        m.close()
        _reset(ctx)


@pytest.mark.parametrize("rows", ROWS)
def test_strip_rows_against_the_oracle(hip_ctx, rows):
    for n_bits in BITS:
        for kind in KINDS:
            _check(hip_ctx, kind, rows, n_bits)


def test_strip_rows_falls_back_where_the_zero_rows_end_and_says_so(hip_ctx):
    """1100 rows: three tiles, the allocation's zero rows reach 1280 but not 1536 — the 256-row form runs."""
    mat, want = _case("half", 1100, 192)
    m = hip_ctx.matrix_from_host(mat)
    try:
        hip_ctx.set_option("k2_strip_rows", 128)
        assert m.pairw() == want
        assert hip_ctx.get_option("k2_strip_rows_used") == 64
    finally:
        m.close()
        _reset(hip_ctx)
    mat, want = _case("half", 1536, 192)
    m = hip_ctx.matrix_from_host(mat)
    try:
        hip_ctx.set_option("k2_strip_rows", 128)
        assert m.pairw() == want
        assert hip_ctx.get_option("k2_strip_rows_used") == 128
        hip_ctx.set_option("k2_strip_operands", 6)   # the 8-wave form keeps its kernel
        assert m.pairw() == want
        assert hip_ctx.get_option("k2_strip_rows_used") == 64 and hip_ctx.get_option("k2_operands_used") == 6
    finally:
        hip_ctx.set_option("k2_strip_operands", 0)
        m.close()
        _reset(hip_ctx)


@pytest.mark.parametrize("rows", (600, 1000))
def test_strip_rows_at_512_slices_and_a_padded_pitch(hip_ctx, rows):
    """65536 bits: 512 slices of 128 bits, rows of 8 KiB — a multiple of 1 KiB, so the pitch pad applies (600 rows fall back
    by the rule above, 1000 run the new form)."""
    for kind in ("half", "ones", "single"):
        _check(hip_ctx, kind, rows, 65536)


def test_strip_rows_second_tile_of_one_row(hip_ctx):
    """513 rows in an allocation that reaches 1024 (a matrix created with 1024 rows and resized: the allocation stays, the
    rows dropped are cleared): the new kernel itself runs a second tile that holds ONE row, and 512 + 65 rows (a second
    tile of one ragged block)."""
    for rows in (513, 577):
        for n_bits in (192, 8256):
            for kind in KINDS:
                mat, want = _case(kind, rows, n_bits)
                m = hip_ctx.matrix(1024, mat.shape[1])
                try:
                    m.resize(rows)
                    m.upload(mat)
                    hip_ctx.set_option("k2_strip_rows", 128)
                    for fold in (-1, 0, 1):
                        hip_ctx.set_option("k2_fold_inline", fold)
                        assert m.pairw() == want, (kind, rows, n_bits, fold)
                        assert hip_ctx.get_option("k2_strip_rows_used") == 128
                    hip_ctx.set_option("k2_fold_inline", -1)
                    assert sum(m.pairw(r, 3) for r in range(3)) == want, (kind, rows, n_bits)
                    hip_ctx.set_option("k2_strip_rows", 64)
                    assert m.pairw() == want and hip_ctx.get_option("k2_strip_rows_used") == 64
                finally:
                    m.close()
                    _reset(hip_ctx)


def test_the_default_rule_takes_the_new_form_where_it_was_measured(hip_ctx):
    """k2_strip_rows 0: 128 rows per wave for one device's whole pass from 2048 rows x 65536 bits up; the 256-row form for
    shards, fewer rows and narrower rows. Totals against the column identity."""
    _reset(hip_ctx)
    for rows, n_bits, used in ((2048, 65536, 128), (2560, 65536, 128), (1536, 65536, 64), (2048, 32768, 64)):
        m = hip_ctx.matrix(rows, n_bits // 64)
        try:
            m.fill_synthetic(n_bits, n_bits // 3, seed=rows)
            want = m.column_identity()
            assert m.pairw() == want, (rows, n_bits)
            assert hip_ctx.get_option("k2_strip_rows_used") == used, (rows, n_bits)
            assert hip_ctx.get_option("k2_operands_used") == 5
            assert sum(m.pairw(r, 2) for r in range(2)) == want, (rows, n_bits)
            assert hip_ctx.get_option("k2_strip_rows_used") == 64, (rows, n_bits)
        finally:
            m.close()
