"""The dense matrix-core paths on saturated and structured rows: everything in the dense kernels whose correctness rests on
a count staying below a bound (16-bit windows, f32 accumulators at 2^24, strip runs of 4096 stages, K2q shares of 8192, the
popcount kernel's uint32 lanes, uint32 OR / XOR epilogues) and on "rows >= n_rows and words >= n_words are zero", with inputs
that REACH the bound — random rows at 4 .. 63 % density reach a quarter to a half of it. Every expected value is a closed
form (tests/_dense_edges.py) or the numpy product; the CPU oracle is not needed. Everything goes through the C-ABI; each case
asserts which kernel ran, and tests/test_dense_edge_shapes.py asserts on the CPU that each shape sits on its limit."""
import time

import numpy as np
import pytest

import stormbitmaps_amd as sb
from stormbitmaps_amd import dist
from tests import _dense_edges as de
from tests.conftest import shipped

pytestmark = pytest.mark.gpu

SENTINEL = 0x9E3779B9
# every settable option and the initialiser of its member in storm_hip_ctx_s (storm_hip_internal.h)
DEFAULTS = {"variant": -1, "probe_bundle": -1, "sparse_probe": -1, "result_mailbox": 1, "sync_poll_us": 0, "matrix_lists": -1,
            "matrix_lists_kernel": 0, "matrix_lists_hash_min_log2": 6, "matrix_lists_debug": 0, "matrix_lists_density": 80,
            "seg_rows": 256, "k2_stages_per_item": 32, "k2_max_run": 0, "k2_ring": 4, "k2_shadow_budget_mb": 96 * 1024,
            "k2_tile_shape": 0, "k2_ring_sync": 0, "k2_wave_below": 400, "k2_part_slots": 0, "k2_part_min_chunks": 8,
            "k2_part_narrow": 1, "k2_part_cost_diag": 80, "k2_ring_cost_diag": 78, "k2_ring_cost_ragged": 40,
            "k2_tile_cost_diag": 63, "k2_tile_cost_ragged": 30, "k2_strip_operands": 0, "k2_shard_pairs": 0, "k2_matrix_pad": -1,
            "k2_fold_inline": -1, "k2_wave_ring": 0, "k2_stream_max_rows": 8192, "k2_stream_groups_per_cu": 0,
            "k2_stream_min_piece": 6, "k2_stream_min_run": 2, "k2_stream_w3_1": 120, "k2_stream_w3_2": 60, "k2_shape": 16,
            "keep_shadow": 0, "k2_matrix_parts": 0, "k2_matrix_min_part": 32, "k2_matrix_split": 1, "k2_pitch_pad": -1,
            "k2_lds_pad": 0, "k2_persistent": 0, "k2_lpt_rounds": 6, "k2_tail_slices": 3, "k2_tail_run": 32, "k2_debug": 0,
            "time_kernels": 0, "chunks_per_item": 0}


@pytest.fixture(scope="module")
def hip_ctx():
    ctx = sb.HipContext(0)
    yield ctx
    ctx.close()


@pytest.fixture()
def ctx(hip_ctx):
    """The module's context; every option a case may touch is back at its default afterwards."""
    try:
        yield hip_ctx
    finally:
        for k, v in DEFAULTS.items():
            hip_ctx.set_option(k, v)


def _set(ctx, **options):
    for k, v in options.items():
        ctx.set_option(k, v)


def _first_diffs(want: np.ndarray, got: np.ndarray, n: int = 4):
    """The first few (i, j, want, got) where two arrays differ."""
    return [(int(i), int(j), int(want[i, j]), int(got[i, j])) for i, j in np.argwhere(want != got)[:n]]


def _sentinel_i32():
    return int(np.array(SENTINEL, dtype=np.uint32).view(np.int32))


def _device_saturated(torch, ctx, n_rows: int, n_bits: int, clear_bit=None, piece: int = 65):
    """A saturated (or, with clear_bit, odd-saturated) matrix built on the device: a piece of all-ones rows made by torch,
    imported until the matrix is full. n_bits is a multiple of 64."""
    assert n_bits % 64 == 0
    W = n_bits // 64
    m = ctx.matrix(n_rows, W)
    src = torch.full((min(piece, n_rows), W), -1, dtype=torch.int64, device="cuda:0")
    if clear_bit is not None:
        word = src[:, clear_bit // 64]
        word &= ~(1 << (clear_bit % 64)) if clear_bit % 64 < 63 else 0x7FFFFFFFFFFFFFFF
    for row0 in range(0, n_rows, src.shape[0]):
        m.import_device(src.data_ptr(), min(src.shape[0], n_rows - row0), W, row0=row0)
    ctx.synchronize()
    del src
    torch.cuda.empty_cache()
    return m


def _square_matrix_device(ctx, a, b, d_out: int, ld: int, op: str):
    """storm_hip_square_matrix_device (api.HipMatrix wraps the host form only)."""
    import ctypes as C
    sb._lib.check(sb.load().storm_hip_square_matrix_device(ctx._h, a._h, b._h, a.OPS[op], C.c_void_p(d_out), ld),
                  "storm_hip_square_matrix_device")


def _wide_strips(n_rows: int) -> bool:
    """Whether k2_strip_operands = 6 runs its 512-row form: the matrix's zero rows (allocated in multiples of 256) must
    reach the next multiple of 512."""
    return (n_rows + 511) // 512 * 512 <= max(256, (n_rows + 255) // 256 * 256)


def _cycle(values, n):
    return [values[i % len(values)] for i in range(n)]


# =========================================================================================================================
# case 1
# =========================================================================================================================
@pytest.mark.parametrize("shape", (de.K2H_NARROW, de.K2H_WIDE), ids=("narrow_127_chunks", "wide_128_chunks"))
def test_k2h_part_windows_at_the_limit_of_16_bit_counts(ctx, shape):
    """tile128_kernel's k-parts travel through windows of 16-bit counts while every part of a tile is at most 127 chunks
    (65024 bits). Rows of 254 chunks in parts of exactly 127 (the largest count a narrow window carries: 65024, in every
    entry at once), and rows of 256 chunks in parts of 128 (65536: must go through wide windows — a 16-bit count would wrap
    to 0 and carry into its neighbour in the packed dword). Saturated, odd-saturated and staircase rows (lengths one bit
    either side of the cut), AND / OR / XOR, triangle / band that starts inside a tile / rectangle, every call twice (tickets
    left at zero), one and two slots per CU, and with the narrow windows switched off."""
    import torch
    M = 64 * shape["n_words"]
    n_cus = ctx.get_option("n_cus")
    N = de.K2H_ROWS[1]
    L = de.staircase_lengths(M, cut_chunks=(shape["part_chunks"],))
    S = [0, 1, 64, 511, 512, 513, M - 512 * shape["part_chunks"] - 1, M - 512 * shape["part_chunks"], M - 1, M]
    pre, suf = _cycle(L, 2 * N // 3), _cycle(S, N - 2 * N // 3)
    inputs = {"saturated": (de.saturated(N, M),) + de.staircase_counts(M, [M] * N),
              "odd_bit0": (de.saturated(N, M, clear=(0,)),) + de.staircase_counts(M, [M - 1] * N),
              "odd_last": (de.saturated(N, M, clear=(M - 1,)),) + de.staircase_counts(M, [M - 1] * N),
              "staircase": (de.staircase(M, pre, suf),) + de.staircase_counts(M, pre, suf)}
    assert (M - 1) % 2 == 1
    _set(ctx, k2_tile_shape=6, k2_part_min_chunks=shape["min_chunks"])
    for name, (mat, n_i, _, cnt) in inputs.items():
        m = ctx.matrix_from_host(mat)
        small = ctx.matrix_from_host(mat[:de.K2H_ROWS[0]])
        ra, rb = de.K2H_RECT
        a, b = ctx.matrix_from_host(mat[:ra]), ctx.matrix_from_host(mat[N - rb:])
        assert np.array_equal(m.row_counts(), n_i)
        for narrow in (1, 0):
            for slots in de.K2H_SLOTS:
                _set(ctx, k2_part_narrow=narrow, k2_part_slots=slots)
                for op in ("and", "or", "xor"):
                    full = de.op_counts(n_i, n_i, cnt, op)
                    want = np.triu(full, k=1).astype(np.uint32)
                    for rep in range(2):
                        got = m.pairw_matrix(op)
                        assert ctx.get_option("k2_tile_shape_used") == 6
                        assert np.array_equal(want, got), (name, narrow, slots, op, rep, _first_diffs(want, got))
                    n0 = de.K2H_ROWS[0]
                    got = small.pairw_matrix(op)
                    assert np.array_equal(want[:n0, :n0], got), (name, "256 rows", narrow, slots, op, _first_diffs(want[:n0, :n0], got))
                    # band that starts inside a tile, left in device memory; untouched entries keep the sentinel
                    r0, nr = de.K2H_BAND
                    band = torch.full((nr, N), _sentinel_i32(), dtype=torch.int32, device="cuda:0")
                    for rep in range(2):
                        m.pairw_matrix_band_device(band.data_ptr(), N, r0, nr, op)
                        gotb = band.cpu().numpy().view(np.uint32)
                        wantb = np.where(np.arange(N)[None, :] > (r0 + np.arange(nr))[:, None], full[r0:r0 + nr], SENTINEL).astype(np.uint32)
                        assert np.array_equal(wantb, gotb), (name, "band", narrow, slots, op, rep, _first_diffs(wantb, gotb))
                    # rectangle: every entry
                    wantr = full[:ra, N - rb:].astype(np.uint32)
                    for rep in range(2):
                        gotr = a.square_matrix(b, op)
                        assert ctx.get_option("k2_tile_shape_used") == 6
                        assert np.array_equal(wantr, gotr), (name, "rectangle", narrow, slots, op, rep, _first_diffs(wantr, gotr))
                # ... and these launches were on the limit: the plan for the device's own CU count (after the numbers, so that a
                # planner that lets a part too long through shows as the wrong count it causes)
                de.assert_k2h_on_limit(dist, shape, n_cus, slots)
        # totals of the same matrix on the default path (closed form: the triangle's sum)
        assert m.pairw() == int(np.triu(cnt, k=1).sum()) and a.square(b) == int(cnt[:ra, N - rb:].sum())
        for x in (m, small, a, b):
            x.close()


# =========================================================================================================================
# case 2
# =========================================================================================================================
def _check_constant_triangle(torch, out, n, value, what):
    """out ([n, n] int32 on the device, pre-filled with the sentinel): `value` strictly above the diagonal, untouched elsewhere."""
    upper = torch.triu(torch.ones((n, n), dtype=torch.bool, device=out.device), diagonal=1)
    want = torch.where(upper, torch.tensor(value, dtype=torch.int32, device=out.device),
                       torch.tensor(_sentinel_i32(), dtype=torch.int32, device=out.device))
    if not torch.equal(out, want):
        bad = torch.nonzero(out != want)[:4].cpu().tolist()
        got = out.cpu().numpy().view(np.uint32)
        raise AssertionError((what, "want", value, [(i, j, int(got[i, j]), "above diagonal" if j > i else "untouched") for i, j in bad]))


@pytest.mark.parametrize("n_bits", de.EXACT_BITS)
def test_per_pair_output_of_odd_saturated_rows_around_two_to_the_24_bits(ctx, n_bits):
    """The 2^24 cut of every per-pair output kernel planned by plan_matrix_tiles (k2_tile_shape 2, 3, 4, 5 with both ring
    syncs, 32): f32 accumulators hold exact integers below 2^24 only, so an item spans at most 2^24 - 128 bits of k and
    longer rows are cut, the parts added as integers. With k2_matrix_split 0 every tile is ONE item unless that cut
    intervenes (with few tiles the load-balancing split would otherwise cut every tile into short parts, and no test would
    see a missing exactness cut): at 2^24 - 512 bits the item is the longest legal one; from 2^24 bits on min_parts >= 2 is
    what keeps the result exact; 2^25 - 512 = 33553920 bits (the longest row) gives two parts, the second of exactly 2^24
    bits. Rows are ODD-saturated (every bit but one set, the same one in every row): every pair counts M - 1, odd, so an
    f32 sum carried past 2^24 in steps of 64 / 128 cannot stay exact (all-ones rows would: every partial sum is even).
    Also with the load-balancing split on, its parts added by atomics and by the summing kernel; OR / XOR; the host form;
    and the totals of the same matrix on the default path (K2b), K2q, 512-row strips, the FP4 strips and tiles, and the
    popcount kernel.
    (No planner of these kernels is exposed to the host, so that an item really stays whole is what the mutation recorded
    with this file's introduction shows: with kMaxExactStages doubled the AND count at 2^24 + 512 bits comes out even.)"""
    import torch
    N, value = de.EXACT_SMALL_ROWS, n_bits - 1
    assert value % 2 == 1 and n_bits < (1 << 25)
    clear_bit = 0 if n_bits != de.EXACT + 512 else n_bits - 1       # (the last bit of the row at one length, bit 0 elsewhere)
    m = _device_saturated(torch, ctx, N, n_bits, clear_bit=clear_bit)
    out = torch.empty((N, N), dtype=torch.int32, device="cuda:0")
    kernels = [(s, 0) for s in shipped(ctx, "k2_tile_shape", (2, 3, 4, 5))] + [(5, 1)]
    for tile_shape, ring_sync in kernels:
        _set(ctx, k2_tile_shape=tile_shape, k2_ring_sync=ring_sync)
        for split, parts in ((0, 0), (1, 0), (1, 1)):
            _set(ctx, k2_matrix_split=split, k2_matrix_parts=parts)
            # (OR / XOR: n_i + n_j - w x count in uint32, largest at the longest rows)
            ops = ("and", "or", "xor") if split == 0 and n_bits in (de.EXACT - 512, de.EXACT + 512, de.EXACT_BITS[-1]) else ("and",)
            for op in ops:
                out.fill_(_sentinel_i32())
                m.pairw_matrix_device(out.data_ptr(), N, op)
                assert ctx.get_option("k2_tile_shape_used") == tile_shape
                assert ctx.last_pass_report()["dense_word_pairs"] == de.choose2(N) * (n_bits // 64)
                _check_constant_triangle(torch, out, N, 0 if op == "xor" else value, (n_bits, tile_shape, ring_sync, split, parts, op))
    _set(ctx, k2_tile_shape=5, k2_ring_sync=0, k2_matrix_split=0)
    host = m.pairw_matrix("and")
    want_host = np.triu(np.full((N, N), value, dtype=np.uint32), k=1)
    assert np.array_equal(host, want_host), _first_diffs(want_host, host)
    _set(ctx, k2_tile_shape=0, k2_matrix_split=1)
    # totals
    want = de.choose2(N) * value
    assert (m.row_counts() == value).all() and m.column_identity() == want
    assert m.pairw() == want and ctx.get_option("k2_operands_used") == 5 and ctx.last_pass_report()["kernels"] == ["strip16_bits_kernel"]
    assert m.square(m) == N * N * value
    assert m.pairw_op("or") == want and m.pairw_op("xor") == 0
    for operands, used, kernel in ((2, 2, "bitstream_kernel"), (6, 6 if _wide_strips(N) else 5, "strip16_bits_kernel")):
        _set(ctx, k2_strip_operands=operands)
        assert m.pairw() == want, (n_bits, operands)
        assert ctx.get_option("k2_operands_used") == used and ctx.last_pass_report()["kernels"] == [kernel]
    _set(ctx, k2_strip_operands=0, variant=2)
    assert m.pairw() == want and ctx.get_option("variant_used") == 2 and ctx.last_pass_report()["kernels"] == ["pairw_dense_kernel"]
    _set(ctx, variant=-1)
    m.close()
    if n_bits <= de.EXACT + 512:
        # the kernels on an FP4 shadow (4 x the bits again): the three lengths around the cut, 130 rows, a shadow of 2 GiB.
        # Per-pair output (k2_tile_shape 32, planned by plan_matrix_tiles too), then the strips and tiles of the totals
        # (variant 3 accumulates k-slices of k2_stages_per_item stages: its own check refuses a k-slice of 2^24 bits and more,
        # which no legal option value reaches, so there is a value to assert and no refusal)
        n = 130
        m = _device_saturated(torch, ctx, n, n_bits, clear_bit=clear_bit)
        out = torch.empty((n, n), dtype=torch.int32, device="cuda:0")
        _set(ctx, k2_tile_shape=32)
        for split, parts in ((0, 0), (1, 0), (1, 1)):
            _set(ctx, k2_matrix_split=split, k2_matrix_parts=parts)
            for op in ("and", "or") if split == 0 else ("and",):
                out.fill_(_sentinel_i32())
                m.pairw_matrix_device(out.data_ptr(), n, op)
                assert ctx.get_option("k2_tile_shape_used") == 32
                _check_constant_triangle(torch, out, n, value, (n_bits, 32, split, parts, op))
        _set(ctx, k2_tile_shape=0, k2_matrix_split=1, k2_matrix_parts=0)
        _set(ctx, k2_strip_operands=4)
        assert m.pairw() == de.choose2(n) * value and ctx.get_option("k2_operands_used") == 4
        assert ctx.last_pass_report()["kernels"] == ["strip16_fp4_kernel"]
        _set(ctx, k2_strip_operands=0, variant=3)
        assert m.pairw() == de.choose2(n) * value and ctx.get_option("variant_used") == 3
        assert ctx.last_pass_report()["kernels"] == ["pairw_fp4_kernel"]
        m.close()


@pytest.mark.parametrize("n_bits", de.K2H_WHOLE_BITS)
def test_k2h_whole_tiles_of_odd_saturated_rows_around_two_to_the_24_bits(ctx, n_bits):
    """K2h has no option that keeps a tile whole: tiles stay whole only where there are at least as many tiles as slots. 2945
    rows are 300 tiles of 128 x 128: at 2^24 - 512 bits 256 of them are whole items of 32767 chunks, the longest an f32
    accumulator takes; at 2^24 + 512 every tile is in two parts because of kMaxExactChunks alone. ONE launch over the whole
    triangle (a band has fewer tiles than slots and would be cut for load balance), its 35 MB of output left on the device
    and compared there with the constant M - 1. 6.2 GB of rows, built on the device."""
    import torch
    N, value = de.K2H_WHOLE_ROWS, n_bits - 1
    assert value % 2 == 1
    n_cus = ctx.get_option("n_cus")
    m = _device_saturated(torch, ctx, N, n_bits, clear_bit=0 if n_bits < de.EXACT else n_bits - 1, piece=95)
    out = torch.empty((N, N), dtype=torch.int32, device="cuda:0")
    _set(ctx, k2_tile_shape=6)
    for op in ("and", "or", "xor"):
        out.fill_(_sentinel_i32())
        m.pairw_matrix_device(out.data_ptr(), N, op)
        assert ctx.get_option("k2_tile_shape_used") == 6
        _check_constant_triangle(torch, out, N, 0 if op == "xor" else value, (n_bits, "K2h", op))
    m.close()
    # ... and the launch was on the limit: the plan for the device's own CU count (after the numbers, so that a missing cut
    # shows as the wrong count it causes)
    plan = dist.matrix_plan(N, n_bits // 64, n_cus=n_cus)
    if n_bits < de.EXACT:
        assert (plan[:, 6] == 1).sum() >= min(n_cus, 256) and plan[:, 3].max() == (de.EXACT - 512) // 512
    else:
        assert (plan[:, 6] >= 2).all() and plan[:, 3].max() < de.EXACT // 512


# =========================================================================================================================
# case 3
# =========================================================================================================================
def _strip_kernels(ctx):
    """(options, k2_operands_used, kernel of the pass report) of every strip form this build carries."""
    forms = [({"k2_strip_operands": 0}, 5, "strip16_bits_kernel"), ({"k2_strip_operands": 5}, 5, "strip16_bits_kernel"),
             ({"k2_strip_operands": 6}, 6, "strip16_bits_kernel"), ({"k2_strip_operands": 4, "k2_shape": 16}, 4, "strip16_fp4_kernel")]
    if 32 in shipped(ctx, "k2_shape", (32,)):          # (tools build only, as the per-XCD work queues)
        forms.append(({"k2_strip_operands": 4, "k2_shape": 32}, 4, "strip16_fp4_kernel"))
    if 1 in shipped(ctx, "k2_persistent", (1,)):
        forms.append(({"k2_strip_operands": 4, "k2_shape": 16, "k2_persistent": 1}, 4, "strip16_fp4_kernel"))
    return forms


@pytest.mark.parametrize("n_rows", de.STRIP_LONG_ROWS)
def test_strip_totals_of_saturated_rows_with_runs_of_4096_stages(ctx, n_rows):
    """The strip kernels never flush their accumulators across the B stages of an item: "<= 256 (512) bits x 4096 stages <
    2^24", and k2_max_run / k2_tail_run accept up to 4096. 262400 (262465) saturated rows of 512 bits with both knobs at 4096
    hold items whose run is exactly 4096 blocks of 64 rows, every product at its maximum; the in-launch fold (a 48-bit sum
    and a 16-bit arrival count in one slot word) and the fold kernel. Total = C(N, 2) x 512."""
    import torch
    n_cus = ctx.get_option("n_cus")
    M = 64 * de.STRIP_LONG_WORDS
    m = _device_saturated(torch, ctx, n_rows, M, piece=65600)
    want = de.choose2(n_rows) * M
    assert m.column_identity() == want
    for options, used, kernel in _strip_kernels(ctx):
        _set(ctx, **options)
        form = 0 if used == 4 else 1
        for max_run, tail_run in de.STRIP_RUNS:
            _set(ctx, k2_max_run=max_run, k2_tail_run=tail_run)
            if (max_run, tail_run) == (4096, 4096) and used != 6:
                assert de.longest_run(dist, n_rows, de.STRIP_LONG_WORDS, form, max_run, tail_run, n_cus) == 4096
            for fold in (0, 1):
                _set(ctx, k2_fold_inline=fold)
                got = [m.pairw() for _ in range(2)]
                assert got == [want] * 2, (n_rows, options, max_run, tail_run, fold, got, want)
                ran = used if used != 6 or _wide_strips(n_rows) else 5
                assert ctx.get_option("k2_operands_used") == ran and ctx.last_pass_report()["kernels"] == [kernel]
        _set(ctx, k2_shape=16, k2_persistent=0, k2_max_run=0, k2_tail_run=32, k2_fold_inline=-1)
    _set(ctx, k2_strip_operands=0, k2_max_run=4096, k2_tail_run=4096)
    for pairs, world in ((0, 2), (1, 3), (0, 8), (1, 8)):
        _set(ctx, k2_shard_pairs=pairs)
        assert sum(m.pairw(r, world) for r in range(world)) == want, (n_rows, pairs, world)
    m.close()


def test_strip_totals_of_saturated_rows_at_the_ragged_edges(ctx):
    """The same forms on small saturated matrices: N = 0, 1, 63, 64, 65, 255 (mod 256); M a multiple of 512, of 64 only, of
    neither; runs of 1, the defaults and 4096; shards of 2, 3 and 8 in both ownership modes sum to C(N, 2) x M."""
    for n_rows in de.STRIP_RAGGED_ROWS:
        for M in de.STRIP_RAGGED_BITS:
            m = ctx.matrix_from_host(de.saturated(n_rows, M))
            want = de.choose2(n_rows) * M
            for options, used, kernel in _strip_kernels(ctx):
                _set(ctx, **options)
                for max_run, tail_run in de.STRIP_RUNS:
                    _set(ctx, k2_max_run=max_run, k2_tail_run=tail_run)
                    for fold in (0, 1):
                        _set(ctx, k2_fold_inline=fold)
                        got = m.pairw()
                        assert got == want, (n_rows, M, options, max_run, tail_run, fold, got, want)
                        assert ctx.get_option("k2_operands_used") == (used if used != 6 or _wide_strips(n_rows) else 5)
                        assert ctx.last_pass_report()["kernels"] == [kernel]
                _set(ctx, k2_max_run=0, k2_tail_run=32, k2_fold_inline=-1)
                if options["k2_strip_operands"] in (0, 4):
                    for world in (2, 3, 8):
                        for pairs in (0, 1):
                            _set(ctx, k2_shard_pairs=pairs)
                            assert sum(m.pairw(r, world) for r in range(world)) == want, (n_rows, M, options, world, pairs)
                    _set(ctx, k2_shard_pairs=0)
                _set(ctx, k2_shape=16, k2_persistent=0)
            _set(ctx, k2_strip_operands=0)
            assert m.pairw_op("or") == want and m.pairw_op("xor") == 0 and m.square(m) == n_rows * n_rows * M
            m.close()


def test_periodic_rows_against_the_numpy_product(ctx):
    """Rows (p, t) with bit b set iff b % p == t, p = 2 .. 512 — among them the four residues mod 4 that K2b's class-pair
    slices separate — against the numpy product: per pair on the output kernels, in total on every strip form and K2q. A
    defect bound to a bit phase shows in exactly the rows of that phase."""
    M = 6 * 512 + 64 + 17
    mat = np.concatenate([de.periodic(M, de.PERIODIC_SPECS)] * 8)          # 280 rows: every phase meets every phase across tiles too
    N = mat.shape[0]
    m = ctx.matrix_from_host(mat)
    for op in ("and", "or", "xor"):
        want = np.triu(de.numpy_counts(mat, op=op), k=1).astype(np.uint32)
        for tile_shape in shipped(ctx, "k2_tile_shape", (2, 3, 4, 5, 6, 32)):
            _set(ctx, k2_tile_shape=tile_shape)
            got = m.pairw_matrix(op)
            assert ctx.get_option("k2_tile_shape_used") == tile_shape
            spec = lambda r: de.PERIODIC_SPECS[r % len(de.PERIODIC_SPECS)]
            assert np.array_equal(want, got), (op, tile_shape, [(spec(i), spec(j), w, g)
                                                                for i, j, w, g in _first_diffs(want, got)])
        _set(ctx, k2_tile_shape=0)
    want = int(np.triu(de.numpy_counts(mat), k=1).sum())
    for operands, used in ((0, 5), (6, 6 if _wide_strips(N) else 5), (4, 4), (2, 2)):
        _set(ctx, k2_strip_operands=operands)
        assert m.pairw() == want and ctx.get_option("k2_operands_used") == used, operands
    _set(ctx, k2_strip_operands=0)
    for variant in (0, 1, 2, 3):
        _set(ctx, variant=variant)
        assert m.pairw() == want and ctx.get_option("variant_used") == variant
    m.close()


# =========================================================================================================================
# case 4
# =========================================================================================================================
@pytest.mark.parametrize("n_rows", de.STREAM_ROWS)
def test_k2q_shares_at_the_limit_of_their_accumulators(ctx, n_rows):
    """bitstream_kernel (K2q) holds its accumulators in halves that stay exact while a workgroup's share is at most
    kBsMaxStages = 8192 stages; the wave's own block is multiplied at half weight and the diagonal's set bits subtracted —
    largest with all-ones rows. By default the stream is cut into shares of ~80 stages; with one workgroup per CU the share
    is L / n_cus and the planner's guard (shares of at most kBsMaxStages / 2 on average) is what cuts it: rows of 2^19 bits
    give several thousand stages per workgroup. Saturated and odd-saturated rows; the longest workgroup must lie in
    (2048, 8192]; also with three workgroups per CU whose later shares are weighted tenfold."""
    import torch
    M = de.STREAM_BITS
    _set(ctx, k2_strip_operands=2)
    for clear_bit in (None, 0, M - 1):
        m = _device_saturated(torch, ctx, n_rows, M, clear_bit=clear_bit, piece=1024)
        value = M if clear_bit is None else M - 1
        want = de.choose2(n_rows) * value
        for per_cu, w1, w2 in ((1, 120, 60), (3, 1000, 1000), (0, 120, 60)):
            _set(ctx, k2_stream_groups_per_cu=per_cu, k2_stream_w3_1=w1, k2_stream_w3_2=w2)
            got = [m.pairw() for _ in range(2)]
            info = ctx.last_launch_info()
            assert ctx.get_option("k2_operands_used") == 2 and ctx.last_pass_report()["kernels"] == ["bitstream_kernel"]
            if per_cu:       # (three weighted workgroups per CU: a share beyond 2048 stages from 8191 rows on)
                assert info["chunks_per_item"] <= de.STREAM_MAX_STAGES, (n_rows, per_cu, info)
                assert 2048 < info["chunks_per_item"] or (per_cu == 3 and n_rows < 8191), (n_rows, per_cu, info)
            assert got == [want] * 2, (n_rows, clear_bit, per_cu, w1, w2, info, got, want)
        m.close()


# =========================================================================================================================
# case 5
# =========================================================================================================================
@pytest.mark.parametrize("variant", (0, 1, 2))
def test_popcount_kernel_at_the_clamp_of_its_uint32_lane_sums(ctx, variant):
    """pairw_dense_kernel's lanes add 32 rows x seg_rows x 64 bits per chunk into uint32 sums; launch_pairw_segments clamps
    chunks_per_item so that the worst case stays below 2^32. seg_rows 32768 (2^26 per chunk) with 4096 chunks per item asked
    for: the clamp must bring it to 63, and with saturated rows — more than seg_rows of them, 63 chunks of 4096 bits — a
    lane's sum really reaches 63 x 2^26 = 0.98 x 2^32 (at least 2^31: a signed or 31-bit accumulator fails too)."""
    seg_rows, cps_want = 32768, 63
    assert 32 * seg_rows * 64 * cps_want < (1 << 32) <= 32 * seg_rows * 64 * (cps_want + 1) and 32 * seg_rows * 64 * cps_want >= (1 << 31)
    import torch
    n_rows, M = seg_rows + 256, cps_want * 4096
    m = _device_saturated(torch, ctx, n_rows, M, piece=4128)
    _set(ctx, variant=variant, seg_rows=seg_rows, chunks_per_item=4096)
    t0 = time.perf_counter()
    got = m.pairw()
    print(f"popcount kernel variant {variant}: {n_rows} x {M} saturated, {time.perf_counter() - t0:.3f} s")
    info = ctx.last_launch_info()
    assert ctx.get_option("variant_used") == variant and ctx.last_pass_report()["kernels"] == ["pairw_dense_kernel"]
    assert info["chunks_per_item"] == cps_want, info
    assert got == de.choose2(n_rows) * M, (variant, got, de.choose2(n_rows) * M, info)
    m.close()


# =========================================================================================================================
# case 6
# =========================================================================================================================
def _observe(ctx, m):
    """Every number the dense paths give for a matrix, by kernel."""
    got = {}
    for name, options in (("default", {}), ("k2q", {"k2_strip_operands": 2}), ("strips512", {"k2_strip_operands": 6}),
                          ("fp4", {"k2_strip_operands": 4}), ("popcount", {"variant": 2})):
        _set(ctx, **options)
        got[name] = m.pairw()
        _set(ctx, k2_strip_operands=0, variant=-1)
    for tile_shape in (5, 6):
        _set(ctx, k2_tile_shape=tile_shape)
        got[f"matrix{tile_shape}"] = m.pairw_matrix("and")
        assert ctx.get_option("k2_tile_shape_used") == tile_shape
        got[f"xor{tile_shape}"] = m.pairw_matrix("xor")
    _set(ctx, k2_tile_shape=0)
    got["row_counts"] = m.row_counts()
    got["column_identity"] = m.column_identity()
    got["square"] = m.square(m)
    return got


def _expect_saturated(n_live, n_rows, M):
    """... of a matrix whose first n_live rows are saturated and whose other rows are zero."""
    live = (np.arange(n_rows) < n_live)
    cnt = np.where(live[:, None] & live[None, :], M, 0)
    n_i = np.where(live, M, 0)
    total = de.choose2(n_live) * M
    want = {k: total for k in ("default", "k2q", "strips512", "fp4", "popcount", "column_identity")}
    for tile_shape in (5, 6):
        want[f"matrix{tile_shape}"] = np.triu(cnt, k=1).astype(np.uint32)
        want[f"xor{tile_shape}"] = np.triu(de.op_counts(n_i, n_i, cnt, "xor"), k=1).astype(np.uint32)
    want["row_counts"] = n_i.astype(np.uint32)
    want["square"] = n_live * n_live * M
    return want


def _assert_same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert np.array_equal(got[k], want[k]), (what, k, _first_diffs(np.atleast_2d(want[k]), np.atleast_2d(got[k])))
        else:
            assert got[k] == want[k], (what, k, got[k], want[k])


@pytest.mark.parametrize("keep_shadow", (0, 1))
@pytest.mark.parametrize("n0", (391, 300))
def test_resize_keeps_rows_beyond_the_matrix_zero(ctx, keep_shadow, n0):
    """"Rows >= n_rows are zero" is what lets every dense kernel run without a ragged-edge path. storm_hip_matrix_resize
    must keep it: a saturated matrix of 700 rows shrunk to N0 (N0 % 256, % 128, % 64 != 0) gives what a fresh N0-row matrix
    gives — totals on every strip form, K2q and the popcount kernel, the per-pair matrix of tilering_kernel and K2h, row
    counts, the column identity, the rectangle with itself; grown back within the allocation and beyond it (the reallocating
    branch) the old rows are unchanged and the new ones download as zero. With keep_shadow 1 the FP4 shadow kept from the
    call before each step must not survive it."""
    n1, W = 700, 70
    M = 64 * W - 13
    assert n0 % 256 and n0 % 128 and n0 % 64
    _set(ctx, keep_shadow=keep_shadow)
    m = ctx.matrix_from_host(de.saturated(n1, M))
    _assert_same(_observe(ctx, m), _expect_saturated(n1, n1, M), "before")
    fresh = ctx.matrix_from_host(de.saturated(n0, M))
    want = _observe(ctx, fresh)
    _assert_same(want, _expect_saturated(n0, n0, M), "fresh")
    fresh.close()
    m.resize(n0)
    assert m.n_rows == n0 and np.array_equal(m.download(), de.saturated(n0, M))
    _assert_same(_observe(ctx, m), want, "shrunk")
    for grown in (n1, 2000):          # (700 rows are allocated as 768: 2000 reallocates)
        m.resize(grown)
        back = m.download()
        assert np.array_equal(back[:n0], de.saturated(n0, M)) and not back[n0:].any(), grown
        _assert_same(_observe(ctx, m), _expect_saturated(n0, grown, M), f"grown to {grown}")
    m.resize(n0 + 1)                    # ... and down again from the reallocated buffer, one zero row kept
    _assert_same(_observe(ctx, m), _expect_saturated(n0, n0 + 1, M), "shrunk again")
    m.close()


@pytest.mark.parametrize("n_words", (65, 71, 72, 127))
def test_sources_with_a_wider_stride_leave_the_surplus_words_out(ctx, n_words):
    """"Words >= n_words are zero": upload, import and the uploading pass from sources whose row stride is n_words + 3 with
    all-ones in the surplus words give what the rows alone give (n_words = 1, 7, 8, 63 mod 64: the matrix's own padding is
    63, 57, 56 and 1 words)."""
    import torch
    M, N = 64 * n_words, 2304              # (the uploading pass multiplies panel by panel from 2048 rows)
    L = de.staircase_lengths(M, cut_chunks=(1, n_words // 8))
    S = [0, 1, 63, 64, 65, 512, M - 1, M]
    pre, suf = _cycle(L, 1500), _cycle(S, N - 1500)
    mat = de.staircase(M, pre, suf)
    n_i, _, cnt = de.staircase_counts(M, pre, suf)
    want_total = int(np.triu(cnt, k=1).sum())
    want300 = np.triu(cnt[:300, :300], k=1).astype(np.uint32)
    wide = np.full((N, n_words + 3), de.ALL, dtype=np.uint64)
    wide[:, :n_words] = mat

    def check(m, how):
        assert np.array_equal(m.download(), mat), how
        assert np.array_equal(m.row_counts(), n_i), how
        assert m.pairw() == want_total == m.column_identity(), how
        for operands in (2, 4):
            _set(ctx, k2_strip_operands=operands)
            assert m.pairw() == want_total, (how, operands)
        _set(ctx, k2_strip_operands=0, variant=2)
        assert m.pairw() == want_total, (how, "popcount")
        _set(ctx, variant=-1)

    m = ctx.matrix(N, n_words)
    m.upload(wide)
    check(m, "upload")
    m.clear()
    dev = torch.from_numpy(wide.view(np.int64)).to("cuda:0")
    m.import_device(dev.data_ptr(), N, n_words + 3)
    ctx.synchronize()
    check(m, "import")
    m.clear()
    assert m.pairw_upload(wide) == want_total and ctx.get_option("variant_used") == 4
    check(m, "pairw_upload")
    m.close()
    small = ctx.matrix(300, n_words)
    small.upload(wide[:300])
    assert small.pairw_upload(wide[:300]) == int(want300.sum(dtype=np.uint64))
    for tile_shape in (5, 6):
        _set(ctx, k2_tile_shape=tile_shape)
        got = small.pairw_matrix("and")
        assert np.array_equal(got, want300), (tile_shape, _first_diffs(want300, got))
    small.close()


def test_positions_at_both_ends_of_the_first_and_last_row(ctx):
    """set_rows_from_positions with positions 0 and 64 n_words - 1 on the first and the last row, nothing in between."""
    for n_rows, n_words in ((130, 65), (257, 8), (300, 127)):
        last = 64 * n_words - 1
        m = ctx.matrix(n_rows, n_words)
        m.set_rows_from_positions([[0, last]] + [[] for _ in range(n_rows - 2)] + [[0, last]])
        want = np.zeros((n_rows, n_words), dtype=np.uint64)
        for r in (0, n_rows - 1):
            want[r, 0] |= np.uint64(1)
            want[r, -1] |= np.uint64(1) << np.uint64(63)
        assert np.array_equal(m.download(), want)
        assert m.pairw() == 2 == m.column_identity()
        pm = m.pairw_matrix("and")
        assert pm[0, n_rows - 1] == 2 and int(pm.sum()) == 2
        m.close()


# =========================================================================================================================
# case 7
# =========================================================================================================================
def _placement_inputs():
    M, N = 40 * 64, 300
    L = de.staircase_lengths(M, cut_chunks=(2, 3))
    S = [0, 1, 63, 64, 65, 511, 512, 513, M - 1, M]
    pre, suf = _cycle(L, 190), _cycle(S, N - 190)
    # (a rotation of the lengths per row block, so that a row or column misplaced by a multiple of the list's period shows too)
    pre = [pre[(i + i // 64) % len(pre)] for i in range(len(pre))]
    return M, N, pre, suf


def _run_into(torch, fn, rows, ld, offset_words, want_of):
    """Calls fn(address) on a device buffer of rows x ld uint32 pre-filled with the sentinel that starts `offset_words` words
    into a 16-byte aligned allocation, and compares the WHOLE buffer (and the words around it) with want_of(sentinel-filled array)."""
    buf = torch.full((rows * ld + 8,), _sentinel_i32(), dtype=torch.int32, device="cuda:0")
    assert buf.data_ptr() % 16 == 0
    fn(buf.data_ptr() + 4 * offset_words)
    got = buf.cpu().numpy().view(np.uint32)
    want = np.full(rows * ld + 8, SENTINEL, dtype=np.uint32)
    body = want[offset_words:offset_words + rows * ld].reshape(rows, ld)
    want_of(body)
    if not np.array_equal(got, want):
        g = got[offset_words:offset_words + rows * ld].reshape(rows, ld)
        outside = np.flatnonzero(np.concatenate([got[:offset_words], got[offset_words + rows * ld:]]) != SENTINEL)
        raise AssertionError((_first_diffs(body, g), "words touched outside the buffer:", outside[:4].tolist()))


# (k2_tile_shape, further options, the whole loop or the reduced one). Every kernel that writes a caller's window stands here:
# 5 tilering_kernel<false> (and <true> under k2_ring_sync), 6 tile128_kernel, 2 tilebits8_kernel, 3 / 4 tile16_bits_kernel /
# tile32_bits_kernel, 32 expand_fp4_kernel + pairw_fp4_kernel<0, true>. The rows are 20 stages of 128 bits, so the tiles are
# cut along k only under k2_matrix_min_part = 4 (default 32): then the parts add into the window zero_tiles_kernel cleared
# or, with k2_matrix_parts = 1, write windows of their own that reduce_parts_kernel adds up.
_PLACEMENT_CASES = [
    pytest.param(5, {}, True, id="5"), pytest.param(6, {}, True, id="6"), pytest.param(2, {}, True, id="2"),
    pytest.param(3, {}, False, id="3"), pytest.param(4, {}, False, id="4"), pytest.param(32, {}, False, id="32"),
    pytest.param(5, {"k2_ring_sync": 1}, False, id="5-ring_sync"),
    pytest.param(2, {"k2_matrix_parts": 1, "k2_matrix_min_part": 4}, False, id="2-matrix_parts"),
    pytest.param(5, {"k2_matrix_parts": 1, "k2_matrix_min_part": 4}, False, id="5-matrix_parts"),
    pytest.param(5, {"k2_matrix_min_part": 4}, False, id="5-cleared_window"),
]


@pytest.mark.parametrize("tile_shape,options,whole", _PLACEMENT_CASES)
def test_device_outputs_touch_only_what_the_header_says(ctx, tile_shape, options, whole):
    """storm_hip_pairw_matrix_device, _band_device and storm_hip_square_matrix_device write out[i * ld + j] for i < j (every
    i, j of a rectangle) and leave everything else untouched: entries on and below the diagonal, the columns from n_rows (B's
    rows) up to ld. Outputs pre-filled with a sentinel, ld = 0, 1, 3 (mod 4), a 16-byte aligned address and one 4 bytes
    further (tile128_kernel's 16-byte row stores have a scalar fall-back selected by exactly these), bands from row 0, 1,
    63, 64, 127, 129, a band of 0 rows, a band that ends at the last row, rectangles whose B has 1, 63, 257 rows. Staircase
    rows: a misplaced row or column shows as a wrong VALUE, not only as a touched sentinel. The cases beyond the three default
    forms run the reduced loop: both ops, ld = 0 and 3 (mod 4), both addresses, the first three bands, the rectangles of 200
    rows against 63 and 257."""
    import torch
    if tile_shape not in shipped(ctx, "k2_tile_shape", (tile_shape,)):
        pytest.skip("this build of the library does not carry the form")
    M, N, pre, suf = _placement_inputs()
    mat = de.staircase(M, pre, suf)
    n_i, _, cnt = de.staircase_counts(M, pre, suf)
    m = ctx.matrix_from_host(mat)
    _set(ctx, k2_tile_shape=tile_shape, **options)
    for op in ("and", "xor"):
        full = de.op_counts(n_i, n_i, cnt, op)
        for ld in ((N, N + 1, N + 3, N + 8) if whole else (N, N + 3)):
            for offset in (0, 1):
                what = (tile_shape, op, ld, offset)

                def triangle(body, row0=0, rows=N):
                    for r in range(rows):
                        body[r, row0 + r + 1:N] = full[row0 + r, row0 + r + 1:N]

                try:
                    _run_into(torch, lambda p: m.pairw_matrix_device(p, ld, op), N, ld, offset, triangle)
                    assert ctx.get_option("k2_tile_shape_used") == tile_shape
                    bands = [(0, 100), (1, 64), (63, 66), (64, 64), (127, 130), (129, 40), (50, 0), (N - 37, 37), (0, N)]
                    for row0, rows in (bands if whole and (op, offset) != ("xor", 1) else bands[:3]):
                        what = (tile_shape, op, ld, offset, "band", row0, rows)
                        _run_into(torch, lambda p: m.pairw_matrix_band_device(p, ld, row0, rows, op), max(rows, 1), ld, offset,
                                  lambda body: triangle(body, row0, rows))
                except AssertionError as e:
                    raise AssertionError((what,) + e.args) from None
    for nb in ((1, 63, 257) if whole else (63, 257)):
        b = ctx.matrix_from_host(mat[N - nb:])
        for na in ((1, 200) if whole else (200,)):
            a = ctx.matrix_from_host(mat[:na])
            for op in ("and", "or"):
                full = de.op_counts(n_i[:na], n_i[N - nb:], cnt[:na, N - nb:], op)
                for ld in ((nb, nb + 1, nb + 3, (nb + 3) // 4 * 4 + 4) if whole else (nb, nb + 3)):
                    for offset in (0, 1):
                        def rectangle(body):
                            body[:, :nb] = full
                        try:
                            _run_into(torch, lambda p: _square_matrix_device(ctx, a, b, p, ld, op), na, ld, offset, rectangle)
                        except AssertionError as e:
                            raise AssertionError(((tile_shape, "rectangle", na, nb, op, ld, offset),) + e.args) from None
                        assert ctx.get_option("k2_tile_shape_used") == tile_shape
            a.close()
        b.close()
    m.close()


def test_empty_shapes(ctx):
    """storm_hip.h: a matrix of fewer than two rows has no pairs and a rectangle with an empty side no entries — the calls
    succeed, write nothing (the host form of a one-row matrix returns its single 0) and the totals are 0."""
    import torch
    sentinel = torch.full((16,), _sentinel_i32(), dtype=torch.int32, device="cuda:0")
    for tile_shape in (0, 5, 6):
        _set(ctx, k2_tile_shape=tile_shape)
        for n_rows in (0, 1):
            m = ctx.matrix(n_rows, 9)
            if n_rows:
                m.upload(de.saturated(1, 9 * 64))
            assert m.pairw() == 0 and m.pairw_op("or") == 0 and m.column_identity() == 0
            assert m.pairw_matrix("and").shape == (n_rows, n_rows) and not m.pairw_matrix("or").any()
            m.pairw_matrix_device(sentinel.data_ptr(), 4, "and")
            m.pairw_matrix_band_device(sentinel.data_ptr(), 4, 0, n_rows, "xor")
            other = ctx.matrix_from_host(de.saturated(3, 9 * 64))
            if n_rows == 0:
                assert m.square(other) == 0 == other.square(m)
                assert m.square_matrix(other, "and").shape == (0, 3) and other.square_matrix(m, "and").shape == (3, 0)
                _square_matrix_device(ctx, m, other, sentinel.data_ptr(), 4, "and")
                _square_matrix_device(ctx, other, m, sentinel.data_ptr(), 4, "and")
            else:
                assert m.square(other) == 3 * 9 * 64 and np.array_equal(other.square_matrix(m, "or"), np.full((3, 1), 9 * 64))
            assert (sentinel.cpu().numpy().view(np.uint32) == SENTINEL).all(), (tile_shape, n_rows)
            other.close()
            m.close()


def test_every_option_reads_back():
    """On a fresh context every key of the option table reads its member's initialiser; after set_option with a legal
    non-default value it reads what was stored (clamped, normalised); unknown names read -1."""
    from tests.test_plan_golden import gen
    assert set(gen.OPTIONS) == set(DEFAULTS)
    stored_as = {"k2_matrix_pad": (100, 64), "k2_fold_inline": (7, 1), "matrix_lists_debug": (3, 3)}
    fresh = sb.HipContext(0)
    try:
        for key, default in DEFAULTS.items():
            assert fresh.get_option(key) == default, key
        assert fresh.get_option("no_such_option") == -1
        for key, (kind, a, b, tools_only) in gen.OPTIONS.items():
            default = DEFAULTS[key]
            if key in stored_as:
                value, want = stored_as[key]
            elif kind == "any":   # a boolean
                value = 5 if default == 0 else 0
                want = int(value != 0)
            else:
                legal = [v for v in ((a, b, a + 1, b - 1) if kind == "range" else a) if v not in tools_only and v != default]
                if key == "k2_stream_max_rows":
                    legal = [0]   # (2^31 is accepted and does not fit the int it is stored in)
                value = want = legal[0] if legal else None
            if value is None or want in tools_only:
                continue   # (k2_ring, k2_shape, k2_persistent, k2_debug: the shipped build takes the default alone)
            fresh.set_option(key, value)
            assert fresh.get_option(key) == want, (key, value)
        for key, default in DEFAULTS.items():
            fresh.set_option(key, default)
            assert fresh.get_option(key) == default, key
    finally:
        fresh.close()
