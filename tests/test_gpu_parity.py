"""Parity of the HIP path against the CPU oracle, the committed golden vectors and the totals
SURVEY.md recorded from the reference — every call goes through the C-ABI of libstorm_hip.so.
Bit-exact: all quantities are integers. Run on the GPU box with `pytest -m gpu`."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests.conftest import shipped

import stormbitmaps_amd as sb
from stormbitmaps_amd import synth

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _load(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


def test_device_is_gfx950(lib):
    assert lib.storm_hip_device_count() >= 1
    buf = C.create_string_buffer(64)
    assert lib.storm_hip_device_arch(0, buf, 64) == 0
    assert buf.value.startswith(b"gfx950")


@pytest.mark.parametrize("case", _load("tiny.json")["cases"], ids=lambda c: c["name"])
def test_hand_computed_matrices(case):
    c = sb.StormContig(case["M"])
    s = sb.Storm()
    for r in case["rows"]:
        assert c.add(r) == len(r)
        assert s.add(r) == 1
    want = case["total"]
    assert c.pairw_intersect_cardinality() == want
    assert c.pairw_intersect_cardinality_blocked(31) == want
    assert c.pairw_intersect_cardinality_list() == want
    assert c.pairw_intersect_cardinality_blocked_list(5) == want
    assert s.pairw_intersect_cardinality() == want
    assert s.pairw_intersect_cardinality_blocked(0) == want
    # per-pair matrices (AND / OR / XOR) against the fixture's set arithmetic
    n = sum(1 for r in case["rows"] if len(r))       # empty rows are not appended (storm.c:1034)
    if n == len(case["rows"]) and n >= 1:
        for name in ("and", "or", "xor"):
            assert c.n_rows == n
            got = c.pairw_matrix(name)
            for i, j, cnt in case["pair_counts"][name]:
                assert got[i, j] == cnt and got[j, i] == 0, (name, i, j)


@pytest.mark.parametrize("case", _load("survey_totals.json")["agree"],
                         ids=lambda c: f"M{c['M']}_N{c['N']}_d{c['draws']}")
def test_reference_totals_recorded_by_survey(orc, case):
    rows = orc.mt_positions(case["M"], case["N"], case["draws"], 42)
    c = sb.StormContig(case["M"])
    s = sb.Storm()
    for r in rows:
        c.add(r)
        s.add(r)
    optimal_b = max(5, 256000 // (((case["M"] + 63) // 64) * 8))  # benchmark.cpp:823-824
    got = [c.pairw_intersect_cardinality(), c.pairw_intersect_cardinality_blocked(optimal_b),
           c.pairw_intersect_cardinality_list(), c.pairw_intersect_cardinality_blocked_list(optimal_b),
           s.pairw_intersect_cardinality(), s.pairw_intersect_cardinality_blocked(0)]
    assert got == [case["total"]] * 6


@pytest.mark.parametrize("case", _load("survey_totals.json")["defects"],
                         ids=lambda c: f"{c['id']}_d{c['draws']}")
def test_truth_in_the_reference_defect_regimes(orc, case):
    rows = orc.mt_positions(case["M"], case["N"], case["draws"], 42)
    if case["container"] == "STORM_t":
        s = sb.Storm()
        for r in rows:
            s.add(r)
        assert s.pairw_intersect_cardinality_blocked(0) == case["truth"]
    else:
        c = sb.StormContig(case["M"])
        for r in rows:
            c.add(r)
        assert c.pairw_intersect_cardinality_blocked(31) == case["truth"]
        assert c.pairw_intersect_cardinality_list() == case["truth"]


@pytest.mark.parametrize("case", _load("synth_totals.json")["dense"], ids=lambda c: c["name"])
def test_dense_golden_vectors(hip_ctx, case):
    mat = synth.dense_matrix_c(case["M"], case["N"], case["draws"], seed=42)
    m = hip_ctx.matrix_from_host(mat)
    try:
        for variant in shipped(hip_ctx, "variant", (2, 0, 1, 3, 4, 5)):  # 3/4 = K2, the FP4 matrix-core paths
            hip_ctx.set_option("variant", variant)
            assert m.pairw() == case["total"], f"variant {variant}"
    finally:
        hip_ctx.set_option("variant", -1)
        m.close()
    assert sb.wrapper_diag(mat) == case["total"]
    assert sb.wrapper_diag_blocked(mat, 31) == case["total"]


@pytest.mark.parametrize("case", _load("synth_totals.json")["sparse"], ids=lambda c: c["name"])
def test_sparse_golden_vectors(lib, hip_ctx, case):
    rows = synth.positions_from_dense(synth.dense_matrix_c(case["M"], case["N"], case["draws"], seed=42))
    s = sb.Storm()
    for r in rows:
        s.add(r)
    assert s.serialized_size() == case["serialized_size"]
    assert s.pairw_intersect_cardinality_blocked(0) == case["total"]
    assert s.pairw_intersect_cardinality() == case["total"]


@pytest.mark.parametrize("M,N,d,seed", [(4096, 300, 2048, 1), (1000, 131, 300, 2), (65536, 513, 9000, 3),
                                        (200, 5, 40, 4), (64, 2, 64, 5), (8256, 260, 4000, 6)])
def test_against_oracle_on_fresh_seeds(hip_ctx, orc, M, N, d, seed):
    mat = synth.dense_matrix_c(M, N, d, seed=seed)
    want = orc.wrapper_diag_blocked(mat, 31)
    assert want == orc.truth_columns(mat)
    m = hip_ctx.matrix_from_host(mat)
    assert m.pairw() == want
    assert m.column_identity() == want
    # per-pair values of a few tiles, including one on the diagonal
    for (i0, i1, j0, j1) in ((0, min(N, 40), 0, min(N, 40)), (0, min(N, 17), max(0, N - 33), N)):
        assert np.array_equal(m.tile_counts(i0, i1, j0, j1), orc.tile_counts(mat, i0, i1, j0, j1))
    m.close()


def test_empty_and_degenerate_shapes(hip_ctx):
    for n in (0, 1):
        m = hip_ctx.matrix(n, 64)
        assert m.pairw() == 0
        m.close()
    mat = np.full((2, 1), np.uint64(0xFFFFFFFFFFFFFFFF))
    m = hip_ctx.matrix_from_host(mat)
    assert m.pairw() == 64
    m.close()
    # all-ones rows: every pair counts M bits (largest per-pair value at this width)
    mat = np.full((130, 70), np.uint64(0xFFFFFFFFFFFFFFFF))
    m = hip_ctx.matrix_from_host(mat)
    assert m.pairw() == 130 * 129 // 2 * 70 * 64
    m.close()
    c = sb.StormContig(4096)
    assert c.pairw_intersect_cardinality() == 0
    c.add([1, 2])
    assert c.pairw_intersect_cardinality_blocked(31) == 0


def test_bad_arguments_fail_loudly(lib, hip_ctx):
    m = hip_ctx.matrix(4, 8)
    out = C.c_uint64()
    assert lib.storm_hip_pairw_dense(hip_ctx._h, m._h, 2, 2, C.byref(out)) == -1
    assert b"shard" in lib.storm_hip_last_error()
    assert lib.storm_hip_pairw_dense(hip_ctx._h, None, 0, 1, C.byref(out)) == -1
    assert lib.storm_hip_pairw_dense(None, m._h, 0, 1, C.byref(out)) == -1
    assert lib.storm_hip_ctx_set_option(hip_ctx._h, b"variant", 9) == -1
    mat = np.zeros((4, 8), dtype=np.uint64)
    # a foreign leaf pointer cannot run on the device
    foreign = C.cast(lib.STORM_get_alignment, C.c_void_p)
    assert lib.STORM_wrapper_diag(4, mat.ctypes.data, 8, foreign) == 2**64 - 1
    ours = lib.STORM_get_intersect_count_func(8)
    assert lib.STORM_wrapper_diag(4, mat.ctypes.data, 8, ours) == 0
    m.close()


def test_device_synthetic_fill_equals_host_generator(hip_ctx):
    for M, N, d in ((4096, 300, 2048), (65536, 64, 32768), (1000, 50, 77)):
        m = hip_ctx.matrix(N, (M + 63) // 64)
        m.fill_synthetic(M, d, seed=42)
        assert np.array_equal(m.download(), synth.dense_matrix_c(M, N, d, seed=42))
        m.close()


def test_device_side_construction_from_positions(hip_ctx, orc):
    M, N, d = 5000, 140, 600
    rows = synth.positions(M, N, d, seed=8)
    m = hip_ctx.matrix(N, (M + 63) // 64)
    m.set_rows_from_positions(rows)
    mat = synth.dense_matrix_c(M, N, d, seed=8)
    assert np.array_equal(m.download(), mat)
    assert m.pairw() == orc.wrapper_diag(mat)
    m.close()


@pytest.mark.parametrize("variant", [2, 3, 4])
def test_shards_partition_the_pair_space(hip_ctx, variant):
    mat = synth.dense_matrix_c(8192, 1100, 3000, seed=9)
    m = hip_ctx.matrix_from_host(mat)
    total = m.pairw()
    hip_ctx.set_option("variant", variant)
    try:
        assert m.pairw() == total
        for world in (2, 3, 8):
            parts = [m.pairw(r, world) for r in range(world)]
            assert sum(parts) == total and max(parts) < total
    finally:
        hip_ctx.set_option("variant", -1)
    m.close()


def test_matrix_core_path_k_slicing_and_edges(hip_ctx, orc):
    """K2 (variant 3): every k-slice length, ragged row counts around the 256-row tile edge,
    all-ones rows (largest f32 accumulator values), and a diagonal-only problem."""
    try:
        for variant, n in ((4, 257), (4, 700), (4, 1025)):
            hip_ctx.set_option("variant", variant)
            mat = synth.dense_matrix_c(9000, n, 4000, seed=n)
            m = hip_ctx.matrix_from_host(mat)
            assert m.pairw() == orc.wrapper_diag_blocked(mat, 31), (variant, n)
            m.close()
        hip_ctx.set_option("variant", 3)
        for n in (2, 255, 256, 257, 513):
            mat = synth.dense_matrix_c(9000, n, 4000, seed=n)
            m = hip_ctx.matrix_from_host(mat)
            want = orc.wrapper_diag_blocked(mat, 31)
            for spi in (1, 3, 32, 1000):
                hip_ctx.set_option("k2_stages_per_item", spi)
                assert m.pairw() == want, (n, spi)
            m.close()
        hip_ctx.set_option("k2_stages_per_item", 32)
        mat = np.full((300, 130), np.uint64(0xFFFFFFFFFFFFFFFF))
        m = hip_ctx.matrix_from_host(mat)
        assert m.pairw() == 300 * 299 // 2 * 130 * 64
        m.close()
    finally:
        hip_ctx.set_option("variant", -1)
        hip_ctx.set_option("k2_stages_per_item", 32)


def test_auto_variant_selection(hip_ctx):
    hip_ctx.set_option("variant", -1)
    small = hip_ctx.matrix_from_host(synth.dense_matrix_c(4096, 300, 900, seed=3))
    assert small.pairw() == small.column_identity()
    assert hip_ctx.get_option("variant_used") == 4       # strips win from N = 64 up (bench_crossover)
    big = hip_ctx.matrix_from_host(synth.dense_matrix_c(4096, 1500, 900, seed=3))
    got = big.pairw()
    assert hip_ctx.get_option("variant_used") == 4       # matrix-core strips
    assert got == big.column_identity()
    small.close()
    big.close()


def test_tiling_options_do_not_change_the_result(hip_ctx):
    mat = synth.dense_matrix_c(16384, 700, 5000, seed=10)
    m = hip_ctx.matrix_from_host(mat)
    base = m.pairw()
    hip_ctx.set_option("variant", 2)
    try:
        for seg_rows in (32, 100, 256, 1024):
            for cps in (0, 1, 3, 4):
                hip_ctx.set_option("seg_rows", seg_rows)
                hip_ctx.set_option("chunks_per_item", cps)
                assert m.pairw() == base, (seg_rows, cps)
    finally:
        hip_ctx.set_option("seg_rows", 256)
        hip_ctx.set_option("chunks_per_item", 0)
        hip_ctx.set_option("variant", -1)
        m.close()


def test_square_and_additivity(hip_ctx, orc):
    mat = synth.dense_matrix_c(4096, 700, 1500, seed=12)
    a, b = mat[:300], mat[300:]
    ma, mb, mall = (hip_ctx.matrix_from_host(x) for x in (a, b, mat))
    sq = ma.square(mb)
    assert sq == orc.wrapper_square(a, b) == sb.wrapper_square(a, b)
    assert mall.pairw() == ma.pairw() + mb.pairw() + sq
    for x in (ma, mb, mall):
        x.close()


def test_headline_shape_properties(hip_ctx):
    """BASELINE config 2 at full size (N=10000, M=65536, dense): the CPU pairwise oracle would
    need ~10-30 s per leaf here, so the full-size checks are size-independent properties; the
    first 2000 rows are additionally pinned by the committed oracle vector."""
    M, N, d = 65536, 10000, 32768
    m = hip_ctx.matrix(N, M // 64)
    m.fill_synthetic(M, d, seed=42)
    total = m.pairw()
    assert total == m.column_identity()                      # sum_c C(n_c, 2)
    assert sum(m.pairw(r, 8) for r in range(8)) == total      # 8-way shard partition
    try:
        for variant in shipped(hip_ctx, "variant", (0, 3, 4, 5)):        # independent operand paths
            hip_ctx.set_option("variant", variant)
            assert m.pairw() == total, variant
    finally:
        hip_ctx.set_option("variant", -1)
    head = hip_ctx.matrix(2000, M // 64)
    head.import_device(m.device_ptr, 2000, m.stride_words)
    gold = {c["name"]: c["total"] for c in _load("synth_totals.json")["dense"]}
    assert head.pairw() == gold["c2_first2000"]
    tail = hip_ctx.matrix(N - 2000, M // 64)
    tail.import_device(m.device_ptr + 2000 * m.stride_words * 8, N - 2000, m.stride_words)
    assert total == head.pairw() + tail.pairw() + head.square(tail)
    for x in (m, head, tail):
        x.close()


def test_wide_shape_properties(hip_ctx, orc):
    """BASELINE config 3 shape (N=10000, M=524288, dense, 655 MB in HBM)."""
    M, N, d = 524288, 10000, 262144
    m = hip_ctx.matrix(N, M // 64)
    m.fill_synthetic(M, d, seed=42)
    total = m.pairw()
    assert total == m.column_identity()
    try:
        for variant in shipped(hip_ctx, "variant", (3, 4, 5)):
            hip_ctx.set_option("variant", variant)
            assert m.pairw() == total, variant
    finally:
        hip_ctx.set_option("variant", -1)
    head = hip_ctx.matrix(300, M // 64)
    head.import_device(m.device_ptr, 300, m.stride_words)
    gold = {c["name"]: c["total"] for c in _load("synth_totals.json")["dense"]}
    assert head.pairw() == gold["c3_first300"]
    # a sampled block of rows from the middle of the matrix, pair by pair on the CPU (the loop being matched:
    # storm.c:1199-1238 with the harness's block size for this width, benchmark.cpp:823-824), as c5 has it below
    sub = m.download(7000, 192)
    want = orc.wrapper_diag_blocked(sub, max(5, 256000 // (M // 64 * 8)))
    sm = hip_ctx.matrix_from_host(sub)
    assert sm.pairw() == want == sm.column_identity()
    assert np.array_equal(m.tile_counts(7000, 7008, 7100, 7116), orc.tile_counts(sub, 0, 8, 100, 116))
    assert sum(m.pairw(r, 8) for r in range(8)) == total
    for x in (m, head, sm):
        x.close()


def test_sparse_container_against_dense_identity(hip_ctx):
    """STORM_t at several densities, N=2000 x M=524288: the sparse device path (K2s on the block
    columns at this size) must equal the dense device path and the column identity on the same
    bits; list-kind and bitmap-kind blocks both occur."""
    M, N = 524288, 2000
    for d in (1, 5, 524, 5242, 33000, 131072):
        m = hip_ctx.matrix(N, M // 64)
        m.fill_synthetic(M, d, seed=42)
        want = m.column_identity()
        assert m.pairw() == want
        m.close()
        s = sb.Storm()
        assert s.add_synthetic(M, N, d, seed=42) == N
        assert s.pairw_intersect_cardinality_blocked(0) == want, d
        assert s.pairw_intersect_cardinality() == want, d
        s.free()


def test_sparse_arena_kernel_variants(lib, hip_ctx, orc):
    """The sparse C-ABI directly, every kernel variant, on mixed block kinds."""
    import ctypes as C
    M, N, d = 196608, 800, 12690    # ~4230 draws per 65536-bit block: list and bitmap kinds mix
    rows = synth.positions(M, N, d, seed=7)
    want = orc.storm(rows).pairw_blocked(0)
    ids, kinds, offs, lens, lists, words, row_off = [], [], [], [], [], [], [0]
    for r in rows:
        blk = r // 65536
        for b in np.unique(blk):
            v = (r[blk == b] - b * 65536).astype(np.uint16)
            ids.append(b)
            if v.size < 4096:
                kinds.append(0); offs.append(sum(len(x) for x in lists)); lens.append(v.size); lists.append(v)
            else:
                bm = np.zeros(1024, dtype=np.uint64)
                np.bitwise_or.at(bm, (v >> 6).astype(np.int64), np.uint64(1) << (v & 63).astype(np.uint64))
                kinds.append(1); offs.append(1024 * len(words)); lens.append(0); words.append(bm)
        row_off.append(len(ids))
    assert 0 in kinds and 1 in kinds
    arr = lambda x, t: np.ascontiguousarray(np.array(x, dtype=t))  # noqa: E731
    a_off, a_id, a_kind, a_doff, a_len = arr(row_off, np.uint64), arr(ids, np.uint32), arr(kinds, np.uint8), arr(offs, np.uint64), arr(lens, np.uint32)
    a_lists = np.concatenate(lists).astype(np.uint16)
    a_words = np.concatenate(words).astype(np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    h = C.c_void_p()
    assert lib.storm_hip_sparse_create(hip_ctx._h, N, len(ids), p(a_off), p(a_id), p(a_kind), p(a_doff), p(a_len),
                                       p(a_lists), a_lists.size, p(a_words), a_words.size, C.byref(h)) == 0, lib.storm_hip_last_error()
    out = C.c_uint64()
    try:
        for variant in shipped(hip_ctx, "variant", (2, 3, 4, 5, -1)):
            hip_ctx.set_option("variant", variant)
            assert lib.storm_hip_pairw_sparse(hip_ctx._h, h, 0, 1, C.byref(out)) == 0, lib.storm_hip_last_error()
            assert out.value == want, variant
            parts = []
            for r in range(3):
                assert lib.storm_hip_pairw_sparse(hip_ctx._h, h, r, 3, C.byref(out)) == 0
                parts.append(out.value)
            assert sum(parts) == want, (variant, parts)
        census = (C.c_uint64 * 4)()
        assert lib.storm_hip_sparse_last_census(hip_ctx._h, C.byref(census)) == 0
        assert census[3] == 3 and census[0] > 0 and census[1] > 0 and census[2] > 0
    finally:
        hip_ctx.set_option("variant", -1)
        lib.storm_hip_sparse_destroy(hip_ctx._h, h)


def test_genomics_scale_shape_properties(hip_ctx):
    """BASELINE config 5 shape on ONE GPU: N=100000 variants x M=1048576 samples, dense
    (13.1 GB of bits + 52 GB FP4 shadow in HBM; 8.2e13 word pairs). A CPU pairwise oracle would
    need hours, so the total is checked against the column-count identity and
    against shard additivity, and a random row subset is pinned pairwise by the oracle."""
    M, N, d = 1048576, 100000, 524288
    m = hip_ctx.matrix(N, M // 64)
    m.fill_synthetic(M, d, seed=42)
    total = m.pairw()
    assert hip_ctx.get_option("variant_used") == 4
    assert total == m.column_identity()
    assert sum(m.pairw(r, 8) for r in range(8)) == total   # the 8-way partition of BASELINE config 5, every shard
    m.close()


def test_sampled_rows_of_a_large_matrix_against_oracle(hip_ctx, orc):
    M, N, d = 1048576, 20000, 524288
    m = hip_ctx.matrix(N, M // 64)
    m.fill_synthetic(M, d, seed=42)
    # rows 17000..17159 of the big matrix, pairwise on the CPU
    sub = m.download(17000, 160)
    want = orc.wrapper_diag_blocked(sub, 31)
    sm = hip_ctx.matrix_from_host(sub)
    for variant in (2, 3):
        hip_ctx.set_option("variant", variant)
        assert sm.pairw() == want
    hip_ctx.set_option("variant", -1)
    assert np.array_equal(m.tile_counts(17000, 17008, 17100, 17116), orc.tile_counts(sub, 0, 8, 100, 116))
    assert m.pairw() == m.column_identity()
    m.close()
    sm.close()


def test_pcie_inclusive_c_api_call(lib):
    """The storm.h entry point on host-built rows: first call pays the H2D copy, the second runs
    on the cached device mirror; both must give the same total as the raw-buffer wrapper."""
    import time
    M, N, d = 65536, 3000, 32768
    mat = synth.dense_matrix_c(M, N, d, seed=42)
    c = sb.StormContig(M)
    for r in synth.positions_from_dense(mat):
        c.add(r)
    t0 = time.perf_counter(); a = c.pairw_intersect_cardinality_blocked(31); t1 = time.perf_counter()
    b = c.pairw_intersect_cardinality_blocked(31); t2 = time.perf_counter()
    assert a == b == sb.wrapper_diag(mat)
    print(f"first call {1e3 * (t1 - t0):.2f} ms (with H2D), cached call {1e3 * (t2 - t1):.2f} ms")


@pytest.mark.parametrize("ranks", (2, 4))
def test_multi_rank_rehearsal_of_bench_on_one_gpu(ranks):
    """bench.py's multi-rank path end to end with real kernels: the ranks share cuda:0, each
    computes its shard (k-groups) of the pair space, partials are all-reduced (gloo here; the
    driver's N>1 runs use RCCL), and the reduced total must equal the column identity. Four
    ranks on one GPU run at very different speeds: every loop in bench.py that contains a
    collective must make the same number of trips on every rank (a per-rank clock in the
    pre-warm once deadlocked exactly this case)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # the bare form, as the driver calls it: bench.py starts its own ranks (child
    # torch.distributed.run on a free port) and relays the job's one JSON line
    cmd = [sys.executable, os.path.join(root, "bench.py"),
           "--gpus", str(ranks), "--backend", "gloo", "--all-on-device0", "--steps", "5", "--warmup", "1",
           "--rows", "3000", "--no-cpu-baseline", "--full"]
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=root, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == ranks and out["verified_against_column_identity"] is True
    assert out["rccl_ranks"] == ranks and out["collective_backend"] == "gloo"
    assert out["distinct_gpus"] == 1 and all(r["device"] == 0 and r["pci_bus_id"] for r in out["per_rank"])
    assert len({r["pid"] for r in out["per_rank"]}) == ranks
    assert out["config"]["kernel_variant"] == 4
    assert "shadow_resident" not in out   # the default path (K2b) has no FP4 shadow to keep
    assert out["roofline"]["kernel"] == "storm::strip16_bits_kernel"
    # the per-rank diagnostics a scaling run is read by
    assert [r["rank"] for r in out["per_rank"]] == list(range(ranks))
    assert all(r["kernel_ms"] > 0 and r["work_items"] > 0 for r in out["per_rank"])
    assert 0 < out["roofline"]["frac_whole_pass"] <= out["roofline"]["frac"] * 1.05
    # at N > 1 the dominant kernel is bracketed on every 4th timed step: steps 0 (.. 4, 8) of the 5
    assert out["roofline"]["kernel_ms_samples"] == 2


def test_plain_bench_prints_the_headline_and_dumps_the_timed_total(tmp_path):
    """A plain `bench.py` run (no --full) prints the headline line only, and --dump-outputs writes what the
    last timed step returned: the all-pairs total, which must be the column identity of the same seeded matrix."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    N, M = 3000, 65536
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--rows", str(N), "--bits", str(M), "--dump-outputs", str(tmp_path / "out")],
                         capture_output=True, text=True, timeout=240, cwd=root, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["unit"] == "words/s" and out["higher_is_better"] is True and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(N * (N - 1) // 2 * 2 * (M // 64) * 1e3 / out["ms_per_step"], rel=1e-9)
    assert not {"roofline", "cpu_baseline", "shadow_resident", "per_rank", "verified_against_column_identity"} & set(out)
    dumped = np.load(tmp_path / "out" / "total.npy")
    assert dumped.dtype == np.float64 and dumped.shape == (1,) and int(dumped[0]) == out["total"]
    ctx = sb.HipContext(0)
    try:
        m = ctx.matrix(N, M // 64)
        m.fill_synthetic(M, M // 2, seed=42)
        assert out["total"] == m.column_identity()
        m.close()
    finally:
        ctx.close()


def test_bench_over_rccl_when_the_box_has_two_gpus():
    """The first multi-GPU box must carry a rank > 0 over RCCL inside the suite, not only in the
    driver's scaling run: `python bench.py --gpus 2` (bare; bench.py starts the ranks), backend
    nccl = RCCL over xGMI, one GPU per rank. Skipped on 1-GPU boxes (RCCL refuses two ranks on
    one device)."""
    import subprocess
    import sys
    n_dev = sb.load().storm_hip_device_count()
    if n_dev < 2:
        pytest.skip(f"{n_dev} GPU visible: RCCL needs one GPU per rank")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "10",
                          "--warmup", "2", "--full"], capture_output=True, text=True, timeout=600, cwd=root, env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["rccl_ranks"] == 2 and out["collective_backend"] == "nccl"
    assert out["distinct_gpus"] == 2 and [r["device"] for r in out["per_rank"]] == [0, 1]
    assert out["verified_against_column_identity"] is True
    assert out["total"] == 507277197315          # c2: the CPU oracle's pair-by-pair sum (BENCH_r02.json cpu_baseline.sample_total)


def test_benchmark_cli_rows_agree_with_golden_totals():
    """tools/storm_benchmark.cpp = the reference's `benchmark <M> <N> [loads]` CLI on this library:
    every method row of one load must report the same total (that is the reference's only
    correctness signal), and the totals must equal the committed oracle vectors."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "stormbitmaps_amd", "storm_benchmark")
    gold = {(c["M"], c["N"], c["draws"]): c["total"] for c in _load("synth_totals.json")["dense"]}
    for M, N, loads, methods in ((4096, 256, "2048,40,5", 3), (65536, 700, "32768,262,1", 5)):
        res = subprocess.run([exe, str(M), str(N), loads, "--reps", "2", "--cpu-seconds", "0.05"], capture_output=True,
                             text=True, timeout=600)
        assert res.returncode == 0, res.stderr
        lines = res.stdout.strip().splitlines()
        assert lines[0].startswith("Samples\tAlts\tMethod")
        assert lines[1].startswith("#Method\tAlts\t") and lines[1].endswith("rows_per_lookup\tnote")
        cols = lines[1].split("\t")
        rows = [dict(zip(cols, l.split("\t"))) for l in lines[2:]]
        assert all(len(l.split("\t")) == len(cols) for l in lines[2:])
        gpu_rows = [r for r in rows if int(r["GPUs"]) > 0]
        cpu_rows = [r for r in rows if int(r["GPUs"]) == 0]
        # every GPU row: priced against the roof of the kernel that ran, never above it; one call timed first
        for r in gpu_rows:
            assert r["kernel"] != "-" and r["roof"] != "-", r
            assert 0.0 <= float(r["roof_frac"]) <= 1.0, r
            assert float(r["time_ms"]) == float(r["first_call_ms"]) > 0 and float(r["steady_ms"]) > 0
            assert float(r["cycles"]) > 0 and float(r["cycles_word"]) > 0
        # the host rows: the library's own SIMD leaves under the harness's blocked loop (a row sample)
        assert {r["#Method"].split("-")[1] for r in cpu_rows} >= {"scalar"}
        assert all("==" in r["note"] and "extrapolated" in r["note"] for r in cpu_rows), cpu_rows
        # [r5] the reference's STORM_t host path (benchmark.cpp:605-613) and its list-probe row (:1039-1045, loads <= 300),
        # over the library's own exported one-pair helpers
        cpu_names = {(r["#Method"], int(r["Alts"])) for r in cpu_rows}
        for load in (int(x) for x in loads.split(",")):
            assert (("storm-blocked-cpu", load) in cpu_names) == (M >= 65536), (M, load, cpu_names)
            assert (("bitmap-scalar-skip-list", load) in cpu_names) == (load <= 300), (M, load, cpu_names)
        for load in (int(x) for x in loads.split(",")):
            totals = {int(r["total"]) for r in gpu_rows if int(r["Alts"]) == load}
            names = [r["#Method"] for r in gpu_rows if int(r["Alts"]) == load]
            assert len(names) == methods, names
            assert totals == {gold[(M, N, load)]}, (M, N, load, totals)
            if N <= 256:   # the CPU sample is the whole matrix: its total is the matrix's
                assert {int(r["total"]) for r in cpu_rows if int(r["Alts"]) == load} <= {gold[(M, N, load)]}


def test_repeated_launches_are_stable(hip_ctx):
    """Race screen for the hand-synchronised LDS rings: 30 back-to-back launches of every MFMA
    variant on the headline shape must all give the identity's total (a wrong vmcnt count showed
    up here as a 5e-7 relative error in 1 launch out of a few)."""
    M, N, d = 65536, 10000, 32768
    m = hip_ctx.matrix(N, M // 64)
    m.fill_synthetic(M, d, seed=43)
    want = m.column_identity()
    try:
        for variant in shipped(hip_ctx, "variant", (5, 4, 3, 2)):
            hip_ctx.set_option("variant", variant)
            got = {m.pairw() for _ in range(30 if variant != 2 else 5)}
            assert got == {want}, (variant, got, want)
    finally:
        hip_ctx.set_option("variant", -1)
        m.close()


def test_in_process_multi_device_sharding_through_the_c_api(lib):
    """STORM_hip_set_devices(): the storm.h entry points shard one call over several contexts and
    add the partials on the host. With one GPU in the box the device list is [0, 0, 0]: three
    contexts, three replicas, three disjoint shards."""
    import ctypes as C
    M, N, d = 65536, 2600, 9000
    c = sb.StormContig(M)
    assert c.add_synthetic(N, d, seed=5) == N
    one = c.pairw_intersect_cardinality_blocked(31)
    ids = (C.c_int * 3)(0, 0, 0)
    try:
        assert lib.STORM_hip_set_devices(3, ids) == 0
        c2 = sb.StormContig(M)
        assert c2.add_synthetic(N, d, seed=5) == N
        assert c2.pairw_intersect_cardinality_blocked(31) == one
        assert c2.pairw_intersect_cardinality() == one
        mat = synth.dense_matrix_c(M, 300, d, seed=5)
        assert sb.wrapper_diag(mat) == sb.HipContext(0).matrix_from_host(mat).pairw()
        c2.free()
    finally:
        one_dev = (C.c_int * 1)(0)
        assert lib.STORM_hip_set_devices(1, one_dev) == 0
    c.free()


def test_materialised_upper_triangle(hip_ctx, orc):
    """the per-pair matrix the reference only sums. Every entry i < j must equal the
    oracle's pair count, entries i >= j stay 0, and the matrix sums to the all-pairs total."""
    for M, N, d in ((9000, 700, 4000), (4096, 257, 2048), (70000, 300, 30000)):
        mat = synth.dense_matrix_c(M, N, d, seed=21)
        m = hip_ctx.matrix_from_host(mat)
        got = m.pairw_matrix()
        want = np.triu(orc.tile_counts(mat, 0, N, 0, N), k=1)
        assert np.array_equal(got, want), (M, N, d)
        assert int(got.sum(dtype=np.uint64)) == m.pairw()
        m.close()


def test_union_and_symmetric_difference(hip_ctx, orc):
    """OR / XOR pair counts (by inclusion-exclusion on the device) against the
    oracle's direct popcount(a|b) / popcount(a^b), as totals and as materialised matrices."""
    for M, N, d in ((9000, 300, 4000), (4096, 513, 100), (65536, 130, 32768)):
        mat = synth.dense_matrix_c(M, N, d, seed=33)
        m = hip_ctx.matrix_from_host(mat)
        assert np.array_equal(m.row_counts(),
                              np.bitwise_count(mat).sum(axis=1, dtype=np.uint64).astype(np.uint32))
        for name, op in (("and", 0), ("or", 1), ("xor", 2)):
            assert m.pairw_op(name) == orc.truth_naive_op(mat, op), (M, N, d, name)
            want = np.triu(orc.tile_counts_op(mat, 0, N, 0, N, op), k=1)
            assert np.array_equal(m.pairw_matrix(name), want), (M, N, d, name)
        m.close()


def test_square_on_matrix_cores(hip_ctx, orc):
    """rectangular sum over A x B on the strip kernel ([A ; B] shadow, no diagonal
    phase) against the oracle's wrapper_square and the popcount kernel; ragged row counts."""
    mat = synth.dense_matrix_c(9000, 2003, 4000, seed=14)
    for na in (1100, 257, 1):
        a, b = mat[:na], mat[na:]
        ma, mb = hip_ctx.matrix_from_host(a), hip_ctx.matrix_from_host(b)
        want = orc.wrapper_square(a, b)
        try:
            for variant in (4, 2, -1):
                hip_ctx.set_option("variant", variant)
                assert ma.square(mb) == want, (na, variant)
                assert mb.square(ma) == want, (na, variant)
        finally:
            hip_ctx.set_option("variant", -1)
        assert ma.pairw() + mb.pairw() + want == orc.wrapper_diag(mat)
        ma.close(); mb.close()


def test_strip_item_shaping_options(hip_ctx, orc):
    """The strip kernel's work-list knobs (run cap, short-item tail, persistent per-XCD queues)
    reshape the schedule only: every combination must give the oracle's total, on a ragged
    shape small enough for the CPU and on shards."""
    M, N, d = 20000, 1500, 9000
    mat = synth.dense_matrix_c(M, N, d, seed=77)
    want = orc.wrapper_diag(mat)
    m = hip_ctx.matrix_from_host(mat)
    defaults = {k: hip_ctx.get_option(k) for k in ("k2_max_run",)}
    try:
        for pad in (0, 128, 1152, -1):                     # row pitch of the FP4 shadow
            hip_ctx.set_option("k2_pitch_pad", pad)
            for variant in shipped(hip_ctx, "variant", (3, 4, 5)):
                hip_ctx.set_option("variant", variant)
                assert m.pairw() == want, (pad, variant)
            assert np.array_equal(m.pairw_matrix()[:40, :300],
                                  np.triu(orc.tile_counts(mat, 0, 40, 0, 300), k=1)), pad
        hip_ctx.set_option("variant", 4)
        hip_ctx.set_option("k2_strip_operands", 4)        # the work-list shaping of the FP4 strips
        for persistent in shipped(hip_ctx, "k2_persistent", (0, 1)):
            for max_run, tail_slices, tail_run in ((4096, 0, 32), (128, 3, 32), (5, 2, 3), (1, 255, 1)):
                hip_ctx.set_option("k2_persistent", persistent)
                hip_ctx.set_option("k2_max_run", max_run)
                hip_ctx.set_option("k2_tail_slices", tail_slices)
                hip_ctx.set_option("k2_tail_run", tail_run)
                assert m.pairw() == want, (persistent, max_run, tail_slices, tail_run)
                assert sum(m.pairw(r, 3) for r in range(3)) == want
    finally:
        hip_ctx.set_option("variant", -1)
        hip_ctx.set_option("k2_strip_operands", 0)
        hip_ctx.set_option("k2_persistent", 0)
        hip_ctx.set_option("k2_max_run", defaults["k2_max_run"])
        hip_ctx.set_option("k2_tail_slices", 3)
        hip_ctx.set_option("k2_tail_run", 32)
        hip_ctx.set_option("k2_pitch_pad", -1)
    m.close()


def test_persistent_queues_at_headline_shape(hip_ctx):
    """Persistent per-XCD queues at N=10000 x M=65536: repeated launches (the queue heads are
    re-zeroed by the fold kernel) must all reproduce the column identity."""
    if not shipped(hip_ctx, "k2_persistent", (1,)):
        pytest.skip("the persistent-queue strips are a form of the tools build (make probes)")
    M, N, d = 65536, 10000, 32768
    m = hip_ctx.matrix(N, M // 64)
    m.fill_synthetic(M, d, seed=44)
    want = m.column_identity()
    try:
        hip_ctx.set_option("k2_persistent", 1)
        assert {m.pairw() for _ in range(10)} == {want}
        assert sum(m.pairw(r, 8) for r in range(8)) == want
    finally:
        hip_ctx.set_option("k2_persistent", 0)
    m.close()


def test_kernel_time_and_trace_probes(hip_ctx):
    """Measurement aids: the in-library timing of the dominant kernel (bench.py's roofline) and the
    per-item schedule trace leave results untouched and report sane numbers."""
    import ctypes as C
    M, N, d = 65536, 3000, 32768
    m = hip_ctx.matrix(N, M // 64)
    m.fill_synthetic(M, d, seed=45)
    want = m.column_identity()
    try:
        hip_ctx.set_option("time_kernels", 1)
        for _ in range(4):
            assert m.pairw() == want
        ms, n = hip_ctx.kernel_time()
        assert n == 4 and 0.0 < ms < 100.0
        assert hip_ctx.kernel_time() == (0.0, 0)          # the series restarts
        hip_ctx.set_option("time_kernels", 0)
        cnt = C.c_uint64(0)
        lib = sb.load()
        if not hip_ctx.get_option("probes_built"):
            # the shipped library carries no timing probes and no trace kernels: the options that
            # select them are refused, loudly (they live in the tools' build, `make probes`)
            for key, value in (("k2_ring", 18), ("k2_ring", 12), ("k2_ring", 3), ("k2_debug", 1)):
                with pytest.raises(sb.StormHipError):
                    hip_ctx.set_option(key, value)
            assert lib.storm_hip_debug_strip_trace(hip_ctx._h, None, 0, C.byref(cnt)) != 0
            assert m.pairw() == want
            return
        hip_ctx.set_option("k2_ring", 18)
        assert m.pairw() == want
        assert lib.storm_hip_debug_strip_trace(hip_ctx._h, None, 0, C.byref(cnt)) == 0
        assert cnt.value == hip_ctx.last_launch_info()["items"] > 0
        out = np.zeros((cnt.value, 8), dtype=np.uint64)
        assert lib.storm_hip_debug_strip_trace(hip_ctx._h, out.ctypes.data_as(C.c_void_p), cnt.value,
                                               C.byref(cnt)) == 0
        assert (out[:, 1] > out[:, 0]).all() and (out[:, 3] & 0xf).max() < 8
    finally:
        hip_ctx.set_option("time_kernels", 0)
        hip_ctx.set_option("k2_ring", 4)
    m.close()


def test_storm_h_matrix_extension(orc):
    """STORM_contig_pairw_matrix on the reference's own container: rows added through
    STORM_contig_add, matrix from the cached device mirror, grown between calls."""
    M, N, d = 5000, 400, 1200
    rows = synth.positions(M, N, d, seed=9)
    mat = synth.dense_matrix(M, N, d, seed=9)
    h = sb.StormContig(M)
    try:
        for r in rows[:250]:
            h.add(r)
        assert np.array_equal(h.pairw_matrix(), np.triu(orc.tile_counts(mat[:250], 0, 250, 0, 250), k=1))
        for r in rows[250:]:
            h.add(r)
        for name, op in (("and", 0), ("or", 1), ("xor", 2)):
            assert np.array_equal(h.pairw_matrix(name),
                                  np.triu(orc.tile_counts_op(mat, 0, N, 0, N, op), k=1)), name
        assert int(h.pairw_matrix().sum(dtype=np.uint64)) == h.pairw_intersect_cardinality()
    finally:
        h.free()


def test_readme_usage_program_in_c():
    """examples/readme_usage.c: the reference README's usage pattern (README.md:89-124) compiled
    as plain C against include/storm.h and linked with libstorm_hip.so. The program compares both
    containers with its own host loop; rows contain duplicate draws (set semantics)."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "stormbitmaps_amd", "readme_usage")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    for args in (["1500", "1000", "128"], ["700", "70000", "5000"], ["2", "64", "3"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (args, r.stdout, r.stderr)
        assert "contig=" in r.stdout and "storm=" in r.stdout


def test_randomised_parity_soak():
    """tools/soak_parity.py for a bounded time: random shapes, densities, shards and tuning
    options through dense / matrix / square / sparse entries, each bit-exact against the oracle
    (profiles/r01_h_soak_parity.json records a 4-minute run: 2598 cases)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "soak_parity.py"), "--seconds", "10",
                        "--seed", "7", "--max-cases", "300"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert summary["all_ok"] and summary["cases"] >= 20


def test_materialised_rectangle(hip_ctx, orc):
    """SURVEY §8f-2 as an operator: every pair (row of A, row of B), AND / OR / XOR counts, ragged
    shapes; sums agree with the rectangle total."""
    mat = synth.dense_matrix_c(9000, 900, 3000, seed=15)
    for na in (300, 257, 1, 899):
        a, b = mat[:na], mat[na:]
        ma, mb = hip_ctx.matrix_from_host(a), hip_ctx.matrix_from_host(b)
        for name, op in (("and", 0), ("or", 1), ("xor", 2)):
            want = orc.tile_counts_op(mat, 0, na, na, 900, op)
            assert np.array_equal(ma.square_matrix(mb, name), want), (na, name)
        assert int(ma.square_matrix(mb).sum(dtype=np.uint64)) == ma.square(mb)
        assert np.array_equal(mb.square_matrix(ma), ma.square_matrix(mb).T)
        ma.close(); mb.close()


def test_rows_beyond_the_dma_offsets_are_multiplied_in_k_chunks(hip_ctx, orc):
    """Rows longer than 2^27 bits do not fit the strip kernel's 32-bit DMA offsets in one piece: the
    pass runs k-chunk by k-chunk over a compact shadow (round 1 fell back to the popcount kernel);
    the popcount kernel and the tile kernel's refusal stay as cross-checks."""
    M, N = 140_000_000, 3
    rng = np.random.default_rng(5)
    mat = rng.integers(0, 1 << 63, size=(N, (M + 63) // 64), dtype=np.uint64)
    mat[:, -1] &= np.uint64((1 << (M % 64)) - 1) if M % 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    m = hip_ctx.matrix_from_host(mat)
    want = orc.wrapper_diag(mat)
    # default path: the strips on bit operands (K2b), whose DMA reaches rows of 2^29 bits
    assert m.pairw() == want
    assert hip_ctx.get_option("variant_used") == 4 and hip_ctx.get_option("k2_operands_used") == 5
    hip_ctx.set_option("k2_strip_operands", 4)     # the FP4 strips: k-chunked
    try:
        assert m.pairw() == want
        assert hip_ctx.get_option("k2_operands_used") == 4
        assert hip_ctx.last_launch_info()["word_pairs_executed"] >= 2      # out[2]: k-chunks of the pass
    finally:
        hip_ctx.set_option("k2_strip_operands", 0)
    try:
        hip_ctx.set_option("variant", 2)
        assert m.pairw() == want
        hip_ctx.set_option("variant", 3)
        with pytest.raises(RuntimeError):
            m.pairw()
    finally:
        hip_ctx.set_option("variant", -1)
    m.close()


def test_keep_shadow_follows_every_mutation(hip_ctx, orc):
    """Option keep_shadow: the FP4 shadow is reused only while (matrix, generation, shard, layout)
    are unchanged — every mutator, a second matrix on the same context, shard and variant changes
    must each force a rebuild."""
    M, N, d = 6000, 700, 2500
    a = synth.dense_matrix_c(M, N, d, seed=1)
    b = synth.dense_matrix_c(M, N, d, seed=2)
    wa, wb = orc.wrapper_diag(a), orc.wrapper_diag(b)
    try:
        hip_ctx.set_option("keep_shadow", 1)
        ma, mb = hip_ctx.matrix_from_host(a), hip_ctx.matrix_from_host(b)
        assert [ma.pairw(), ma.pairw(), mb.pairw(), ma.pairw(), mb.pairw()] == [wa, wa, wb, wa, wb]
        ma.upload(b)                                   # same buffer, new content
        assert ma.pairw() == wb
        ma.upload(a[:10], row0=5)                      # partial overwrite
        mixed = b.copy(); mixed[5:15] = a[:10]
        assert ma.pairw() == orc.wrapper_diag(mixed)
        assert sum(ma.pairw(r, 3) for r in range(3)) == orc.wrapper_diag(mixed)   # shard change
        assert ma.pairw() == orc.wrapper_diag(mixed)
        for variant in shipped(hip_ctx, "variant", (5, 3, 4)):    # layout change
            hip_ctx.set_option("variant", variant)
            assert ma.pairw() == orc.wrapper_diag(mixed), variant
        hip_ctx.set_option("variant", -1)
        assert ma.pairw_matrix().sum(dtype=np.uint64) == orc.wrapper_diag(mixed)  # tile layout in between
        assert ma.pairw() == orc.wrapper_diag(mixed)
        assert ma.square(mb) == orc.wrapper_square(mixed, b)                      # [A ; B] in between
        assert ma.pairw() == orc.wrapper_diag(mixed)
        ma.fill_synthetic(M, d, seed=1)
        assert ma.pairw() == wa
        ma.clear()
        assert ma.pairw() == 0
        ma.close(); mb.close()
    finally:
        hip_ctx.set_option("keep_shadow", 0)
        hip_ctx.set_option("variant", -1)


def test_materialised_bands(hip_ctx, orc):
    """The triangle in bands (for outputs too large to hold at once): stacking the bands gives the
    full matrix; unaligned band edges, AND / XOR."""
    import torch
    M, N, d = 9000, 1100, 3500
    mat = synth.dense_matrix_c(M, N, d, seed=16)
    m = hip_ctx.matrix_from_host(mat)
    for name, op in (("and", 0), ("xor", 2)):
        want = np.triu(orc.tile_counts_op(mat, 0, N, 0, N, op), k=1)
        got = np.zeros_like(want)
        for r0, nr in ((0, 256), (256, 300), (556, 1), (557, 543)):
            buf = torch.zeros((nr, N), dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            m.pairw_matrix_band_device(buf.data_ptr(), N, r0, nr, name)
            got[r0:r0 + nr] = buf.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want), name
    m.close()
