"""STORM_t device paths at their block, window and counter limits.

The arena (K3), the list probe (K4, probe_lists_kernel), the window join (K5, lists_matrix_kernel), the hash join (K5h,
lists_hash_kernel) and the staged gather, fed with rows built to sit on the edges of their formulations rather than the
uniform random rows of synth.positions: pair counts up to 65535 in 16-bit LDS counters, positions listed by every row of
a group, cells and windows at the thresholds where the kernels change their way, hash chains that wrap, block kinds on
either side of 4096, ragged row counts. Every case is checked against two references: the CPU oracle (storm.c:790-814
per pair) and a numpy count written here that shares no code with it. Every case also asserts which kernel ran
(STORM_hip_last_pass), so that a change of dispatch cannot make a case hollow.

The last test edits rows through the public block and row functions so that every block header comes back the same
(same ids, same counts, other positions): the device copies must follow.
"""
import ctypes as C

import numpy as np
import pytest

import stormbitmaps_amd as sb

pytestmark = pytest.mark.gpu

RAN_PROBE, RAN_LISTS, RAN_TILES = 32, 64, 128
COMBOS = ((1, 1), (1, 2), (0, 0), (-1, 0))   # (matrix_lists, matrix_lists_kernel)
OPS = ("and", "or", "xor")
SENTINEL = -7
WIN = 8191                # K5 window (storm_hip_lists.hip: kLmWin)
LH_FILL = 8192            # K5h: elements of a group at most (kLhFill)
LH_MAX_POS = (1 << 26) - 2


# ---------------------------------------------------------------------------------------------- references and rules
def _u32(values):
    return np.ascontiguousarray(values, dtype=np.uint32)


def _dedup(rows):
    return [np.unique(_u32(r)) for r in rows]


def _np_total(rows):
    """sum over positions of C(n_p, 2): the all-pairs total, from the rows' distinct positions alone."""
    rows = _dedup(rows)
    if not any(len(r) for r in rows):
        return 0
    _, n = np.unique(np.concatenate(rows), return_counts=True)
    return sum(c * (c - 1) // 2 for c in n.tolist())


def _blocks(row):
    """{block id: raw count} of one STORM_add (the kind is decided on the raw count, duplicates included)."""
    ids, cnt = np.unique(_u32(row) // 65536, return_counts=True)
    return dict(zip(ids.tolist(), cnt.tolist()))


def _k5_eligible(rows):
    n = 0
    for r in rows:
        if any(c >= 4096 for c in _blocks(r).values()):
            return False           # a bitmap block
        d = len(np.unique(_u32(r)))
        if d > 65535:
            return False           # 16-bit counters
        n += d
    return n > 0


def _hash_g(rows):
    """K5h's group size: the largest G of 64 / 32 / 16 / 8 whose every group lists at most kLhFill positions; 0 when none
    fits or a listed block has id 1023 or more (kLhMaxPos)."""
    lens = [len(np.unique(_u32(r))) for r in rows]
    ids = [int(_u32(r).max()) // 65536 for r in rows if len(r)]
    if not ids or max(ids) * 65536 + 65535 > LH_MAX_POS:
        return 0
    for g in (64, 32, 16, 8):
        if max(sum(lens[i:i + g]) for i in range(0, len(lens), g)) <= LH_FILL:
            return g
    return 0


def _worthwhile(rows):
    """The automatic rule (storm_hip_rowlists_worthwhile_counts, default density 80 / 10000 of the dense replica's bits)."""
    n = sum(len(np.unique(_u32(r))) for r in rows)
    max_id = max(int(_u32(r).max()) // 65536 for r in rows if len(r))
    bits = ((max_id + 1) * 65536 + 511) // 512 * 512 * len(rows)
    return n <= bits * 80 / 10000


def _expected_pass(rows, lists, kernel):
    """(kernel mask, group rows or None) the per-pair matrix must report."""
    if lists == 0 or not _k5_eligible(rows):
        return RAN_TILES, None
    if lists == 1:
        return RAN_LISTS, (_hash_g(rows) or 64) if kernel == 2 else 64
    if not _worthwhile(rows):
        return RAN_TILES, None
    return RAN_LISTS, 64      # (auto: the hash kernel from G = 64 on, else the window kernel: 64 rows either way)


def _probe_expected(rows):
    """Whether the totals take the list-probe kernel (K4) at sparse_probe != 0: a column with two list blocks or more,
    and the matrix-core variant (a column at least 64 pool rows wide)."""
    per_col, lists_col, bitmaps_col = {}, {}, {}
    for r in rows:
        for b, c in _blocks(r).items():
            per_col[b] = per_col.get(b, 0) + 1
            if c < 4096:
                lists_col[b] = lists_col.get(b, 0) + 1
            else:
                bitmaps_col[b] = bitmaps_col.get(b, 0) + 1
    if not per_col:
        return False
    wide = max(per_col.values()) >= 64 or any(lists_col.get(b, 0) and bitmaps_col.get(b, 0) for b in per_col)
    return wide and any(n >= 2 for n in lists_col.values())


def _last_pass():
    out = (C.c_uint64 * 4)()
    assert sb.load().STORM_hip_last_pass(out) == 0
    return [int(x) for x in out]


def _set(key, value):
    assert sb.load().STORM_hip_set_option(key.encode(), value) == 0, key


@pytest.fixture(autouse=True)
def _restore_options():
    yield
    for key, value in (("matrix_lists", -1), ("matrix_lists_kernel", 0), ("sparse_probe", -1), ("probe_bundle", -1)):
        sb.load().STORM_hip_set_option(key.encode(), value)


def _storm(rows):
    s = sb.Storm()
    for r in rows:
        assert s.add(_u32(r)) == 1
    return s


def _diff(got, want):
    bad = np.argwhere(got != want)
    return [(int(i), int(j), int(got[i, j]), int(want[i, j])) for i, j in bad[:6]]


# ---------------------------------------------------------------------------------------------- the checks
def check_matrix(s, rows, want, pairs=(), combos=COMBOS, ops=OPS, host_ops=("and",)):
    """pairw_matrix_device for every (matrix_lists, matrix_lists_kernel) and op against the oracle's matrix `want`
    (and), entries i >= j and rows / columns beyond N left at the sentinel; pairw_matrix to host; the kernel that ran."""
    import torch
    N = len(rows)
    lens = np.array([len(np.unique(_u32(r))) for r in rows], dtype=np.int64)
    want = want.astype(np.int64)
    for i, j, k in pairs:      # the pairs built to share k positions: numpy's own count, the oracle's, as built
        assert len(np.intersect1d(rows[i], rows[j])) == k == want[i, j], (i, j, k, int(want[i, j]))
    upper = np.triu(np.ones((N, N), dtype=bool), k=1)
    ref_of = {"and": want, "or": lens[:, None] + lens[None, :] - want, "xor": lens[:, None] + lens[None, :] - 2 * want}
    dev = torch.full((N + 1, N + 3), SENTINEL, dtype=torch.int32, device="cuda:0")
    for lists, kernel in combos:
        _set("matrix_lists", lists)
        _set("matrix_lists_kernel", kernel)
        kind, group = _expected_pass(rows, lists, kernel)
        for op in ops:
            ref = ref_of[op]
            dev.fill_(SENTINEL)
            s.pairw_matrix_device(dev.data_ptr(), N + 1, N + 3, op)
            full = dev.cpu().numpy()
            got = full[:N, :N].astype(np.int64)
            ran = _last_pass()
            assert np.array_equal(got[upper], ref[upper]), (N, op, lists, kernel, ran, _diff(np.where(upper, got, 0), np.where(upper, ref, 0)))
            assert (got[~upper] == SENTINEL).all() and (full[N:] == SENTINEL).all() and (full[:, N:] == SENTINEL).all(), (op, lists, kernel)
            assert ran[0] == kind, (N, op, lists, kernel, ran, kind)
            if group is not None:
                assert ran[3] == group, (N, op, lists, kernel, ran, group)
        for op in host_ops:
            host = s.pairw_matrix(op).astype(np.int64)
            assert np.array_equal(host, np.triu(ref_of[op], k=1)), (N, op, lists, kernel, _diff(host, np.triu(ref_of[op], k=1)))
            assert _last_pass()[0] == kind, (op, lists, kernel)


def check_totals(s, rows, want, serialized=True):
    """STORM_pairw_intersect_cardinality and _blocked(0) on the handle (a first call on a fresh container takes the staged
    build, the next ones the steady path), then the same container from its serialized bytes with sparse_probe 0 / 1
    and probe_bundle 1 / 4, the probe kernel reported exactly where it is expected."""
    lib = sb.load()
    probe = _probe_expected(rows)
    got = [s.pairw_intersect_cardinality()]
    if len(rows) >= 2:     # (fewer rows: no pass runs, nothing is reported)
        assert bool(_last_pass()[0] & RAN_PROBE) == probe, (len(rows), _last_pass(), probe)
    got.append(s.pairw_intersect_cardinality_blocked(0))
    got.append(s.pairw_intersect_cardinality())
    assert got == [want] * 3, (len(rows), got, want)
    if not serialized or len(rows) < 2:
        return
    ctx = sb.HipContext(0)
    data = s.serialize()
    h = C.c_void_p()
    assert lib.storm_hip_sparse_create_serialized(ctx._h, data.ctypes.data_as(C.c_void_p), data.size, C.byref(h)) == 0, \
        lib.storm_hip_last_error()
    out = C.c_uint64()
    try:
        for sp, bundle in ((0, 1), (1, 1), (1, 4)):
            ctx.set_option("sparse_probe", sp)
            ctx.set_option("probe_bundle", bundle)
            assert lib.storm_hip_pairw_sparse(ctx._h, h, 0, 1, C.byref(out)) == 0, lib.storm_hip_last_error()
            assert out.value == want, (len(rows), sp, bundle, out.value, want)
            ran = ctx.last_pass_report()["kernels"]
            assert ("probe_lists_kernel" in ran) == (sp == 1 and probe), (sp, bundle, ran, probe)
    finally:
        lib.storm_hip_sparse_destroy(ctx._h, h)
        ctx.close()


def check_all(orc, rows, pairs=(), combos=COMBOS, ops=OPS, serialized=True):
    o = orc.storm(rows)
    want = o.pair_counts()
    total = _np_total(rows)
    assert o.pairw() == o.pairw_blocked(0) == total == int(want.sum(dtype=np.uint64))
    s = _storm(rows)
    try:
        check_totals(s, rows, total, serialized)      # (first: the staged build)
        check_matrix(s, rows, want, pairs, combos, ops)
        assert s.pairw_intersect_cardinality() == total
    finally:
        s.free()


# ---------------------------------------------------------------------------------------------- A. counter range
def _seq(which, n, n_blocks=34):
    """Element i of sequence 0 / 1: block i % n_blocks, offset 2 (i // n_blocks) + which. The two sequences are disjoint,
    and any prefix of one with any prefix of the other puts at most 2 x ceil(65536 / 34) = 3856 positions in a block:
    every block stays a list."""
    i = np.arange(n, dtype=np.uint64)
    return np.sort(i % n_blocks * 65536 + 2 * (i // n_blocks) + which).astype(np.uint32)


def _sharing(k, n=65535, salt=0):
    """A row of n positions sharing exactly k with _seq(0, n): the first k of sequence 0, then n - k of sequence 1."""
    i = np.arange(n, dtype=np.uint64)
    seq = lambda which, idx: idx % 34 * 65536 + 2 * (idx // 34) + which
    return np.sort(np.concatenate([seq(0, i[:k]), seq(1, i[salt:salt + n - k])])).astype(np.uint32)


def _short_rows(N, seed, d=12, n_blocks=34):
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(N):
        if i % 5 == 4:
            rows.append(np.zeros(0, dtype=np.uint32))
        else:
            rows.append(np.unique(rng.integers(0, n_blocks * 65536, size=d, dtype=np.uint64)).astype(np.uint32))
    return rows


def test_counter_range_rows_of_65535_positions(orc):
    """K5 / K5h keep a pair's count in a 16-bit half of a 32-bit LDS word, columns j (even) and j + 1 in one word. Rows of
    exactly 65535 positions over 34 blocks (every block a list): pairs that share exactly 65535, 65534, 32768, 256 and 255
    positions, inside one 64-row group, on the tile diagonal and across the 768-row chunk edge; two adjacent columns of
    one tile with 65535 and 0 against the same row (a carry would show in the second)."""
    X = _seq(0, 65535)
    Z = _seq(1, 65535)                       # shares nothing with X
    N = 800
    rows = _short_rows(N, seed=1)
    layout = {0: X, 2: X, 3: Z, 4: _sharing(65534), 5: _sharing(32768), 6: _sharing(256), 7: _sharing(255),
              70: _sharing(65534, salt=3), 768: X, 769: Z, 799: _sharing(256, salt=7)}
    for i, r in layout.items():
        rows[i] = r
    pairs = [(0, 2, 65535), (0, 3, 0), (0, 4, 65534), (0, 5, 32768), (0, 6, 256), (0, 7, 255), (0, 70, 65534),
             (0, 768, 65535), (0, 769, 0), (2, 768, 65535), (3, 769, 65535), (0, 799, 256), (4, 70, 65534 - 0)]
    # (4 and 70 share the first 65534 of sequence 0; their sequence-1 parts are offset by 3 and do not meet)
    pairs[-1] = (4, 70, len(np.intersect1d(rows[4], rows[70])))
    assert pairs[-1][2] >= 65534
    check_all(orc, rows, pairs, ops=("and", "xor"))


def test_counter_range_a_row_of_65536_positions_is_declined_by_k5(orc):
    """A row of 65536 positions does not fit a 16-bit counter: K5 must decline the container (dense replica) whatever the
    option says, and the count of 65536 between two such rows — next to a column with 0 in the same counter word —
    must come out whole."""
    X6 = _seq(0, 65536)
    rows = _short_rows(140, seed=2)
    rows[0], rows[10], rows[11], rows[12] = X6, X6, _seq(1, 65535), _sharing(65535)
    pairs = [(0, 10, 65536), (0, 11, 0), (0, 12, 65535), (10, 12, 65535)]
    assert not _k5_eligible(rows)
    check_all(orc, rows, pairs, ops=("and",))


def test_counter_range_a_group_listing_the_same_positions(orc):
    """K4: every one of the 128 rows of a probe group lists the same positions (Cn = 128: C(128, 2) pairs per position);
    K5h: the same positions from every row of a group — equal keys chained through the buckets — 600 per row so that
    only G = 8 fits the hash table."""
    rng = np.random.default_rng(3)
    P = np.unique(rng.integers(0, 3 * 65536, size=640, dtype=np.uint64)).astype(np.uint32)[:600]
    Q = np.unique(np.concatenate([P[:300], rng.integers(0, 3 * 65536, size=400, dtype=np.uint64).astype(np.uint32)]))[:600]
    rows = [P] * 128 + [Q] * 64 + _short_rows(70, seed=4, d=30, n_blocks=3)
    assert _hash_g(rows) == 8
    check_all(orc, rows, [(0, 127, 600), (5, 130, len(np.intersect1d(P, Q)))])


# ---------------------------------------------------------------------------------------------- B. K5 windows
def test_k5_windows_edges_and_one_sided_windows(orc):
    """Positions with p % 8191 in {0, 8190} (the first and last entry of a window's table; entry 0 is the sentinel), the
    first and the last window of the rows (the last block's end is no multiple of 8191 or 65536), and windows in which
    only the A group lists anything, only the far chunk, or both, alternating: tiles (group 0, chunk 1) see all three."""
    rng = np.random.default_rng(5)
    max_block = 9
    last = max_block * 65536 + 65535
    n_win = last // WIN + 1
    N = 900
    rows = []
    for i in range(N):
        if i < 64:
            wins = [w for w in range(n_win) if w % 3 != 1]          # A side of tile (0, 1): windows 0, 2 mod 3
        elif i >= 768:
            wins = [w for w in range(n_win) if w % 3 != 0]          # far side of tile (0, 1): windows 1, 2 mod 3
        else:
            wins = list(rng.choice(n_win, size=6, replace=False))
        pos = []
        for w in wins:
            base = w * WIN
            cand = [base, base + WIN - 1, base + int(rng.integers(1, WIN - 1))]
            pos += [p for p in cand if p <= last and rng.random() < 0.7]
        if i % 7 == 0:
            pos += [0, last, last - 1, (n_win - 1) * WIN]
        rows.append(np.unique(np.array(pos, dtype=np.uint32)))
    rows[400] = np.zeros(0, dtype=np.uint32)
    assert _k5_eligible(rows) and max(len(r) for r in rows) < 4096
    check_all(orc, rows, combos=((1, 1), (1, 2), (0, 0)), ops=("and", "or"))


# ---------------------------------------------------------------------------------------------- C. K5 thresholds
def _spread(counts_by_window, row_ids, rng):
    """{row: positions}: every window w gets counts_by_window[w] elements over the given rows, evenly, distinct per row."""
    out = {r: [] for r in row_ids}
    for w, total in counts_by_window.items():
        per, extra = divmod(total, len(row_ids))
        for k, r in enumerate(row_ids):
            n = per + (k < extra)
            if n:
                out[r].append(w * WIN + rng.choice(WIN, size=n, replace=False))
    return out


def test_k5_thresholds_cells_far_groups_and_a_toggles(orc):
    """Each just below, at and just above:
    - a (group, window) cell of 12287 / 12288 / 12289 elements (kDealMax: the bank deal keeps out beyond it);
    - far elements of one chunk in one window at 8192 / 16384 / 24576 +- 1 (the far-register groups switch at 8 x 1024,
      16 x 1024, beyond 24 x 1024 the remainder loop);
    - A-group elements in one window at 1024 +- 1 (one register per thread, then the toggle remainder)."""
    rng = np.random.default_rng(6)
    N = 768
    pos = {r: [] for r in range(N)}
    group0 = list(range(64))
    for part in (_spread({0: 12287, 1: 12288, 2: 12289, 3: 1023, 4: 1024, 5: 1025}, group0, rng),
                 _spread({6 + k: c for k, c in enumerate((8191, 8192, 8193, 16383, 16384, 16385, 24575, 24576, 24577))},
                         list(range(N)), rng)):
        for r, p in part.items():
            pos[r] += p
    rows = [np.unique(np.concatenate(pos[r]).astype(np.uint32)) if pos[r] else np.zeros(0, np.uint32) for r in range(N)]
    # the cells as built (distinct per row and window, so nothing was merged away)
    win = lambda rs, w: sum(int(((r // WIN) == w).sum()) for r in rs)
    assert [win(rows[:64], w) for w in range(6)] == [12287, 12288, 12289, 1023, 1024, 1025]
    assert [win(rows, 6 + k) for k in range(9)] == [8191, 8192, 8193, 16383, 16384, 16385, 24575, 24576, 24577]
    assert _k5_eligible(rows)
    check_all(orc, rows, combos=((1, 1), (1, 2), (-1, 0)), ops=("and", "xor"))


# ---------------------------------------------------------------------------------------------- D. K5h
def _hash(p):
    return ((_u32(p).astype(np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)) >> np.uint64(19)


@pytest.mark.parametrize("group0", [8192, 8193])
def test_k5h_group_size_at_the_table_fill(orc, group0):
    """The worst 64-row group at 8192 elements: G = 64; at 8193: G falls to 32."""
    rng = np.random.default_rng(group0)
    N = 130
    rows = []
    for i in range(N):
        n = group0 // 64 + (i == 0 and group0 % 64) if i < 64 else 60
        rows.append(np.sort(rng.choice(4 * 65536, size=n, replace=False)).astype(np.uint32))
    assert sum(len(r) for r in rows[:64]) == group0
    assert _hash_g(rows) == (64 if group0 == 8192 else 32)
    check_all(orc, rows, combos=((1, 2), (1, 1), (-1, 0)), ops=("and", "or"))


def test_k5h_chains_on_one_home_bucket_wrap_to_bucket_zero(orc):
    """Positions chosen to share one home bucket ((p * 0x9E3779B1 mod 2^32) >> 19): bucket 8191, whose chains wrap to
    bucket 0, and bucket 0 itself; many rows of one group list the same of them (equal keys on one chain)."""
    cand = np.arange(0, 1022 * 65536, 7, dtype=np.uint64).astype(np.uint32)
    h = _hash(cand)
    top = cand[h == 8191][:48]
    zero = cand[h == 0][:24]
    one = cand[h == 1][:8]
    assert len(top) == 48 and len(zero) == 24 and len(one) == 8
    rng = np.random.default_rng(8)
    N = 129
    rows = []
    for i in range(N):
        if i < 40:
            sel = np.concatenate([top[: 24 + i % 24], zero[: i % 24], one[: i % 8]])    # rows of group 0: long equal chains
        else:
            sel = rng.choice(np.concatenate([top, zero, one]), size=int(rng.integers(0, 30)), replace=False)
        rows.append(np.unique(sel).astype(np.uint32))
    assert _hash_g(rows) == 64
    check_all(orc, rows, combos=((1, 2), (1, 1)), ops=("and", "xor"))


@pytest.mark.parametrize("last_id", [1022, 1023])
def test_k5h_last_block_id(orc, last_id):
    """Rows whose last block id is 1022 are K5h-eligible; one block at id 1023 (positions past kLhMaxPos) makes the container
    ineligible even when the hash kernel is forced: the window kernel takes it."""
    rng = np.random.default_rng(last_id)
    N = 130
    rows = []
    for i in range(N):
        ids = np.unique(rng.integers(0, 1022, size=6))
        if i % 9 == 0:
            ids = np.append(ids, 1022)
        p = ids.astype(np.uint64) * 65536 + rng.integers(0, 65536, size=len(ids)).astype(np.uint64)
        rows.append(np.unique(np.concatenate([p, [1022 * 65536 + 65535, 5]]).astype(np.uint32)))
    if last_id == 1023:
        rows[77] = np.append(rows[77], np.uint32(1023 * 65536 + 3))
        rows[78] = np.append(rows[78], np.uint32(1023 * 65536 + 3))
    assert _hash_g(rows) == (64 if last_id == 1022 else 0)
    check_all(orc, rows, combos=((1, 2), (1, 1)), ops=("and", "or"))


# ---------------------------------------------------------------------------------------------- E. kinds and shapes
def test_block_kinds_at_4096_and_block_edges(orc):
    """Blocks of exactly 4095 (list) and 4096 (bitmap) positions in the same column; positions 0 and 65535 of a block; a
    column with a single list row; rows that are all bitmaps; empty rows in between; duplicates inside one STORM_add (the
    kind is decided on the raw count: 4096 values with a duplicate make a bitmap of 4095 bits)."""
    rng = np.random.default_rng(9)
    N = 200
    rows = []
    for i in range(N):
        r = [rng.integers(0, 4 * 65536, size=40)]
        if i % 10 == 0:
            r.append(rng.choice(65536, size=4095 + (i // 10) % 2, replace=False))     # column 0: 4095 / 4096
        if i % 13 == 0:
            r.append([0, 65535, 65536, 2 * 65536 - 1])
        rows.append(np.unique(np.concatenate(r).astype(np.uint32)))
    rows[5] = np.zeros(0, np.uint32)
    rows[6] = np.concatenate([rng.choice(65536, size=5000, replace=False),
                              65536 * 3 + rng.choice(65536, size=4096, replace=False)]).astype(np.uint32)
    rows[6].sort()
    rows[7] = np.zeros(0, np.uint32)
    rows[8] = np.array([9 * 65536 + 17, 9 * 65536 + 65535], dtype=np.uint32)          # column 9: one list row
    dup = np.sort(np.concatenate([np.arange(2 * 65536, 2 * 65536 + 4095), [2 * 65536 + 100]])).astype(np.uint32)
    rows[9] = dup                                                                     # 4096 values, 4095 distinct
    rows[10] = np.array([5, 5, 5, 9, 9, 70000, 70000, 70001], dtype=np.uint32)
    assert _blocks(rows[9])[2] == 4096 and len(np.unique(rows[9])) == 4095
    check_all(orc, rows, combos=((1, 1), (0, 0)), ops=("and", "xor"))
    # every row all bitmaps
    bm = [np.sort(np.concatenate([b * 65536 + rng.choice(65536, size=4096 + i, replace=False) for b in (0, 2)])).astype(np.uint32)
          for i in range(70)]
    bm[3] = np.zeros(0, np.uint32)
    check_all(orc, bm, combos=((1, 2), (-1, 0)), ops=("and",))


@pytest.mark.parametrize("N", [1, 2, 127, 128, 129, 767, 768, 769])
def test_ragged_row_counts(orc, N):
    """Row counts around the 64-row groups, the 128-row probe groups and the 768-row chunks: list-only rows (K5 / K5h
    eligible) with empty rows in between, and (N <= 129) a bitmap block in the last row."""
    rng = np.random.default_rng(N)
    rows = []
    for i in range(N):
        d = 0 if i % 11 == 3 else int(rng.integers(1, 80))
        rows.append(np.unique(rng.integers(0, 3 * 65536, size=d, dtype=np.uint64)).astype(np.uint32))
    check_all(orc, rows, ops=("and", "or"))
    if N <= 129:
        rows[-1] = np.unique(np.concatenate([rows[-1], 65536 + np.arange(0, 65536, 7)]).astype(np.uint32))
        check_all(orc, rows, combos=((1, 1), (0, 0)), ops=("and",), serialized=False)


def test_probe_streams_of_several_chunks_and_three_shards(orc):
    """Case E of tests/test_arena_plan.py (700 lists of 800 positions in one block column: every octant's far stream has
    several chunks, the last atom is ragged) as a STORM_t: the total through every build and both item lists, then the
    arena's shards of worlds 1 and 3 summed."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "make_arena_digests", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_arena_digests.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    rows = [row[0][2].astype(np.uint32) for row in gen.case_rows("E")]
    want = _np_total(rows)
    assert orc.storm(rows).pairw() == want
    s = _storm(rows)
    lib = sb.load()
    ctx = sb.HipContext(0)
    h = C.c_void_p()
    try:
        check_totals(s, rows, want)
        data = s.serialize()
        assert lib.storm_hip_sparse_create_serialized(ctx._h, data.ctypes.data_as(C.c_void_p), data.size, C.byref(h)) == 0, \
            lib.storm_hip_last_error()
        out = C.c_uint64()
        ctx.set_option("sparse_probe", 1)
        for bundle in (1, 4):
            ctx.set_option("probe_bundle", bundle)
            for world in (1, 3, 1):     # (back to one shard: the list on the device is planned again)
                parts = []
                for rank in range(world):
                    assert lib.storm_hip_pairw_sparse(ctx._h, h, rank, world, C.byref(out)) == 0, lib.storm_hip_last_error()
                    assert "probe_lists_kernel" in ctx.last_pass_report()["kernels"]
                    parts.append(out.value)
                assert sum(parts) == want and (world == 1 or all(parts)), (bundle, world, parts, want)
    finally:
        if h:
            lib.storm_hip_sparse_destroy(ctx._h, h)
        ctx.close()
        s.free()


# ---------------------------------------------------------------------------------------------- device copies follow edits
_ROW_BYTES, _BLOCK_BYTES = 32, 128     # sizeof(STORM_bitmap_cont_t), sizeof(STORM_bitmap_t) (tests/test_abi.py)


def _block_fns(lib):
    for name in ("STORM_bitmap_cont_add", "STORM_bitmap_add", "STORM_bitmap_add_scalar_only"):
        getattr(lib, name).argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        getattr(lib, name).restype = C.c_int
    for name in ("STORM_bitmap_cont_clear", "STORM_bitmap_clear"):
        getattr(lib, name).argtypes = [C.c_void_p]
        getattr(lib, name).restype = C.c_int


def _row_ptr(s, i):
    return C.cast(s._h, C.POINTER(C.c_void_p))[0] + i * _ROW_BYTES      # STORM_s.conts[i]


def _block_ptr(s, i, b):
    return C.cast(C.c_void_p(_row_ptr(s, i)), C.POINTER(C.c_void_p))[0] + b * _BLOCK_BYTES   # conts[i].bitmaps[b]


def _same_headers(rng, row, avoid):
    """Other positions with the same block ids and the same count per block (so the same kind)."""
    out = []
    for b, c in _blocks(row).items():
        free = np.setdiff1d(np.arange(65536, dtype=np.uint32), (np.concatenate([row, avoid]) % 65536)[np.concatenate([row, avoid]) // 65536 == b])
        out.append(b * 65536 + np.sort(rng.choice(free, size=c, replace=False)).astype(np.uint32))
    return np.sort(np.concatenate(out)).astype(np.uint32)


def test_device_copies_follow_edits_that_keep_every_block_header(orc):
    """STORM_bitmap_cont_clear + STORM_bitmap_cont_add, then STORM_bitmap_clear + STORM_bitmap_add on a single block, that
    give back the same block ids and the same count per block with other positions: the staged build (edit before the
    first call), the cached arena, K5 lists and dense replica (edit after a first call) must all answer for the rows as
    they are now (the reference recomputes from the container on every call)."""
    import torch
    lib = sb.load()
    _block_fns(lib)
    rng = np.random.default_rng(11)
    for list_only in (False, True):
        N = 150
        rows = []
        for i in range(N):
            r = rng.integers(0, 2 * 65536, size=300 if list_only else 900, dtype=np.uint64)
            rows.append(np.unique(r).astype(np.uint32))
        victim = 17
        # the victim: a list block in column 0 and (mixed) a bitmap block in column 1
        rows[victim] = np.sort(np.concatenate([rng.choice(65536, size=250, replace=False),
                                               65536 + rng.choice(65536, size=200 if list_only else 5000, replace=False)])).astype(np.uint32)
        kinds = {b: c >= 4096 for b, c in _blocks(rows[victim]).items()}
        assert kinds == {0: False, 1: not list_only}
        s = _storm(rows)
        dev = torch.zeros((N, N), dtype=torch.int32, device="cuda:0")

        def check(stage):
            want = orc.storm(rows).pair_counts().astype(np.int64)
            total = _np_total(rows)
            got = {}
            if list_only:     # K5 first (its build reads the stage too), then the arena
                _set("matrix_lists", 1)
                s.pairw_matrix_device(dev.data_ptr(), N, N)
                got["lists"] = np.triu(dev.cpu().numpy().astype(np.int64), k=1)
                assert _last_pass()[0] == RAN_LISTS
            got["total"] = s.pairw_intersect_cardinality()
            got["blocked"] = s.pairw_intersect_cardinality_blocked(0)
            _set("matrix_lists", 0)
            dev.zero_()
            s.pairw_matrix_device(dev.data_ptr(), N, N)
            got["dense"] = np.triu(dev.cpu().numpy().astype(np.int64), k=1)
            assert _last_pass()[0] == RAN_TILES
            _set("matrix_lists", -1)
            for k, v in got.items():
                ok = v == total if k in ("total", "blocked") else np.array_equal(v, np.triu(want, k=1))
                assert ok, (stage, list_only, k, v if k in ("total", "blocked") else _diff(v, np.triu(want, k=1)), total)

        before = _np_total(rows)
        # 1. before any call: the staged build must not take the staged blocks of the victim
        new = _same_headers(rng, rows[victim], rows[victim])
        assert lib.STORM_bitmap_cont_clear(C.c_void_p(_row_ptr(s, victim))) == 1
        assert lib.STORM_bitmap_cont_add(C.c_void_p(_row_ptr(s, victim)), new.ctypes.data_as(C.c_void_p), new.size) == 1
        rows[victim] = new
        assert _np_total(rows) != before
        check("staged")
        # 2. after a first call: the cached arena, K5 lists and dense replica
        before = _np_total(rows)
        new = _same_headers(rng, rows[victim], rows[victim])
        assert lib.STORM_bitmap_cont_clear(C.c_void_p(_row_ptr(s, victim))) == 1
        assert lib.STORM_bitmap_cont_add(C.c_void_p(_row_ptr(s, victim)), new.ctypes.data_as(C.c_void_p), new.size) == 1
        rows[victim] = new
        assert _np_total(rows) != before
        check("cached, row edit")
        # 3. one block: cleared and filled again with as many other positions, of the same kind
        for b in (1, 0):
            before = _np_total(rows)
            blk = rows[victim][rows[victim] // 65536 == b]
            new_blk = _same_headers(rng, blk, blk)
            fn = lib.STORM_bitmap_add if kinds[b] else lib.STORM_bitmap_add_scalar_only
            assert lib.STORM_bitmap_clear(C.c_void_p(_block_ptr(s, victim, b))) == 1
            assert fn(C.c_void_p(_block_ptr(s, victim, b)), new_blk.ctypes.data_as(C.c_void_p), new_blk.size) == new_blk.size
            rows[victim] = np.sort(np.concatenate([rows[victim][rows[victim] // 65536 != b], new_blk])).astype(np.uint32)
            assert _np_total(rows) != before
            check(f"cached, block {b} edit")
        s.free()
