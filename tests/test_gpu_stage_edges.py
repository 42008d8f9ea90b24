"""The block stage (storm_hip_stage_*, storm_hip_sparse.hip) at the limits of its four containers — the bitmap ring
(512 blocks), the bitmap chunk (8192 blocks), the list ring (4 MiB) and the list chunk (64 MiB, with its gap) — through the
C-ABI alone. DESIGN.md §2 states the limits; tests/test_stage_plan.py checks the list arithmetic without a device.

References, both written here: the total is sum_p C(n_p, 2) over the set-bit counts n_p of every position of every block
column (np.bincount for lists, np.unpackbits for bitmaps); per-pair counts are B @ B.T of a 0/1 float32 matrix per block
column (sums <= 65536: exact), as int64. Every arena total is also compared with the un-staged build of the same
description, and every pass states which kernel family ran (storm_hip_last_pass_report)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EINVAL = -1
NONE = 2 ** 64 - 1                      # "not staged"
BUF_BLOCKS, CHUNK_BLOCKS = 512, 8192    # storm_hip_stage_s::kBufBlocks, kChunkBlocks
LIST_BUF, LIST_CHUNK = 4 << 20, 64 << 20
RAN_BIT_STRIPS, RAN_LIST_PROBE, RAN_LISTS_MATRIX = 16, 32, 64
SENTINEL = -7


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Desc:
    """The flat block description of storm_hip.h, block after block, row after row."""

    def __init__(self):
        self.off, self.ids, self.kinds, self.lens, self.ptrs, self.toks, self.keep = [0], [], [], [], [], [], []

    def block(self, bid, kind, data, tok, n=None):
        data = np.ascontiguousarray(data)
        self.keep.append(data)
        self.ids.append(int(bid))
        self.kinds.append(kind)
        self.lens.append(0 if kind else (len(data) if n is None else n))
        self.ptrs.append(data.ctypes.data)
        self.toks.append(int(tok))

    def end_row(self):
        self.off.append(len(self.ids))

    def copy(self):
        other = Desc()
        other.__dict__.update({k: list(v) for k, v in self.__dict__.items()})
        return other

    def arrays(self, toks=None, lens=None):
        return (len(self.off) - 1, len(self.ids), np.array(self.off, dtype=np.uint64), np.array(self.ids, dtype=np.uint32),
                np.array(self.kinds, dtype=np.uint8), np.array(self.lens if lens is None else lens, dtype=np.uint32),
                np.array(self.ptrs, dtype=np.uint64), np.array(self.toks if toks is None else toks, dtype=np.uint64))


def _arena(lib, ctx, arrays, stage):
    """(rc, handle) of storm_hip_sparse_create_blocks_staged, or of the un-staged build when stage is None."""
    n_rows, n_blocks, off, ids, kinds, lens, ptrs, toks = arrays
    h = C.c_void_p()
    if stage is None:
        rc = lib.storm_hip_sparse_create_blocks(ctx._h, n_rows, n_blocks, _p(off), _p(ids), _p(kinds), _p(lens), _p(ptrs), C.byref(h))
    else:
        rc = lib.storm_hip_sparse_create_blocks_staged(ctx._h, n_rows, n_blocks, _p(off), _p(ids), _p(kinds), _p(lens), _p(ptrs),
                                                       stage, _p(toks), C.byref(h))
    return rc, h


def _rowlists(lib, ctx, arrays, stage):
    n_rows, n_blocks, off, ids, kinds, lens, ptrs, toks = arrays
    l = C.c_void_p()
    rc = lib.storm_hip_rowlists_create_blocks_staged(ctx._h, n_rows, n_blocks, _p(off), _p(ids), _p(kinds), _p(lens), _p(ptrs),
                                                     stage, _p(toks), C.byref(l))
    return rc, l


def _ran(lib, ctx):
    out = (C.c_uint64 * 4)()
    assert lib.storm_hip_last_pass_report(ctx._h, out) == 0
    return int(out[0])


def _total(lib, ctx, h, probe=-1):
    """(total, mask of the kernels that ran) of one all-pairs pass over the arena."""
    out = C.c_uint64()
    ctx.set_option("sparse_probe", probe)
    try:
        assert lib.storm_hip_pairw_sparse(ctx._h, h, 0, 1, C.byref(out)) == 0, lib.storm_hip_last_error()
    finally:
        ctx.set_option("sparse_probe", -1)
    return int(out.value), _ran(lib, ctx)


def _arena_total(lib, ctx, arrays, stage, probe=-1):
    rc, h = _arena(lib, ctx, arrays, stage)
    assert rc == 0 and h.value, lib.storm_hip_last_error()
    try:
        return _total(lib, ctx, h, probe)
    finally:
        lib.storm_hip_sparse_destroy(ctx._h, h)


def _pair_matrix(lib, ctx, arrays, stage):
    """The K5 per-pair matrix of the description, written into a sentinel-filled buffer: (matrix, mask)."""
    import torch
    n_rows = arrays[0]
    rc, l = _rowlists(lib, ctx, arrays, stage)
    assert rc == 0 and l.value, lib.storm_hip_last_error()
    try:
        dev = torch.full((n_rows, n_rows), SENTINEL, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()     # (the fill runs on torch's stream, the kernel on the context's)
        assert lib.storm_hip_rowlists_pairw_matrix_device(ctx._h, l, 0, C.c_void_p(dev.data_ptr()), n_rows) == 0, lib.storm_hip_last_error()
        ctx.synchronize()
        return dev.cpu().numpy().astype(np.int64), _ran(lib, ctx)
    finally:
        lib.storm_hip_rowlists_destroy(ctx._h, l)


def _check_pair_matrix(got, want):
    upper = np.triu(np.ones(want.shape, dtype=bool), k=1)
    assert (got[~upper] == SENTINEL).all()                  # entries i >= j are not written
    bad = np.argwhere((got != want) & upper)
    assert len(bad) == 0, (len(bad), [(int(i), int(j), int(got[i, j]), int(want[i, j])) for i, j in bad[:5]])


class Stage:
    def __init__(self, lib, ctx):
        self.lib, self.ctx, self.h = lib, ctx, C.c_void_p()
        assert lib.storm_hip_stage_create(ctx._h, C.byref(self.h)) == 0, lib.storm_hip_last_error()

    def add(self, words):
        tok = C.c_uint64(NONE)
        assert self.lib.storm_hip_stage_add(self.ctx._h, self.h, _p(words), C.byref(tok)) == 0, self.lib.storm_hip_last_error()
        return tok.value

    def add_list(self, lst):
        tok = C.c_uint64(NONE)
        assert self.lib.storm_hip_stage_add_list(self.ctx._h, self.h, _p(lst), len(lst), C.byref(tok)) == 0, self.lib.storm_hip_last_error()
        return tok.value

    def count(self):
        return int(self.lib.storm_hip_stage_count(self.h))

    def destroy(self):
        if self.h:
            self.lib.storm_hip_stage_destroy(self.ctx._h, self.h)
            self.h = None


# ---- the references ----
def _choose2_sum(counts):
    counts = counts.astype(np.int64)
    return int((counts * (counts - 1) // 2).sum())


def _bitmap_total(columns):
    """columns: per block column its blocks' words, (rows, 1024) uint64."""
    total = 0
    for words in columns:
        if len(words):
            bits = np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(len(words), 8192), axis=1, bitorder="little")
            total += _choose2_sum(bits.sum(axis=0, dtype=np.int64))
    return total


def _lists_total(columns):
    """columns: per block column its lists (arrays of positions)."""
    return sum(_choose2_sum(np.bincount(np.concatenate(lists).astype(np.int64), minlength=65536)) for lists in columns if lists)


def _pair_counts(n_rows, columns):
    """columns: per block column [(row, positions), ...] -> the (n_rows, n_rows) matrix of shared positions, int64."""
    want = np.zeros((n_rows, n_rows), dtype=np.int64)
    for members in columns:
        rows = np.array([r for r, _ in members], dtype=np.int64)
        B = np.zeros((len(members), 65536), dtype=np.float32)
        for k, (_, pos) in enumerate(members):
            B[k, pos] = 1.0
        want[np.ix_(rows, rows)] += (B @ B.T).astype(np.int64)
    return want


def _random_blocks(rng, n):
    """n bitmap blocks of varied density: every third one is the AND of two draws (a quarter of the bits set)."""
    words = rng.integers(0, 2 ** 64, size=(n, 1024), dtype=np.uint64)
    words[1::3] &= rng.integers(0, 2 ** 64, size=(len(words[1::3]), 1024), dtype=np.uint64)
    return words


# ---- a. the bitmap ring ----
@pytest.fixture(scope="module")
def ring_blocks():
    return _random_blocks(np.random.default_rng(601), 2 * BUF_BLOCKS + 1)


@pytest.mark.parametrize("n_blocks", (BUF_BLOCKS - 1, BUF_BLOCKS, BUF_BLOCKS + 1, 2 * BUF_BLOCKS, 2 * BUF_BLOCKS + 1))
def test_bitmap_ring_at_its_buffer_ends(hip_ctx, lib, ring_blocks, n_blocks):
    """511 blocks: a buffer that was never sent; 512: sent exactly full, the build finds an empty buffer; 513: the second
    buffer in use; 1024: both sent; 1025: the third fill has waited for the first buffer's event. Block b is row b // 4 of
    block column b % 4 (every third block is sparser: a block in the wrong column changes the total)."""
    n_cols = 4
    stage = Stage(lib, hip_ctx)
    try:
        d = Desc()
        for b in range(n_blocks):
            tok = stage.add(ring_blocks[b])
            assert tok == b
            d.block(b % n_cols, 1, ring_blocks[b], tok)
            if b % n_cols == n_cols - 1 or b == n_blocks - 1:
                d.end_row()
        assert stage.count() == n_blocks
        want = _bitmap_total([ring_blocks[c:n_blocks:n_cols] for c in range(n_cols)])
        got, ran = _arena_total(lib, hip_ctx, d.arrays(), stage.h)
        plain, ran_plain = _arena_total(lib, hip_ctx, d.arrays(), None)
        print(f"bitmap ring, {n_blocks} blocks: staged {got}, un-staged {plain}, numpy {want}, ran {ran} / {ran_plain}")
        assert got == want and plain == want
        assert ran == RAN_BIT_STRIPS and ran_plain == RAN_BIT_STRIPS      # columns of 128 rows and more: the matrix cores
    finally:
        stage.destroy()


# ---- b. the bitmap chunk boundary ----
def test_bitmap_buffer_that_runs_across_a_chunk_boundary(hip_ctx, lib):
    """131 rows x 64 block columns = 8384 blocks. The first 2 rows are staged and built from (a buffer of 128 blocks leaves
    early, so every later buffer starts at a token of 128 + 512 k); the buffer of tokens 7808 .. 8319 then crosses token
    8192 inside one send (stage_send's two copies), and the build of all 131 rows gathers from two chunks."""
    n_rows, n_cols, first = 131, 64, 2
    rng = np.random.default_rng(602)
    words = rng.integers(0, 2 ** 64, size=(n_rows, n_cols, 1024), dtype=np.uint64)
    words[::3] &= rng.integers(0, 2 ** 64, size=words[::3].shape, dtype=np.uint64)     # every third row is sparser
    words[:, 1::5] &= np.uint64(0x00FF00FF00FF00FF)                                       # and every fifth column
    stage = Stage(lib, hip_ctx)
    try:
        d = Desc()
        for r in range(n_rows):
            if r == first:
                few = d.copy()
                want_few = _bitmap_total([words[:first, c] for c in range(n_cols)])
                got_few, ran_few = _arena_total(lib, hip_ctx, few.arrays(), stage.h)
                print(f"bitmap chunk, first {first} rows: staged {got_few}, numpy {want_few}, ran {ran_few}")
                # columns of 2 rows: the popcount kernel over the pool's segments (variant 2), which has no flag of its own
                assert got_few == want_few and ran_few == 0 and hip_ctx.get_option("variant_used") == 2
            for c in range(n_cols):
                tok = stage.add(words[r, c])
                assert tok == r * n_cols + c
                d.block(c, 1, words[r, c], tok)
            d.end_row()
        assert stage.count() == n_rows * n_cols > CHUNK_BLOCKS
        assert (CHUNK_BLOCKS - first * n_cols) % BUF_BLOCKS != 0                          # a buffer does straddle the chunk's end
        want = _bitmap_total([words[:, c] for c in range(n_cols)])
        got, ran = _arena_total(lib, hip_ctx, d.arrays(), stage.h)
        plain, ran_plain = _arena_total(lib, hip_ctx, d.arrays(), None)
        print(f"bitmap chunk, {n_rows} rows: staged {got}, un-staged {plain}, numpy {want}, ran {ran} / {ran_plain}")
        assert got == want and plain == want
        assert ran == RAN_BIT_STRIPS and ran_plain == RAN_BIT_STRIPS
    finally:
        stage.destroy()


# ---- c. the list ring ----
def _ascending(rng, n):
    """n distinct positions of a block, ascending."""
    if n == 65536:
        return np.arange(65536, dtype=np.uint16)
    return np.flatnonzero(rng.permutation(65536) < n).astype(np.uint16)


def test_list_ring_at_its_buffer_end(hip_ctx, lib):
    """Lists of 30000 positions and a last one that ends the first buffer exactly at 4 MiB (it fits: not sent early); the
    same again with one position more (that list does not fit and opens the third fill, which reuses the first buffer);
    one list of 65536 positions; 14 MiB in all. One list per row, row r in block column r % 2. The arena takes all rows;
    the row lists (K5: rows of at most 65535 positions) all but the full one."""
    rng = np.random.default_rng(603)
    fit = LIST_BUF // 2 - 69 * 30000
    lengths = [30000] * 69 + [fit] + [30000] * 69 + [fit + 1] + [65536] + [30000] * 100 + [1, 65535]
    n_cols, full_row = 2, lengths.index(65536)      # (columns of 64 rows and more: the matrix-core variant, whose lists go to K4)
    lists = [_ascending(rng, n) for n in lengths]
    stage = Stage(lib, hip_ctx)
    try:
        d, k5 = Desc(), Desc()
        toks = []
        for r, lst in enumerate(lists):
            toks.append(stage.add_list(lst))
            d.block(r % n_cols, 0, lst, toks[-1])
            d.end_row()
            if r != full_row:
                k5.block(r % n_cols, 0, lst, toks[-1])
                k5.end_row()
        ends = [t + 2 * n for t, n in zip(toks, lengths)]
        assert toks[0] == 0 and toks[1:] == ends[:-1]                  # back to back: one chunk, no gap
        assert ends[69] == LIST_BUF and toks[70] == LIST_BUF           # the first buffer was exactly full ...
        assert ends[138] < 2 * LIST_BUF < ends[139]                    # ... the second left one position short of the next list
        assert 3 * LIST_BUF < ends[-1] <= LIST_CHUNK                   # both buffers reused; the builder reads the one chunk in place
        want = _lists_total([lists[c::n_cols] for c in range(n_cols)])
        got, ran = _arena_total(lib, hip_ctx, d.arrays(), stage.h)
        plain, ran_plain = _arena_total(lib, hip_ctx, d.arrays(), None)
        print(f"list ring: staged {got}, un-staged {plain}, numpy {want}, ran {ran} / {ran_plain}")
        assert got == want and plain == want
        assert ran == RAN_LIST_PROBE and ran_plain == RAN_LIST_PROBE   # list-only columns: probe_lists_kernel
        rows = [r for r in range(len(lists)) if r != full_row]
        want_pairs = _pair_counts(len(rows), [[(k, lists[r].astype(np.int64)) for k, r in enumerate(rows) if r % n_cols == c]
                                              for c in range(n_cols)])
        got_pairs, ran = _pair_matrix(lib, hip_ctx, k5.arrays(), stage.h)
        assert ran == RAN_LISTS_MATRIX
        _check_pair_matrix(got_pairs, want_pairs)
    finally:
        stage.destroy()


# ---- d. the list chunk boundary and its gap; g. refusals ----
class ChunkStage:
    """One list of 100 positions, then 16 block columns x 66 rows of lists of a random half of the block: 66 MiB. One list
    per row (K5 takes rows of at most 65535 positions): row 0 is the short list in column 0, row r >= 1 lies in column
    (r - 1) % 16."""
    N_COLS, PER_COL = 16, 66

    def __init__(self, lib, ctx):
        rng = np.random.default_rng(604)
        n = self.N_COLS * self.PER_COL
        bits = rng.integers(0, 2, size=(n, 65536), dtype=np.uint8)
        self.lists = [np.sort(rng.choice(65536, size=100, replace=False)).astype(np.uint16)]
        self.lists += [np.flatnonzero(bits[k]).astype(np.uint16) for k in range(n)]
        self.cols = [0] + [k % self.N_COLS for k in range(n)]
        self.lengths = [len(lst) for lst in self.lists]
        self.stage = Stage(lib, ctx)
        self.desc = Desc()
        self.toks = []
        for lst, c in zip(self.lists, self.cols):
            self.toks.append(self.stage.add_list(lst))
            self.desc.block(c, 0, lst, self.toks[-1])
            self.desc.end_row()
        self.members = [[(r, self.lists[r].astype(np.int64)) for r in range(len(self.lists)) if self.cols[r] == c]
                        for c in range(self.N_COLS)]
        self.total = _lists_total([[pos for _, pos in m] for m in self.members])


@pytest.fixture(scope="module")
def chunk_stage(hip_ctx, lib):
    s = ChunkStage(lib, hip_ctx)
    yield s
    s.stage.destroy()


def _jump(s):
    """(k, end of list k, token of list k + 1) of the one place where the tokens of the chunk stage are not back to back."""
    ends = [t + 2 * n for t, n in zip(s.toks, s.lengths)]
    jumps = [k for k in range(len(s.toks) - 1) if s.toks[k + 1] != ends[k]]
    assert len(jumps) == 1
    return jumps[0], ends[jumps[0]], s.toks[jumps[0] + 1]


def test_lists_in_two_chunks_are_tied_to_their_rows(hip_ctx, lib, chunk_stage):
    """The tokens jump at the 64 MiB boundary and leave a gap; the arena gathers the lists through the table
    (stage_gather_lists: more than one chunk) and K5's per-pair matrix ties every list — those of the second chunk too —
    to its row."""
    s = chunk_stage
    k, end, nxt = _jump(s)
    assert end < LIST_CHUNK == nxt and s.toks[-1] + 2 * s.lengths[-1] > LIST_CHUNK     # a non-empty gap, lists behind it
    assert all(t % 2 == 0 and t // LIST_CHUNK == (t + 2 * n - 1) // LIST_CHUNK for t, n in zip(s.toks, s.lengths))
    got, ran = _arena_total(lib, hip_ctx, s.desc.arrays(), s.stage.h)
    plain, ran_plain = _arena_total(lib, hip_ctx, s.desc.arrays(), None)
    print(f"list chunk: gap [{end}, {nxt}), staged {got}, un-staged {plain}, numpy {s.total}, ran {ran} / {ran_plain}")
    assert got == s.total and plain == s.total
    assert ran == RAN_LIST_PROBE and ran_plain == RAN_LIST_PROBE
    want_pairs = _pair_counts(len(s.lists), s.members)
    assert int(np.triu(want_pairs, k=1).sum()) == s.total
    got_pairs, ran = _pair_matrix(lib, hip_ctx, s.desc.arrays(), s.stage.h)
    assert ran == RAN_LISTS_MATRIX
    _check_pair_matrix(got_pairs, want_pairs)


def test_list_tokens_the_stage_cannot_answer_are_refused(hip_ctx, lib, chunk_stage):
    """storm_hip.h: an odd token, a token beyond the stage, a token in the gap in front of a chunk's end, a list that would
    run across a chunk's end and a list that runs past what its chunk holds are refused by both staged builders —
    STORM_HIP_EINVAL, *out NULL, the message names the stage token — on the host, before anything is sent or launched.
    (Until this test existed the gap and the straddling list were read.)"""
    s = chunk_stage
    k, end, nxt = _jump(s)
    last = len(s.toks) - 1
    cross = (LIST_CHUNK - s.toks[k]) // 2 + 1         # list k, the last of chunk 0, with a length that runs past the chunk's end
    assert s.lengths[k] < cross <= 65535
    cases = {"odd": (5, s.toks[5] + 1, None),
             "beyond the list space": (5, (s.toks[-1] // LIST_CHUNK + 1) * LIST_CHUNK, None),
             "far beyond the list space": (5, 1 << 40, None),
             "wraps around": (5, 2 ** 64 - 2, None),
             "in the gap": (0, end, None),              # (row 0: 100 positions; the gap is wider than that or not: refused either way)
             "the gap's last bytes": (0, nxt - 2, 1),
             "across the chunk's end": (k, s.toks[k], cross),
             "past what the last chunk holds": (last, s.toks[last], s.lengths[last] + 1)}
    for what, (b, tok, n) in cases.items():
        toks, lens = list(s.toks), list(s.lengths)
        toks[b] = tok
        if n is not None:
            lens[b] = n
        arrays = s.desc.arrays(toks=toks, lens=lens)
        for name, create in (("arena", _arena), ("row lists", _rowlists)):
            rc, h = create(lib, hip_ctx, arrays, s.stage.h)
            message = lib.storm_hip_last_error()
            message = message.decode() if isinstance(message, bytes) else str(message)
            assert rc == EINVAL and not h.value and "stage token" in message, (what, name, rc, h.value, message)
    # storm_hip_stage_add_list refuses 0 and 65537 positions and the stage is where it was
    some = np.arange(70000, dtype=np.uint16)
    for n in (0, 65537):
        tok = C.c_uint64(NONE)
        assert lib.storm_hip_stage_add_list(hip_ctx._h, s.stage.h, _p(some), n, C.byref(tok)) == EINVAL
    more = np.arange(10, dtype=np.uint16)
    assert s.stage.add_list(more) == s.toks[last] + 2 * s.lengths[last]
    # ... and the right tokens still build the right arena
    got, ran = _arena_total(lib, hip_ctx, s.desc.arrays(), s.stage.h)
    assert got == s.total and ran == RAN_LIST_PROBE


# ---- e. short lists from two chunks into K4 ----
def test_short_lists_of_two_chunks_through_the_probe_kernel_and_the_dense_path(hip_ctx, lib):
    """42100 lists of 800 positions (64.2 MiB: the last 157 lie in the second chunk, behind a gap of 64 bytes), 8 block
    columns, row r = blocks 8 r .. 8 r + 7: probe_lists_kernel (sparse_probe 1) and the dense path (0) on the same arena."""
    n_lists, n_pos, n_cols = 42100, 800, 8
    rng = np.random.default_rng(605)
    step = 65536 // n_pos
    lists = (rng.integers(0, step, size=(n_lists, n_pos), dtype=np.uint16) + np.arange(n_pos, dtype=np.uint16) * np.uint16(step))
    stage = Stage(lib, hip_ctx)
    try:
        d = Desc()
        toks = []
        for b in range(n_lists):
            toks.append(stage.add_list(lists[b]))
            d.block(b % n_cols, 0, lists[b], toks[-1])
            if b % n_cols == n_cols - 1 or b == n_lists - 1:
                d.end_row()
        toks = np.array(toks, dtype=np.int64)
        first1 = int(np.flatnonzero(toks >= LIST_CHUNK)[0])
        assert toks[first1] == LIST_CHUNK and toks[first1 - 1] + 2 * n_pos < LIST_CHUNK and first1 < n_lists - 1
        want = sum(_choose2_sum(np.bincount(lists[c::n_cols].ravel().astype(np.int64), minlength=65536)) for c in range(n_cols))
        rc, h = _arena(lib, hip_ctx, d.arrays(), stage.h)
        assert rc == 0 and h.value, lib.storm_hip_last_error()
        try:
            for probe, kernel in ((1, RAN_LIST_PROBE), (0, RAN_BIT_STRIPS), (-1, RAN_LIST_PROBE)):
                got, ran = _total(lib, hip_ctx, h, probe)
                print(f"short lists, sparse_probe {probe}: {got}, numpy {want}, ran {ran}")
                assert got == want and ran == kernel, (probe, got, want, ran)
        finally:
            lib.storm_hip_sparse_destroy(hip_ctx._h, h)
        plain, _ = _arena_total(lib, hip_ctx, d.arrays(), None)
        assert plain == want
    finally:
        stage.destroy()


# ---- f. where the bytes came from ----
def _positions_of(words):
    return np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little")).astype(np.int64)


def test_staged_blocks_and_block_ptr_are_told_apart(hip_ctx, lib, orc):
    """Every block is staged with content X while block_ptr holds content Y of the same lengths. storm_hip.h: the bitmaps
    come from the stage when EVERY bitmap token is below storm_hip_stage_count, else all from block_ptr; a list comes from
    the stage unless its token is ~0; the row lists come from the stage when every non-empty block carries a token, else all
    from block_ptr. 70 rows: column 0 bitmaps, column 1 bitmaps and lists in turn, columns 2 and 3 lists (one of them
    empty)."""
    rng = np.random.default_rng(606)
    n_rows = 70
    stage = Stage(lib, hip_ctx)
    try:
        d, k5 = Desc(), Desc()
        x, y = [], []                                  # per block of d: (column, kind, positions) of either content
        for r in range(n_rows):
            for c in range(4):
                bitmap = c == 0 or (c == 1 and r % 2 == 0)
                if bitmap:
                    wx, wy = _random_blocks(rng, 3)[r % 3], _random_blocks(rng, 3)[(r + 1) % 3]
                    tok = stage.add(wx)
                    d.block(c, 1, wy, tok)
                    x.append((c, 1, _positions_of(wx)))
                    y.append((c, 1, _positions_of(wy)))
                else:
                    n = 0 if (r, c) == (7, 2) else int(rng.integers(200, 1500))
                    lx, ly = _ascending(rng, n), _ascending(rng, n)
                    tok = stage.add_list(lx) if n else NONE
                    d.block(c, 0, ly, tok)
                    x.append((c, 0, lx.astype(np.int64)))
                    y.append((c, 0, ly.astype(np.int64)))
                    if c >= 2:
                        k5.block(c, 0, ly, tok)
            d.end_row()
            k5.end_row()
        n_blocks = len(x)
        kinds = np.array([kind for _, kind, _ in x])
        bitmaps, lists = np.flatnonzero(kinds == 1), np.flatnonzero((kinds == 0) & (np.array(d.lens) > 0))
        assert stage.count() == len(bitmaps) and 200 <= n_blocks <= 400

        def rows_of(choice, only_cols=None):
            """The container's rows as global positions, block b from x or y by choice[b]."""
            rows, b = [], 0
            for r in range(n_rows):
                row = []
                for c in range(4):
                    col, _, pos = (x if choice[b] else y)[b]
                    if only_cols is None or col in only_cols:
                        row.append(col * 65536 + pos)
                    b += 1
                rows.append(np.concatenate(row).astype(np.uint32))
            return rows

        def total_of(choice):
            chosen = [(x if choice[b] else y)[b] for b in range(n_blocks)]
            want = orc.storm(rows_of(choice)).pairw()
            assert want == sum(_choose2_sum(np.bincount(np.concatenate([pos for col, _, pos in chosen if col == c]), minlength=65536))
                               for c in range(4))
            return want

        all_x = np.ones(n_blocks, dtype=bool)
        bitmaps_y = all_x.copy()
        bitmaps_y[bitmaps] = False
        half_lists_y = all_x.copy()
        half_lists_y[lists[::2]] = False
        lists_y = all_x.copy()
        lists_y[lists] = False
        base = np.array(d.toks, dtype=np.uint64)

        def tokens(change):
            t = base.copy()
            for b, v in change.items():
                t[b] = v
            return t

        mixtures = {"every block staged": (tokens({}), all_x),
                    "one bitmap token = the stage's count": (tokens({bitmaps[3]: stage.count()}), bitmaps_y),
                    "one bitmap token = ~0": (tokens({bitmaps[-1]: NONE}), bitmaps_y),
                    "every second list ~0": (tokens({b: NONE for b in lists[::2]}), half_lists_y),
                    "every list ~0": (tokens({b: NONE for b in lists}), lists_y)}
        wants = {name: total_of(choice) for name, (_, choice) in mixtures.items()}
        assert len(set(wants.values())) == 4, wants          # the mixtures are told apart by their totals
        for name, (toks, _) in mixtures.items():
            got, ran = _arena_total(lib, hip_ctx, d.arrays(toks=toks), stage.h)
            print(f"dispatch, {name}: {got}, want {wants[name]}, ran {ran}")
            assert got == wants[name], (name, got, wants)
            assert ran == RAN_LIST_PROBE | RAN_BIT_STRIPS, (name, ran)
        plain, _ = _arena_total(lib, hip_ctx, d.arrays(), None)
        assert plain == total_of(~all_x)
        # the row lists of columns 2 and 3
        k5_blocks = [b for b in range(n_blocks) if x[b][0] >= 2]
        k5_toks = base[k5_blocks]
        k5_lens = np.array(k5.lens)
        one_none = k5_toks.copy()
        one_none[np.flatnonzero(k5_lens > 0)[11]] = NONE
        pair_wants = {}
        for name, toks, choice in (("every list staged", k5_toks, all_x), ("one list ~0", one_none, ~all_x)):
            pair_wants[name] = orc.storm(rows_of(choice, only_cols=(2, 3))).pair_counts().astype(np.int64)
            got_pairs, ran = _pair_matrix(lib, hip_ctx, k5.arrays(toks=toks), stage.h)
            assert ran == RAN_LISTS_MATRIX
            _check_pair_matrix(got_pairs, pair_wants[name])
        assert not np.array_equal(np.triu(pair_wants["every list staged"], k=1), np.triu(pair_wants["one list ~0"], k=1))
    finally:
        stage.destroy()
