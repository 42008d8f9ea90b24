"""Inputs, closed forms and limit shapes shared by tests/test_gpu_dense_edges.py (GPU) and tests/test_dense_edge_shapes.py
(CPU). The input families are the ones whose pair counts are known without multiplying anything:

  saturated      every bit set                                   count = M
  odd-saturated  every bit but ONE (the same in every row) set   count = M - 1 (odd for even M)
  staircase      row i = its first L_i bits / its last S_j bits  count = min(L_i, L_j) / min(S_i, S_j) / max(0, L_i + S_j - M)
  periodic       bit b set iff b % p == t                        (numpy product)

and the shapes are the ones that put a dense kernel ON a bound it states in its comments (a count that must stay below
2^16, 2^24, a run of 4096 stages, ...). The CPU file asserts, with the host-only planners, that each shape really sits on
its limit; the GPU file asserts the numbers."""
import numpy as np

ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def n_words_of(n_bits: int) -> int:
    return (n_bits + 63) // 64


def prefix_rows(n_bits: int, lengths) -> np.ndarray:
    """Row i = bits [0, lengths[i]) set, as [n, ceil(n_bits / 64)] uint64 (bit v in word v / 64 at bit v % 64)."""
    L = np.asarray(lengths, dtype=np.int64)
    assert L.size == 0 or (L.min() >= 0 and L.max() <= n_bits)
    w = np.arange(n_words_of(n_bits), dtype=np.int64)
    nb = np.clip(L[:, None] - 64 * w[None, :], 0, 64)
    part = (np.uint64(1) << np.minimum(nb, 63).astype(np.uint64)) - np.uint64(1)
    return np.ascontiguousarray(np.where(nb == 64, ALL, part).astype(np.uint64))


def saturated(n_rows: int, n_bits: int, clear=()) -> np.ndarray:
    """Every bit of every row set (the last word masked), except the bit positions in `clear` (cleared in EVERY row)."""
    mat = prefix_rows(n_bits, np.full(n_rows, n_bits))
    for b in clear:
        mat[:, b // 64] &= ~(np.uint64(1) << np.uint64(b % 64))
    return mat


def staircase(n_bits: int, prefixes, suffixes=()) -> np.ndarray:
    """Rows of the first L bits for L in `prefixes`, then rows of the LAST S bits for S in `suffixes`."""
    top = prefix_rows(n_bits, prefixes)
    S = np.asarray(suffixes, dtype=np.int64)
    if S.size == 0:
        return top
    bottom = prefix_rows(n_bits, np.full(S.size, n_bits)) & ~prefix_rows(n_bits, n_bits - S)
    return np.ascontiguousarray(np.concatenate([top, bottom]))


def staircase_counts(n_bits: int, prefixes, suffixes=(), b_prefixes=None, b_suffixes=()):
    """(row counts of A, row counts of B, AND counts A x B) of two staircase matrices in closed form, int64. B defaults to A
    (the square whose upper triangle is the pairwise matrix)."""
    L, S = np.asarray(prefixes, dtype=np.int64), np.asarray(suffixes, dtype=np.int64)
    L2 = L if b_prefixes is None else np.asarray(b_prefixes, dtype=np.int64)
    S2 = S if b_prefixes is None else np.asarray(b_suffixes, dtype=np.int64)
    cross = lambda l, s: np.maximum(0, l[:, None] + s[None, :] - n_bits)
    cnt = np.block([[np.minimum(L[:, None], L2[None, :]), cross(L, S2)],
                    [cross(L2, S).T, np.minimum(S[:, None], S2[None, :])]])
    return np.concatenate([L, S]), np.concatenate([L2, S2]), cnt.astype(np.int64)


def op_counts(n_a, n_b, cnt, op: str) -> np.ndarray:
    """|a OP b| from the AND counts and the rows' own counts, int64."""
    s = np.asarray(n_a, dtype=np.int64)[:, None] + np.asarray(n_b, dtype=np.int64)[None, :]
    return {"and": cnt, "or": s - cnt, "xor": s - 2 * cnt}[op]


def staircase_lengths(n_bits: int, cut_chunks=()) -> list:
    """The lengths that walk every edge of k: words, 128-bit stages, 512-bit chunks, a trip of four chunks, the row's end,
    and one bit either side of every k-cut (in 512-bit chunks) a planner reports."""
    edges = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 2047, 2048, 2049, n_bits - 1, n_bits]
    for c in cut_chunks:
        edges += [512 * int(c) - 1, 512 * int(c), 512 * int(c) + 1]
    return sorted({e for e in edges if 0 <= e <= n_bits})


def periodic(n_bits: int, specs) -> np.ndarray:
    """Row (p, t): bit b set iff b % p == t."""
    b = np.arange(64 * n_words_of(n_bits), dtype=np.int64)
    bits = np.stack([((b % p) == t) & (b < n_bits) for p, t in specs]).astype(np.uint8)
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little").view(np.uint64))


PERIODIC_SPECS = tuple((p, t) for p in (2, 4, 8, 64, 128, 256, 512) for t in sorted({0, 1, 2, 3, p // 2, p - 1}) if t < p)


def numpy_counts(a: np.ndarray, b: np.ndarray = None, op: str = "and") -> np.ndarray:
    """The plain reference of the same operation: every bit unpacked, an int64 matrix product. [rows of a, rows of b]."""
    ua = np.unpackbits(np.ascontiguousarray(a).view(np.uint8), axis=1, bitorder="little").astype(np.int64)
    ub = ua if b is None else np.unpackbits(np.ascontiguousarray(b).view(np.uint8), axis=1, bitorder="little").astype(np.int64)
    return op_counts(ua.sum(axis=1), ub.sum(axis=1), ua @ ub.T, op)


def choose2(n: int) -> int:
    return n * (n - 1) // 2


# ---- case 1: K2h (tile128_kernel) k-parts at the limit of their 16-bit windows --------------------------------------------
# 254 chunks with k2_part_min_chunks 127: every tile in two `narrow` parts of exactly 127 chunks (65024 bits < 2^16);
# 256 chunks with min_chunks 128: two WIDE parts of 128 (65536 bits: what a 16-bit count cannot hold).
K2H_NARROW = {"n_words": 2032, "min_chunks": 127, "part_chunks": 127, "narrow": 1}
K2H_WIDE = {"n_words": 2048, "min_chunks": 128, "part_chunks": 128, "narrow": 0}
K2H_ROWS = (256, 300)
K2H_BAND = (65, 150)        # (row0, rows): starts inside a tile
K2H_RECT = (200, 257)       # (rows of A, rows of B)
K2H_SLOTS = (0, 1, 2)


def k2h_plans(dist, shape, n_cus: int, slots: int):
    """The K2h item lists of every launch case 1 makes with `shape` (triangles, the band, the rectangle)."""
    kw = dict(n_cus=n_cus, slots_per_cu=slots, min_chunks=shape["min_chunks"])
    plans = [dist.matrix_plan(n, shape["n_words"], **kw) for n in K2H_ROWS]
    plans.append(dist.matrix_plan(K2H_ROWS[1], shape["n_words"], band_row0=K2H_BAND[0], band_rows=K2H_BAND[1], **kw))
    plans.append(dist.matrix_plan(K2H_RECT[0], shape["n_words"], n_rows_b=K2H_RECT[1], **kw))
    return plans


def assert_k2h_on_limit(dist, shape, n_cus: int, slots: int):
    for plan in k2h_plans(dist, shape, n_cus, slots):
        assert len(plan) and (plan[:, 6] == 2).all(), (shape, n_cus, slots, "every tile in two parts")
        assert (plan[:, 3] == shape["part_chunks"]).all(), (shape, n_cus, slots, sorted(set(plan[:, 3].tolist())))
        assert (plan[:, 7] == shape["narrow"]).all(), (shape, n_cus, slots, "narrow flag")
        for t in np.unique(plan[:, 4]):       # the parts of a tile cover its chunks exactly once
            parts = plan[plan[:, 4] == t]
            assert sorted(parts[:, 2].tolist()) == [0, shape["part_chunks"]]


# ---- case 2: the 2^24 cut of the per-pair output kernels -------------------------------------------------------------------
EXACT = 1 << 24
EXACT_BITS = (EXACT - 512, EXACT, EXACT + 512, (1 << 25) - 512)    # (the last: 33553920 bits = 262140 stages of 128)
EXACT_SMALL_ROWS = 260      # two diagonal 256 x 256 tiles (one ragged: 4 rows) and the tile between them
K2H_WHOLE_ROWS = 2945       # 23 tiles of 128 rows and one ragged row: 300 tiles, 256 of them whole on 256 CUs
K2H_WHOLE_BITS = (EXACT - 512, EXACT + 512)


def assert_k2h_whole_tiles_on_limit(dist, n_cus: int):
    """At 2^24 - 512 bits the K2h plan holds WHOLE tiles of 32767 chunks (the longest item an f32 accumulator takes) and none
    longer; from 2^24 bits on every tile is cut and no part reaches 2^24 bits."""
    limit = (EXACT - 512) // 512
    p = dist.matrix_plan(K2H_WHOLE_ROWS, (EXACT - 512) // 64, n_cus=n_cus)
    whole = p[p[:, 6] == 1]
    assert len(whole) >= 256 and (whole[:, 3] == limit).all() and p[:, 3].max() == limit, (n_cus, len(whole), p[:, 3].max())
    for bits in (EXACT, EXACT + 512, (1 << 25) - 512):
        p = dist.matrix_plan(K2H_WHOLE_ROWS, bits // 64, n_cus=n_cus)
        assert (p[:, 6] >= 2).all() and p[:, 3].max() <= limit, (n_cus, bits, p[:, 6].min(), p[:, 3].max())


# ---- case 3: strip totals with the longest runs ----------------------------------------------------------------------------
STRIP_LONG_ROWS = (262400, 262465)   # 4100 / 4102 blocks of 64 rows: room for a run of 4096 later blocks
STRIP_LONG_WORDS = 8                 # one 512-bit chunk: two k-slices
STRIP_RUNS = ((1, 1), (0, 32), (4096, 4096))     # (k2_max_run, k2_tail_run); (0, 32) = the defaults (0: by the estimate)
STRIP_RAGGED_ROWS = (256, 257, 319, 320, 321, 511, 1280 + 63, 2048 + 255)   # N = 0, 1, 63, 64, 65, 255 (mod 256) and two longer
STRIP_RAGGED_BITS = (1024, 1088, 1000)           # a multiple of 512, of 64 only, of neither


def longest_run(dist, n_rows: int, n_words: int, form: int, max_run: int, tail_run: int, n_cus: int = 256) -> int:
    p = dist.strip_plan(n_rows, n_words, 0, 1, form=form, max_run=max_run, tail_run=tail_run, n_cus=n_cus)
    return int((p[:, 3].astype(np.int64) - p[:, 2].astype(np.int64)).max())


# ---- case 4: K2q with one workgroup per CU: shares at the guard -------------------------------------------------------------
STREAM_ROWS = (8192, 8191, 4097)
STREAM_BITS = 1 << 19
STREAM_MAX_STAGES = 8192             # kBsMaxStages
