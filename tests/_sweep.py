"""The seeded parity sweep of the lag, dosage, LD and top-k calls: the case generator, the plain numpy references and the
runner tests/test_gpu_sweep_ld.py, tools/soak_ld.py and `python -m tests._sweep` share. The checker, never the thing under
test: nothing here imports the library at module level, and no reference reads anything the library computed.

    cases(family, seed, count)      parameter records from np.random.default_rng([family id, seed]); a record holds everything
                                    that rebuilds its inputs (shapes, lag, k, measure or stat, missing share, option draws and
                                    an input seed)
    run_case(family, rec, ctx)      the case on the GPU, host and _device forms, against the references below; raises
                                    AssertionError with got, want and the first differing positions; returns Stats
    python -m tests._sweep --family F --seed S --case I      replays exactly that case

References: the unpacked 0/1 or 0/1/2/3 rows multiplied as float64 matrices in panels of columns (every sum is far below
2^53, so the products are exact, and BLAS keeps a case in milliseconds), ratios formed from those integers as
storm_similarity_math.h, storm_dosage_math.h and storm_ldscore_math.h describe them, NaN masks from integer comparisons
alone. tests/test_sweep_cases.py checks the references against per-sample Python loops and the headers' host builds."""
import argparse
import json
import sys

import numpy as np

FAMILIES = ("bits", "topk", "dosage", "dosage_lag", "ldscore", "prune")
N_MAX = 420
N_EDGES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 385, 420)
S_SET = (1, 2, 31, 32, 33, 96, 257, 1000)
M_SET = (64, 100, 1000, 4096, 65536, 70000)
LAG_SET = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, "n-1", "n", 10000)
K_SET = (1, 2, 8, 64, 127, 128)
MISSING_SET = (0.0, 0.1, 0.4)
MEASURES = ("jaccard", "cosine", "ld_d", "ld_r2")
SCORES = MEASURES + ("count",)
OPS = ("and", "or", "xor")
NAN_BITS = 0x7FC00000
NO_INDEX = 0xFFFFFFFF
SENTINEL = 0xDEADBEEF
SENTINEL_I32 = int(np.uint32(SENTINEL).view(np.int32))
GUARD = 5
GUARD_F, GUARD_I, GUARD_K = -77.5, 0x5EADBEEF, 0x77
PRUNE_MARGIN = 2.0 ** -20                      # tests/test_gpu_streams_ld.py's distance of every r^2 from min_r2


# ------------------------------------------------------------------------------------------ the case generator
def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _draw_n(rng):
    u = rng.random()
    if u < 0.10:
        return int(_pick(rng, (1, 2)))
    if u < 0.55:
        return int(_pick(rng, N_EDGES))
    return int(rng.integers(1, N_MAX + 1))


def _draw_samples(rng):
    return int(_pick(rng, S_SET)) if rng.random() < 0.5 else int(rng.integers(3, 3001))


def _draw_width(rng):
    return int(_pick(rng, M_SET)) if rng.random() < 0.5 else int(rng.integers(65, 70001))


def _draw_lag(rng, n):
    if rng.random() < 0.65:
        v = _pick(rng, LAG_SET)
        return max(n - 1, 1) if v == "n-1" else n if v == "n" else int(v)
    return int(rng.integers(1, 501))


def _bit_rows(rng, rec, n, width, contig):
    """how the bit rows of one container are made: synth.positions of `draws` draws or random_bits (density 0.5), and the
    rows replaced by an empty and a full one (a STORM_contiguous_t takes no empty row)"""
    gen = _pick(rng, ("positions", "random_bits"))
    draws = int(_pick(rng, (1, 7, 60, max(1, width // 16), max(1, width // 3))))
    rows = rng.permutation(n)
    empty = int(rows[0]) if (not contig and rng.random() < 0.35) else -1
    full = int(rows[-1]) if (n > 1 and rng.random() < 0.3) else -1
    return {"gen": gen, "draws": min(draws, 3000), "empty_row": empty, "full_row": full}


def _bits_case(rng):
    container = _pick(rng, ("contig", "storm_list", "storm_bitmap", "storm_rect", "hip"))
    n, width = _draw_n(rng), _draw_width(rng)
    rec = {"container": container, "n": n, "M": width, "max_lag": _draw_lag(rng, n), "pad": int(rng.integers(1, 8)),
           "off": int(rng.integers(0, 2)), "input_seed": int(rng.integers(1 << 31))}
    rec.update(_bit_rows(rng, rec, n, width, container == "contig"))
    if container == "storm_bitmap":                       # at least 4096 positions inside one 65536-bit block
        if width < 9000:
            rec["M"] = int(_pick(rng, (65536, 70000, int(rng.integers(9000, 70001)))))
        rec["gen"] = "random_bits"
        if n == 1:
            rec["empty_row"] = -1                         # the only row is the one with the bitmap block
    if container == "storm_list":                         # fewer than 4096 positions in any block
        rec["gen"], rec["full_row"] = "positions", -1
    if container == "storm_rect":
        rec["nb"] = 1 if rng.random() < 0.15 else _draw_n(rng)
        if rng.random() < 0.15:
            rec["n"], rec["max_lag"] = 1, 1
            rec["empty_row"] = rec["full_row"] = -1
        mb = _draw_width(rng)
        rec["Mb"] = mb if mb != rec["M"] else mb + 1
    return rec


def _topk_case(rng):
    form = _pick(rng, ("contig", "storm", "hip", "hip_cross", "storm_square"))
    n, width = _draw_n(rng), _draw_width(rng)
    rec = {"form": form, "n": n, "M": width, "k": int(_pick(rng, K_SET)), "score": _pick(rng, SCORES),
           "panel_rows": int(_pick(rng, (0, 256, 512))), "pad": int(rng.integers(0, 4)),
           "input_seed": int(rng.integers(1 << 31))}
    rec.update(_bit_rows(rng, rec, n, width, form == "contig"))
    if form in ("hip_cross", "storm_square"):
        rec["nb"] = 1 if rng.random() < 0.1 else _draw_n(rng)
    # half of the rows empty: under cosine and r^2 they have no candidate and are nobody's, under Jaccard only each other's
    rec["half_empty"] = bool(form != "contig" and rng.random() < 0.25)
    return rec


def _special_rows(rng, rec, n, samples):
    """rows that get a constant row, an all-missing row (missing > 0) and a row that is constant on what it shares with the
    row behind it (missing > 0, two samples or more): distinct rows where n allows it, -1 otherwise"""
    rows = [int(x) for x in rng.permutation(n)]
    rec["shared_row"] = -1
    if rec["missing"] > 0 and n >= 2 and samples >= 2 and rng.random() < 0.6:
        r = int(rng.integers(0, n - 1))
        rec["shared_row"] = r
        rows = [x for x in rows if x not in (r, r + 1)]
    rec["const_row"] = rows.pop() if rows and rng.random() < 0.6 else -1
    rec["const_value"] = int(rng.integers(0, 3))
    rec["allmiss_row"] = rows.pop() if rows and rec["missing"] > 0 and rng.random() < 0.6 else -1


def _dosage_base(rng):
    n, samples = _draw_n(rng), _draw_samples(rng)
    rec = {"n": n, "S": samples, "missing": float(_pick(rng, MISSING_SET)), "pad": int(rng.integers(1, 8)),
           "input_seed": int(rng.integers(1 << 31))}
    _special_rows(rng, rec, n, samples)
    return rec


def _dosage_case(rng):
    rec = _dosage_base(rng)
    rec["nb"] = 1 if rng.random() < 0.1 else _draw_n(rng)
    if rng.random() < 0.1:
        rec["n"] = 1
        rec["shared_row"] = rec["const_row"] = rec["allmiss_row"] = -1
    return rec


def _dosage_lag_case(rng):
    rec = _dosage_base(rng)
    rec["max_lag"] = _draw_lag(rng, rec["n"])
    return rec


def _window_draws(rng, rec):
    """positions (non-decreasing, steps of 0 .. 4, so equal positions occur) from a seed of their own, a distance, and how
    max_lag relates to what the windows need: "auto" (None), "exact", "more" (need + extra)"""
    rec["use_pos"] = bool(rng.random() < 0.5)
    rec["pos_seed"] = int(rng.integers(1 << 31))
    rec["max_dist"] = float(_pick(rng, (0.0, 1.0, 2.5, 9.0, 40.0, 130.0, 300.0)))
    rec["lag_mode"] = _pick(rng, ("auto", "exact", "more"))
    rec["lag_extra"] = int(_pick(rng, (1, 2, 64, 500)))


def _ldscore_case(rng):
    rec = _dosage_base(rng)
    rec["max_lag"] = _draw_lag(rng, rec["n"])
    rec["n_annot"] = int(_pick(rng, (1, 2, 63, 64, 65, 130))) if rng.random() < 0.6 else int(rng.integers(1, 131))
    rec["annot_stat"] = _pick(rng, ("r2", "r2_adj"))
    rec["annot_complete"] = bool(rng.random() < 0.5)
    _window_draws(rng, rec)
    rec["use_pos"] = True                                  # every case runs the annotated call with and without positions
    return rec


def _prune_case(rng):
    rec = _dosage_base(rng)
    rec["max_lag"] = _draw_lag(rng, rec["n"])
    rec["complete"] = bool(rng.random() < 0.5)
    rec["target"] = float(_pick(rng, (0.1, 0.2, 0.5, 0.8)))
    rec["priority"] = _pick(rng, ("none", "random", "ties"))
    _window_draws(rng, rec)
    return rec


_DRAW = {"bits": _bits_case, "topk": _topk_case, "dosage": _dosage_case, "dosage_lag": _dosage_lag_case,
         "ldscore": _ldscore_case, "prune": _prune_case}


def cases(family, seed, count):
    """`count` parameter records of the family, each with its `family`, `seed` and `index`"""
    rng = np.random.default_rng([FAMILIES.index(family), int(seed)])
    for index in range(count):
        rec = _DRAW[family](rng)
        rec.update(family=family, seed=int(seed), index=index)
        yield rec


# ------------------------------------------------------------------------------------------ inputs from a record
def random_bits_dense(rng, n, n_bits):
    """tests/test_gpu_lag_matrix.py's random_bits (density 0.5), unpacked: [n, n_bits] uint8"""
    from tests.test_gpu_lag_matrix import random_bits
    words = random_bits(rng, n, n_bits)
    return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :n_bits].copy()


def bit_matrix(rec, n, width, salt=0):
    """the [n, width] uint8 0/1 rows of one container of a bits or topk record"""
    from stormbitmaps_amd import synth
    rng = np.random.default_rng([rec["input_seed"], salt])
    if rec["gen"] == "random_bits":
        dense = random_bits_dense(rng, n, width)
    else:
        dense = np.zeros((n, width), dtype=np.uint8)
        for i, p in enumerate(synth.positions(width, n, rec["draws"], seed=rec["input_seed"] % 100003 + salt)):
            dense[i, p] = 1
    if rec.get("half_empty"):
        dense[rng.permutation(n)[: n // 2]] = 0
    if 0 <= rec["full_row"] < n:
        dense[rec["full_row"]] = 1
    if 0 <= rec["empty_row"] < n:
        dense[rec["empty_row"]] = 0
    if rec.get("container") == "contig" or rec.get("form") == "contig":
        for i in np.flatnonzero(dense.sum(axis=1) == 0):   # a STORM_contiguous_t appends no empty row
            dense[i, int(rng.integers(width))] = 1
    return dense


def pack_bits(dense):
    """[n, width] 0/1 -> [n, ceil(width / 64)] uint64, bit v in word v / 64"""
    n, width = dense.shape
    padded = np.zeros((n, (width + 63) // 64 * 64), dtype=np.uint8)
    padded[:, :width] = dense
    return np.ascontiguousarray(np.packbits(padded, axis=1, bitorder="little")).view(np.uint64)


def dosage_matrix(rec, n=None, salt=0):
    """the [n, S] uint8 dosages of a record: tests/_prune.py's rows with real LD, the record's missing share (value 3) and its
    special rows; salt != 0: the other side of a rectangle, which has no special rows"""
    from tests._prune import ld_rows
    n = rec["n"] if n is None else n
    samples = rec["S"]
    G = ld_rows(n, samples, [rec["input_seed"], salt], missing=rec["missing"])
    if salt:
        return G
    r = rec["shared_row"]
    if 0 <= r < n - 1:
        h = samples // 2
        G[r + 1, :h] = 3                                   # the two rows share the samples [h, S) at most
        G[r, h:] = 1                                       # ... where row r is constant
        G[r, :h] = np.arange(h) % 3
    if 0 <= rec["const_row"] < n:
        G[rec["const_row"]] = rec["const_value"]
    if 0 <= rec["allmiss_row"] < n:
        G[rec["allmiss_row"]] = 3
    return G


def positions_of(rec, n):
    rng = np.random.default_rng(rec["pos_seed"])
    return np.cumsum(rng.integers(0, 5, size=n)).astype(np.float64)


def annotations_of(rec, n):
    """[n, n_annot] float32: normal columns, a column of ones, binary columns, a column of zeros"""
    rng = np.random.default_rng([rec["input_seed"], 7])
    c = rec["n_annot"]
    a = rng.normal(size=(n, c)).astype(np.float32)
    a[:, 0] = 1.0
    for col in range(1, c):
        kind = col % 4
        if kind == 1:
            a[:, col] = rng.integers(0, 2, size=n)
        elif kind == 2 and col % 8 == 2:
            a[:, col] = 0.0
    return a


def priority_of(rec, n):
    rng = np.random.default_rng([rec["input_seed"], 9])
    if rec["priority"] == "none":
        return None
    p = rng.random(n, dtype=np.float32)
    return np.floor(p * 4).astype(np.float32) if rec["priority"] == "ties" else p


# ------------------------------------------------------------------------------------------ references
PANEL = 8192


def matmul_exact(A, B):
    """A @ B.T of small non-negative integer matrices [na, W], [nb, W] as int64: float64 products in panels of columns,
    every partial sum an integer far below 2^53"""
    A, B = np.asarray(A), np.asarray(B)
    out = np.zeros((A.shape[0], B.shape[0]), dtype=np.float64)
    for k in range(0, A.shape[1], PANEL):
        out += A[:, k:k + PANEL].astype(np.float64) @ B[:, k:k + PANEL].astype(np.float64).T
    return out.astype(np.int64)


def bit_counts(Da, Db=None):
    """(c [na, nb], a [na], b [nb]) int64: |A_i & B_j| and the rows' own counts"""
    Db = Da if Db is None else Db
    width = max(Da.shape[1], Db.shape[1])

    def widen(D):
        if D.shape[1] == width:
            return D
        out = np.zeros((D.shape[0], width), dtype=D.dtype)
        out[:, :D.shape[1]] = D
        return out
    return matmul_exact(widen(Da), widen(Db)), Da.sum(axis=1, dtype=np.int64), Db.sum(axis=1, dtype=np.int64)


def bit_ops(c, a, b):
    s = a[:, None] + b[None, :]
    return {"and": c, "or": s - c, "xor": s - 2 * c}


def similarity64(measure, c, a, b, M):
    """(value float64, undefined bool) of a measure or of "count", the operations of storm_similarity_math.h on the exact
    integers; the mask from integer comparisons"""
    c = np.asarray(c, dtype=np.int64)
    A = np.broadcast_to(np.asarray(a, dtype=np.int64)[:, None], c.shape)
    B = np.broadcast_to(np.asarray(b, dtype=np.int64)[None, :], c.shape)
    M = int(M)
    with np.errstate(divide="ignore", invalid="ignore"):
        if measure == "count":
            return c.astype(np.float64), np.zeros(c.shape, dtype=bool)
        if measure == "jaccard":
            u = A + B - c
            nan = u == 0
            v = c.astype(np.float64) / u.astype(np.float64)
        elif measure == "cosine":
            p = A * B
            nan = p == 0
            v = c.astype(np.float64) / np.sqrt(p.astype(np.float64))
        else:
            num = M * c - A * B
            d = np.abs(num).astype(np.float64)
            if measure == "ld_d":
                nan = np.zeros(c.shape, dtype=bool)
                v = np.where(num < 0, -1.0, 1.0) * (d / (float(M) * float(M)))
            else:
                nan = (A == 0) | (A >= M) | (B == 0) | (B >= M)
                v = (d * d) / ((A * (M - A)).astype(np.float64) * (B * (M - B)).astype(np.float64))
    return np.where(nan, 0.0, v), nan


def dosage_sums(Ga, Gb=None):
    """the exact integer sums of two sets of dosage rows, all [na, nb] or per row int64. Plain (3 is an ordinary value):
    P, s, q. Over the samples both rows have (3 = missing): N, Pc, sx (sum g_i m_j), sy, qx (sum g_i^2 m_j), qy; miss [na]."""
    Gb = Ga if Gb is None else Gb
    out = {"P": matmul_exact(Ga, Gb)}
    for G, tag in ((Ga, "i"), (Gb, "j")):
        g = G.astype(np.int64)
        out["s_" + tag], out["q_" + tag] = g.sum(axis=1), (g * g).sum(axis=1)
    za, zb = np.where(Ga == 3, 0, Ga), np.where(Gb == 3, 0, Gb)
    ma, mb = (Ga != 3).astype(np.uint8), (Gb != 3).astype(np.uint8)
    out["miss"] = (Ga == 3).sum(axis=1, dtype=np.int64)
    out["N"], out["Pc"] = matmul_exact(ma, mb), matmul_exact(za, zb)
    out["sx"], out["sy"] = matmul_exact(za, mb), matmul_exact(ma, zb)
    out["qx"], out["qy"] = matmul_exact(za * za, mb), matmul_exact(ma, zb * zb)
    return out


def _corr64(num, d_i, d_j, measure):
    """storm_dosage_math.h's lines on exact integers: r^2 = num^2 / (d_i d_j), r = +-|num| / sqrt(d_i d_j); NaN mask
    d_i == 0 or d_j == 0"""
    nan = (d_i == 0) | (d_j == 0)
    mag = np.abs(num).astype(np.float64)
    den = np.where(nan, 1, d_i).astype(np.float64) * np.where(nan, 1, d_j).astype(np.float64)
    if measure == "r2":
        v = (mag * mag) / den
    else:
        v = np.where(num < 0, -1.0, 1.0) * (mag / np.sqrt(den))
    return np.where(nan, 0.0, v), nan


def corr_plain64(sums, samples, measure):
    """(float64 value, undefined) of STORM_dosage_pairw_corr: over all samples, 3 an ordinary value"""
    S = int(samples)
    num = S * sums["P"] - sums["s_i"][:, None] * sums["s_j"][None, :]
    d_i = S * sums["q_i"] - sums["s_i"] ** 2
    d_j = S * sums["q_j"] - sums["s_j"] ** 2
    return _corr64(num, np.broadcast_to(d_i[:, None], num.shape), np.broadcast_to(d_j[None, :], num.shape), measure)


def corr_complete64(sums, measure):
    """(float64 value, undefined) of STORM_dosage_pairw_corr_complete: over the samples both rows have. Undefined covers
    N < 2 and a row constant on the shared samples: both make a d zero"""
    N = sums["N"]
    num = N * sums["Pc"] - sums["sx"] * sums["sy"]
    return _corr64(num, N * sums["qx"] - sums["sx"] ** 2, N * sums["qy"] - sums["sy"] ** 2, measure)


def ld_window(n, max_lag, pos=None, max_dist=None):
    """[n, n] bool: j is in row i's window: 1 <= |i - j| <= min(max_lag, n - 1) and, with positions, |pos_i - pos_j| <=
    max_dist. max_lag None: the positions alone."""
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    w = i != j
    if max_lag is not None:
        w &= np.abs(i - j) <= max_lag
    if pos is not None:
        w = w & (np.abs(pos[:, None] - pos[None, :]) <= max_dist)
    return w


def window_need(n, pos, max_dist):
    """the lag the windows of these positions need: the largest |i - j| inside a window"""
    w = ld_window(n, None, pos, max_dist)
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    return int(np.where(w, np.abs(i - j), 0).max(initial=0))


def ldscore_terms(r2, nan, N, stat):
    """(term float64, summed bool) per pair as storm_ldscore_math.h: r^2, or r^2 - (1 - r^2) / (N - 2) where N >= 3"""
    N = np.broadcast_to(np.asarray(N, dtype=np.int64), r2.shape)
    if stat == "r2":
        return r2, ~nan
    ok = ~nan & (N >= 3)
    with np.errstate(all="ignore"):
        t = r2 - (1.0 - r2) / np.where(ok, N - 2, 1).astype(np.float64)
    return np.where(ok, t, 0.0), ok


def ldscore_reference(r2, nan, N, stat, window, annot=None):
    """(want, magnitude, pairs): plain — per row the sum of the terms of the summed pairs of its window, the sum of their
    magnitudes, their number; annot [n, C] — the same per column with every term times the OTHER row's annotation"""
    t, ok = ldscore_terms(r2, nan, N, stat)
    summed = ok & window
    T = np.where(summed, t, 0.0)
    pairs = summed.sum(axis=1).astype(np.uint32)
    if annot is None:
        return T.sum(axis=1), np.abs(T).sum(axis=1), pairs
    a = annot.astype(np.float64)
    return T @ a, np.abs(T) @ np.abs(a), pairs


def prune_threshold(values, target):
    """min_r2 as float32 for a target t: the midpoint of the widest gap among the distinct in-window r^2 in
    (t - 0.05, t + 0.05) and the two ends; fewer than two distinct in-window values: t itself"""
    values = np.unique(np.asarray(values, dtype=np.float64))
    if values.size < 2:
        return np.float32(target)
    lo, hi = target - 0.05, target + 0.05
    pts = np.concatenate([[lo], values[(values > lo) & (values < hi)], [hi]])
    g = int(np.argmax(np.diff(pts)))
    return np.float32((pts[g] + pts[g + 1]) / 2)


def prune_margin(values, min_r2):
    """the smallest relative distance of an in-window r^2 from min_r2 (inf without values)"""
    values = np.asarray(values, dtype=np.float64)
    return float(np.abs(values - float(min_r2)).min(initial=np.inf) / float(min_r2))


# ------------------------------------------------------------------------------------------ comparing
class Stats:
    """what a run saw: cases, the worst ulp distance of a float from its reference, the worst error-to-bound ratio"""

    def __init__(self):
        self.cases, self.worst_ulp, self.worst_ratio, self.min_margin = 0, 0, 0.0, float("inf")

    def merge(self, other):
        self.cases += other.cases
        self.worst_ulp = max(self.worst_ulp, other.worst_ulp)
        self.worst_ratio = max(self.worst_ratio, other.worst_ratio)
        self.min_margin = min(self.min_margin, other.min_margin)

    def as_dict(self):
        return {"cases": self.cases, "worst_ulp": self.worst_ulp, "worst_ratio": round(self.worst_ratio, 4),
                "min_margin": None if self.min_margin == float("inf") else self.min_margin}


def ordered(bits):
    i = np.asarray(bits).astype(np.int64)
    return np.where(i & 0x80000000, -(i & 0x7FFFFFFF), i)


def bits_of(a):
    return np.ascontiguousarray(a).view(np.uint32)


def equal(got, want, what, where=None):
    """got == want (over `where`), or AssertionError with the first differing positions and both values there"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, "shape", got.shape, want.shape)
    diff = got != want
    if where is not None:
        diff = diff & where
    if diff.any():
        at = np.argwhere(diff)[:5]
        raise AssertionError(f"{what}: {int(diff.sum())} entries differ; first at {at.tolist()}: got "
                             f"{[got[tuple(p)].item() for p in at]}, want {[want[tuple(p)].item() for p in at]}")


def close_floats(stats, got_bits, want64, nan, where, what):
    """the 1-ulp rule: the one NaN pattern exactly on the integer mask, elsewhere at most 1 ulp from float32(want64)"""
    got_bits = np.asarray(got_bits, dtype=np.uint32)
    is_nan = (got_bits & 0x7FFFFFFF) > 0x7F800000
    equal(is_nan & where, nan & where, f"{what}: NaN mask")
    equal(got_bits, np.full(got_bits.shape, NAN_BITS, dtype=np.uint32), f"{what}: NaN pattern", nan & where)
    ok = where & ~nan
    want_bits = np.asarray(want64, dtype=np.float64).astype(np.float32).view(np.uint32)
    ulps = np.where(ok, np.abs(ordered(got_bits) - ordered(want_bits)), 0)
    worst = int(ulps.max(initial=0))
    stats.worst_ulp = max(stats.worst_ulp, worst)
    if worst > 1:
        at = np.argwhere(ulps > 1)[:5]
        raise AssertionError(f"{what}: up to {worst} ulp; first at {at.tolist()}: got "
                             f"{[float(got_bits[tuple(p)].view(np.float32)) for p in at]}, want {[float(want64[tuple(p)]) for p in at]}")


def within_bound(stats, score, want, limit, what):
    err = np.abs(np.asarray(score).astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / limit)
    stats.worst_ratio = max(stats.worst_ratio, float(ratio.max(initial=0.0)))
    if not (err <= limit).all():
        at = np.argwhere(~(err <= limit))[:5]
        raise AssertionError(f"{what}: error above the bound; first at {at.tolist()}: got {[float(np.asarray(score)[tuple(p)]) for p in at]}, "
                             f"want {[float(want[tuple(p)]) for p in at]}, bound {[float(limit[tuple(p)]) for p in at]}")


def lag_mask(n, L):
    return (np.arange(n)[:, None] + 1 + np.arange(L)[None, :]) < n


def to_lag(full, L, fill=0):
    """the pairs (i, i + 1 + d) of an [n, n] matrix in the lag layout [n, L], `fill` in the corner"""
    n = full.shape[0]
    ok = lag_mask(n, L)
    i = np.broadcast_to(np.arange(n)[:, None], ok.shape)
    j = i + 1 + np.arange(L)[None, :]
    out = np.full((n, L), fill, dtype=full.dtype)
    out[ok] = full[i[ok], j[ok]]
    return out


def upper(n):
    return np.triu(np.ones((n, n), dtype=bool), 1)


def device_words(rows, ld, off=0):
    """a sentinel-filled int32 device tensor of rows x ld words, `off` words behind a 16-byte boundary: (flat, 2-D view)"""
    import torch
    flat = torch.full((off + max(rows * ld, 1),), SENTINEL_I32, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    return flat, flat[off:off + rows * ld].view(rows, ld)


def read_words(flat, view, inside, what):
    """the view as uint32 after a call, once everything outside `inside` (guard rows, pitch columns, the words in front of
    the view) still holds the sentinel"""
    got = view.cpu().numpy().view(np.uint32)
    off = flat.numel() - max(view.numel(), 1)
    assert (flat[:off].cpu().numpy().view(np.uint32) == SENTINEL).all(), f"{what}: written in front of the output"
    full = np.zeros(got.shape, dtype=bool)
    full[:inside.shape[0], :inside.shape[1]] = inside
    equal(got, np.full(got.shape, SENTINEL, dtype=np.uint32), f"{what}: written outside the layout", ~full)
    return got[:inside.shape[0], :inside.shape[1]]


# ------------------------------------------------------------------------------------------ a. bit containers
def _bit_container(sb, ctx, kind, dense, width):
    if kind == "hip":
        return ctx.matrix_from_host(pack_bits(dense))
    s = sb.StormContig(width) if kind == "contig" else sb.Storm()
    for row in dense:
        p = np.flatnonzero(row).astype(np.uint32)
        s.add(p)
    assert s.n_rows == dense.shape[0], (kind, s.n_rows, dense.shape)
    return s


def _close(x):
    (x.close if hasattr(x, "close") else x.free)()


def run_bits(rec, ctx, stats):
    import ctypes as C
    import stormbitmaps_amd as sb
    from tests.test_gpu_similarity import check, expected
    kind, n, M, max_lag, pad, off = rec["container"], rec["n"], rec["M"], rec["max_lag"], rec["pad"], rec["off"]
    rng = np.random.default_rng([rec["input_seed"], 1])
    Da = bit_matrix(rec, n, M)
    if kind in ("storm_bitmap", "storm_list"):
        per_block = max(int(Da[:, b:b + 65536].sum(axis=1).max()) for b in range(0, M, 65536))
        assert (per_block >= 4096) == (kind == "storm_bitmap"), (kind, per_block)
    c, a, _ = bit_counts(Da)
    ops = bit_ops(c, a, a)
    L = min(max_lag, max(n - 1, 0))
    tri, inside = upper(n), lag_mask(n, L)
    n_bits = max(M, rec.get("Mb", 0))
    want = {ms: expected(ms, c, a, a, n_bits, rng) for ms in MEASURES}
    s = _bit_container(sb, ctx, "hip" if kind == "hip" else "contig" if kind == "contig" else "storm", Da, M)
    other = None
    try:
        host_tri = {}
        for ms in MEASURES:                                # ---- the triangle
            values, nan = want[ms]
            if kind == "hip":
                out = np.zeros((n, n), dtype=np.float32)
                assert sb.load().storm_hip_pairw_similarity(ctx._h, s._h, MEASURES.index(ms), n_bits,
                                                            out.ctypes.data_as(C.c_void_p), n) == 0, sb._lib.last_error()
                host = bits_of(out)
                flat, view = device_words(n + 2, n + pad, off)
                assert sb.load().storm_hip_pairw_similarity_device(ctx._h, s._h, MEASURES.index(ms), n_bits,
                                                                   C.c_void_p(view.data_ptr()), n + pad) == 0, sb._lib.last_error()
                ctx.synchronize()
                # (storm_hip.h: entries i >= j are "as the count kernel left them": only the rows and columns behind n are guarded)
                dev = read_words(flat, view, np.ones((n, n), dtype=bool), f"storm_hip_pairw_similarity_device {ms}")
                equal(dev, host, f"storm_hip_pairw_similarity_device {ms} against the host form", tri)
            else:
                host = bits_of(s.pairw_similarity(ms, n_bits=n_bits))
                equal(host, np.zeros((n, n), dtype=np.uint32), f"pairw_similarity {ms}: i >= j", ~tri)
                flat, view = device_words(n + 2, n + pad, off)
                s.pairw_similarity_device(view.data_ptr(), n + 2, n + pad, ms, n_bits=n_bits)
                dev = read_words(flat, view, tri if n >= 2 else np.zeros((n, n), bool), f"pairw_similarity_device {ms}")
                equal(dev, host, f"pairw_similarity_device {ms} against the host form", tri)
            stats.worst_ulp = max(stats.worst_ulp, check(host, values, nan, tri, ("pairw_similarity", ms)))
            host_tri[ms] = host
        if kind == "storm_rect":                           # ---- the rectangle against a container of another width
            nb, Mb = rec["nb"], rec["Mb"]
            Db = bit_matrix(dict(rec, empty_row=-1, full_row=-1), nb, Mb, salt=1)
            other = _bit_container(sb, ctx, "storm", Db, Mb)
            cr, ar, br = bit_counts(Da, Db)
            everywhere = np.ones((n, nb), dtype=bool)
            for ms in MEASURES:
                values, nan = expected(ms, cr, ar, br, n_bits, rng)
                host = bits_of(s.square_similarity(other, ms, n_bits=n_bits))
                stats.worst_ulp = max(stats.worst_ulp, check(host, values, nan, None, ("square_similarity", ms)))
                flat, view = device_words(n + 1, nb + pad, off)
                s.square_similarity_device(other, view.data_ptr(), n + 1, nb + pad, ms, n_bits=n_bits)
                equal(read_words(flat, view, everywhere, f"square_similarity_device {ms}"), host, f"square_similarity_device {ms}")
        for op in OPS:                                     # ---- counts in the lag layout
            ref = to_lag(ops[op], L).astype(np.uint32)
            host = s.pairw_lag_matrix(max_lag, op)
            equal(host, ref, f"pairw_lag_matrix {op}")     # 0 in the corner
            flat, view = device_words(n + 2, L + pad, off)
            if kind == "hip":
                s.pairw_lag_matrix_device(view.data_ptr(), L + pad, max_lag, op)
            else:
                s.pairw_lag_matrix_device(view.data_ptr(), n + 2, L + pad, max_lag, op)
            equal(read_words(flat, view, inside, f"pairw_lag_matrix_device {op}"), ref, f"pairw_lag_matrix_device {op}", inside)
        for ms in MEASURES:                                # ---- measures in the lag layout
            values, nan = want[ms]
            host = bits_of(s.pairw_lag_similarity(max_lag, ms, n_bits=n_bits))
            equal(host, np.zeros((n, L), dtype=np.uint32), f"pairw_lag_similarity {ms}: the corner", ~inside)
            stats.worst_ulp = max(stats.worst_ulp, check(host, to_lag(values, L), to_lag(nan, L, False), inside,
                                                         ("pairw_lag_similarity", ms)))
            equal(host, to_lag(host_tri[ms], L), f"pairw_lag_similarity {ms} against the triangle's bits", inside)
            flat, view = device_words(n + 2, L + pad, off)
            if kind == "hip":
                s.pairw_lag_similarity_device(view.data_ptr(), L + pad, max_lag, ms, n_bits)
            else:
                s.pairw_lag_similarity_device(view.data_ptr(), n + 2, L + pad, max_lag, ms, n_bits=n_bits)
            equal(read_words(flat, view, inside, f"pairw_lag_similarity_device {ms}"), host, f"pairw_lag_similarity_device {ms}",
                  inside)
    finally:
        _close(s)
        if other is not None:
            _close(other)


# ------------------------------------------------------------------------------------------ b. top-k
def check_topk_floats(stats, idx, val_bits, v64, nan, k, skip_self, what):
    """The five properties of a float top-k result against the float64 values v64 [n, m] (undefined where nan).

    A device value may sit one float from the rational, so two columns whose values are one ulp apart may legitimately swap,
    and the list cannot be compared with a ranking of the reference. Asserted instead, for every row:
      1. min(k, candidates) entries are listed, in front; the rest is padding (0xFFFFFFFF with the NaN pattern). A candidate
         is a defined entry and, in the pairwise forms, never the row itself.
      2. the listed columns are distinct candidates;
      3. each listed value is within 1 ulp of float32(v64) of its column;
      4. the listed (value, column) pairs are in the kernel's order: value descending, then column ascending;
      5. no unlisted candidate's float32 reference exceeds the last listed value by more than 2 ulps. The kernel ranks by its
         own floats: an unlisted candidate's device float u' is not above the last listed device float l'. Each of the two
         values compared may sit one ulp from the float32 of its float64 reference — u' up to 1 ulp below the reference u of
         its column, l' up to 1 ulp above the reference of its own — so u <= u' + 1 ulp <= l' + 1 ulp, and with the ulp of
         the listed side, 2 ulps: one for each of the two values compared."""
    n, m = v64.shape
    cand = ~nan
    if skip_self:
        cand[np.arange(min(n, m)), np.arange(min(n, m))] = False
    ref = ordered(np.where(nan, 0.0, v64).astype(np.float32).view(np.uint32))
    n_cand = cand.sum(axis=1)
    for r in range(n):
        cnt = int(min(k, n_cand[r]))
        cols, vals = idx[r, :cnt].astype(np.int64), ordered(val_bits[r, :cnt])
        where = f"{what}: row {r}: idx {idx[r].tolist()[:8]} val {val_bits[r].view(np.float32).tolist()[:8]}"
        assert (idx[r, cnt:] == NO_INDEX).all() and (val_bits[r, cnt:] == NAN_BITS).all(), f"{where}: padding behind {cnt} entries"
        assert (cols < m).all() and cand[r, cols].all() and np.unique(cols).size == cnt, f"{where}: not {cnt} distinct candidates"
        if not cnt:
            continue
        ulps = np.abs(vals - ref[r, cols])
        stats.worst_ulp = max(stats.worst_ulp, int(ulps.max()))
        assert ulps.max() <= 1, f"{where}: {int(ulps.max())} ulp from the reference {v64[r, cols].tolist()[:8]}"
        key = vals * (1 << 32) + (NO_INDEX - cols)
        assert (np.diff(key) < 0).all(), f"{where}: not in the kernel's order"
        if cnt < n_cand[r]:
            unlisted = cand[r].copy()
            unlisted[cols] = False
            over = ref[r][unlisted] - vals[-1]
            assert over.max() <= 2, (f"{where}: column {int(np.flatnonzero(unlisted)[np.argmax(over)])} is unlisted and "
                                     f"{int(over.max())} ulp above the last listed value")


def run_topk(rec, ctx, stats):
    import ctypes as C
    import stormbitmaps_amd as sb
    form, n, M, k, score, panel, pad = rec["form"], rec["n"], rec["M"], rec["k"], rec["score"], rec["panel_rows"], rec["pad"]
    cross = form in ("hip_cross", "storm_square")
    Da = bit_matrix(rec, n, M)
    nb = rec["nb"] if cross else n
    Db = bit_matrix(dict(rec, empty_row=-1, full_row=-1), nb, M, salt=1) if cross else Da
    c, a, b = bit_counts(Da, Db)
    v64, nan = similarity64(score, c, a, b, M)
    kind = {"contig": "contig", "storm": "storm", "storm_square": "storm"}.get(form, "hip")
    s = _bit_container(sb, ctx, kind, Da, M)
    other = _bit_container(sb, ctx, kind, Db, M) if cross else None
    try:
        if form == "hip_cross":
            host = s.cross_topk(other, k, score, n_bits=M, panel_rows=panel)
        elif form == "storm_square":
            host = s.square_topk(other, k, score, n_bits=M, panel_rows=panel)
        else:
            host = s.pairw_topk(k, score, n_bits=M, panel_rows=panel)
        flat_i, view_i = device_words(n + 1, k + pad)
        flat_v, view_v = device_words(n + 1, k + pad)
        di, dv = view_i.data_ptr(), view_v.data_ptr()
        if form == "hip_cross":
            assert sb.load().storm_hip_cross_dense_topk_device(ctx._h, s._h, other._h, SCORES.index(score), M, k, panel,
                                                               C.c_void_p(di), C.c_void_p(dv), k + pad) == 0, sb._lib.last_error()
        elif form == "storm_square":
            s.square_topk_device(other, di, dv, n + 1, k + pad, k, score, n_bits=M, panel_rows=panel)
        elif form == "hip":
            s.pairw_topk_device(di, dv, k + pad, k, score, n_bits=M, panel_rows=panel)
        else:
            s.pairw_topk_device(di, dv, n + 1, k + pad, k, score, n_bits=M, panel_rows=panel)
        ctx.synchronize()
        listed = np.ones((n, k), dtype=bool)
        dev = (read_words(flat_i, view_i, listed, "topk_device idx"), read_words(flat_v, view_v, listed, "topk_device val"))
        for (idx, val), name in ((host, "host"), (dev, "device")):
            what = f"{form} topk {score} k={k} ({name})"
            assert idx.shape == (n, k) and val.shape == (n, k), (what, idx.shape, val.shape)
            val_bits = bits_of(val)
            if score == "count":                           # integers: numpy's ranking itself
                cand = np.ones(c.shape, dtype=bool)
                if not cross:
                    cand[np.arange(n), np.arange(n)] = False
                order = np.argsort(np.where(cand, -c, 1), axis=1, kind="stable")[:, :k]     # value descending, column ascending
                want_i = np.full((n, k), NO_INDEX, dtype=np.uint32)
                want_v = np.zeros((n, k), dtype=np.uint32)
                take = np.take_along_axis(cand, order, axis=1)
                want_i[:, :order.shape[1]][take] = order.astype(np.uint32)[take]
                want_v[:, :order.shape[1]][take] = np.take_along_axis(c, order, axis=1).astype(np.uint32)[take]
                equal(idx, want_i, f"{what}: idx")
                equal(val_bits, want_v, f"{what}: val")
            else:
                check_topk_floats(stats, idx, val_bits, v64, nan.copy(), k, not cross, what)
        equal(dev[0], host[0], f"{form} topk {score}: the device form's idx against the host form's")
        equal(dev[1], bits_of(host[1]), f"{form} topk {score}: the device form's val against the host form's")
    finally:
        _close(s)
        if other is not None:
            _close(other)


# ------------------------------------------------------------------------------------------ c, d. dosage
def _dosage_container(sb, G):
    from tests.test_gpu_dosage import pack
    d = sb.StormDosage(G.shape[1])
    for i, row in enumerate(G):
        if i % 2 == 0:
            d.add(row)
        else:
            d.add_packed(pack(row[None, :]))
    assert d.n_rows == G.shape[0]
    return d


def _both_forms(call, rows, cols, pad, inside, host_fill, what):
    """call(device=None) and call(device=tensor): the host array as uint32 — `host_fill` outside `inside` — and the device
    window, equal on `inside` and untouched elsewhere, guard row and pitch columns included"""
    host = bits_of(call(None))
    assert host.shape == (rows, cols), (what, host.shape, (rows, cols))
    equal(host, np.full(host.shape, host_fill, dtype=np.uint32), f"{what}: outside the layout (host form)", ~inside)
    flat, view = device_words(rows + 1, cols + pad)
    assert call(view) is None
    dev = read_words(flat, view, inside, f"{what} (device form)")
    equal(dev, host, f"{what}: the device form against the host form", inside)
    return host


def run_dosage(rec, ctx, stats):
    import stormbitmaps_amd as sb
    n, nb, S, pad = rec["n"], rec["nb"], rec["S"], rec["pad"]
    Ga, Gb = dosage_matrix(rec), dosage_matrix(rec, nb, salt=1)
    sums = dosage_sums(Ga)
    tri = upper(n)
    d, other = _dosage_container(sb, Ga), _dosage_container(sb, Gb)
    try:
        s, q = d.row_sums()
        equal(s, sums["s_i"].astype(np.uint32), "row_sums: sum")
        equal(q, sums["q_i"].astype(np.uint32), "row_sums: sum of squares")
        equal(d.row_missing(), sums["miss"].astype(np.uint32), "row_missing")
        equal(_both_forms(lambda t: d.pairw_dot(device=t), n, n, pad, tri, 0, "pairw_dot"), sums["P"].astype(np.uint32),
              "pairw_dot", tri)
        equal(_both_forms(lambda t: d.pairw_nobs(device=t), n, n, pad, tri, 0, "pairw_nobs"), sums["N"].astype(np.uint32),
              "pairw_nobs", tri)
        rect = dosage_sums(Ga, Gb)["P"].astype(np.uint32)
        equal(_both_forms(lambda t: d.square_dot(other, device=t), n, nb, pad, np.ones((n, nb), bool), 0, "square_dot"), rect,
              "square_dot")
        for measure in ("r", "r2"):
            plain = _both_forms(lambda t: d.pairw_corr(measure, device=t), n, n, pad, tri, 0, f"pairw_corr {measure}")
            close_floats(stats, plain, *corr_plain64(sums, S, measure), tri, f"pairw_corr {measure}")
            comp = _both_forms(lambda t: d.pairw_corr_complete(measure, device=t), n, n, pad, tri, 0,
                               f"pairw_corr_complete {measure}")
            close_floats(stats, comp, *corr_complete64(sums, measure), tri, f"pairw_corr_complete {measure}")
            if not (Ga == 3).any():
                equal(comp, plain, f"pairw_corr_complete {measure} against pairw_corr without a missing value", tri)
    finally:
        d.free()
        other.free()


def run_dosage_lag(rec, ctx, stats):
    import stormbitmaps_amd as sb
    n, S, max_lag, pad = rec["n"], rec["S"], rec["max_lag"], rec["pad"]
    G = dosage_matrix(rec)
    sums = dosage_sums(G)
    L = min(max_lag, n - 1)
    inside = lag_mask(n, L)
    d = _dosage_container(sb, G)
    try:
        dot = _both_forms(lambda t: d.pairw_lag_dot(max_lag, device=t), n, L, pad, inside, 0, "pairw_lag_dot")
        equal(dot, to_lag(sums["P"], L).astype(np.uint32), "pairw_lag_dot", inside)
        equal(dot, to_lag(d.pairw_dot(), L), "pairw_lag_dot against pairw_dot", inside)
        nobs = _both_forms(lambda t: d.pairw_lag_nobs(max_lag, device=t), n, L, pad, inside, 0, "pairw_lag_nobs")
        equal(nobs, to_lag(sums["N"], L).astype(np.uint32), "pairw_lag_nobs", inside)
        equal(nobs, to_lag(d.pairw_nobs(), L), "pairw_lag_nobs against pairw_nobs", inside)
        for measure in ("r", "r2"):
            for name, ref, square in (("pairw_lag_corr", corr_plain64(sums, S, measure), d.pairw_corr),
                                      ("pairw_lag_corr_complete", corr_complete64(sums, measure), d.pairw_corr_complete)):
                band = _both_forms(lambda t: getattr(d, name)(max_lag, measure, device=t), n, L, pad, inside, 0, f"{name} {measure}")
                close_floats(stats, band, to_lag(ref[0], L), to_lag(ref[1], L, False), inside, f"{name} {measure}")
                equal(band, to_lag(bits_of(square(measure)), L), f"{name} {measure} against the n x n call's bits", inside)
    finally:
        d.free()


# ------------------------------------------------------------------------------------------ e. LD scores
def _r2_of(G, S, complete):
    """(r^2 float64 [n, n], undefined, N) of the rows, end to end from the unpacked dosages"""
    sums = dosage_sums(G)
    if complete:
        return corr_complete64(sums, "r2") + (sums["N"],)
    return corr_plain64(sums, S, "r2") + (np.full(sums["P"].shape, S, dtype=np.int64),)


def _vector_outputs(n, n_cols=None, pad=0):
    import torch
    score = torch.full((n + GUARD,) if n_cols is None else (n + GUARD, n_cols + pad), GUARD_F, dtype=torch.float32, device="cuda:0")
    pairs = torch.full((n + GUARD,), GUARD_I, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    return score, pairs


def refused(call, match, what):
    """the call raises RuntimeError whose message holds `match`"""
    try:
        call()
    except RuntimeError as e:
        assert match in str(e), f"{what}: refused with another message: {e}"
        return
    raise AssertionError(f"{what}: not refused")


def _window_lag(rec, need):
    return None if rec["lag_mode"] == "auto" or need == 0 else need if rec["lag_mode"] == "exact" else need + rec["lag_extra"]


def run_ldscore(rec, ctx, stats):
    import torch
    import stormbitmaps_amd as sb
    n, S, max_lag, pad = rec["n"], rec["S"], rec["max_lag"], rec["pad"]
    G = dosage_matrix(rec)
    pos, max_dist = positions_of(rec, n), rec["max_dist"]
    need = window_need(n, pos, max_dist)
    annot = annotations_of(rec, n)
    n_annot = annot.shape[1]
    d = _dosage_container(sb, G)
    try:
        assert d.ldscore_window_lag(pos, max_dist) == need, ("ldscore_window_lag", d.ldscore_window_lag(pos, max_dist), need)
        for complete in (False, True):
            r2, nan, N = _r2_of(G, S, complete)
            for stat in ("r2", "r2_adj"):                  # ---- the plain scores
                what = f"lag_ldscore {stat} complete={complete}"
                if stat == "r2_adj" and S < 3 and not complete:   # storm.h: _ADJ with n_samples < 3 is refused, nothing written
                    d_score, d_pairs = _vector_outputs(n)
                    refused(lambda: d.lag_ldscore(max_lag, stat, complete=complete), "at least 3 samples", what)
                    refused(lambda: d.lag_ldscore(max_lag, stat, complete=complete, device=(d_score, d_pairs)),
                            "at least 3 samples", what)
                    torch.cuda.synchronize()
                    assert (d_score.cpu().numpy() == np.float32(GUARD_F)).all() and (d_pairs.cpu().numpy() == GUARD_I).all(), what
                    continue
                want, mag, pairs = ldscore_reference(r2, nan, N, stat, ld_window(n, max_lag))
                score, got_pairs = d.lag_ldscore(max_lag, stat, complete=complete)
                equal(got_pairs, pairs, f"{what}: n_pairs")
                within_bound(stats, score, want, 2.0 ** -22 * (mag + 1.0), what)
                d_score, d_pairs = _vector_outputs(n)
                assert d.lag_ldscore(max_lag, stat, complete=complete, device=(d_score, d_pairs)) is None
                dev, dev_pairs = d_score.cpu().numpy(), d_pairs.cpu().numpy().view(np.uint32)
                rows = n if n >= 2 else 0                  # storm.h: fewer than two rows: 0, nothing written
                assert (dev[rows:] == np.float32(GUARD_F)).all() and (dev_pairs[rows:] == GUARD_I).all(), \
                    f"{what}: written behind row {rows}"
                equal(bits_of(dev[:rows]), bits_of(score[:rows]), f"{what}: the device form's bits")
                equal(dev_pairs[:rows], pairs[:rows], f"{what}: the device form's n_pairs")
        complete, stat = rec["annot_complete"], rec["annot_stat"]
        r2, nan, N = _r2_of(G, S, complete)
        d_annot = torch.from_numpy(annot).to("cuda:0")
        for use_pos in (False, True):                      # ---- the stratified scores
            lag = _window_lag(rec, need) if use_pos else max_lag
            kw = {"pos": pos, "max_dist": max_dist} if use_pos else {}
            what = f"lag_ldscore_annot {stat} complete={complete} pos={use_pos} max_lag={lag}"
            if stat == "r2_adj" and S < 3 and not complete:
                d_score, d_pairs = _vector_outputs(n, n_annot, pad)
                refused(lambda: d.lag_ldscore_annot(annot, lag, stat, complete=complete, **kw), "at least 3 samples", what)
                refused(lambda: d.lag_ldscore_annot(d_annot, lag, stat, complete=complete, device=(d_score, d_pairs), **kw),
                        "at least 3 samples", what)
                torch.cuda.synchronize()
                assert (d_score.cpu().numpy() == np.float32(GUARD_F)).all() and (d_pairs.cpu().numpy() == GUARD_I).all(), what
                continue
            window = ld_window(n, lag, pos if use_pos else None, max_dist)
            want, mag, pairs = ldscore_reference(r2, nan, N, stat, window, annot)
            a_abs = np.abs(annot.astype(np.float64))
            a_max = np.array([a_abs[window[r]].max(axis=0, initial=0.0) for r in range(n)]).reshape(n, n_annot)
            score, got_pairs = d.lag_ldscore_annot(annot, lag, stat, complete=complete, **kw)
            equal(got_pairs, pairs, f"{what}: n_pairs")
            within_bound(stats, score, want, 2.0 ** -22 * (mag + a_max), what)
            d_score, d_pairs = _vector_outputs(n, n_annot, pad)
            assert d.lag_ldscore_annot(d_annot, lag, stat, complete=complete, device=(d_score, d_pairs), **kw) is None
            dev, dev_pairs = d_score.cpu().numpy(), d_pairs.cpu().numpy().view(np.uint32)
            rows = n if n >= 2 else 0                      # storm.h: fewer than two rows: 0, nothing written
            assert (dev[rows:] == np.float32(GUARD_F)).all() and (dev[:, n_annot:] == np.float32(GUARD_F)).all() and \
                (dev_pairs[rows:] == GUARD_I).all(), f"{what}: written outside the output"
            equal(bits_of(dev[:rows, :n_annot]), bits_of(score[:rows]), f"{what}: the device form's bits")
            equal(dev_pairs[:rows], pairs[:rows], f"{what}: the device form's n_pairs")
        if need >= 2:                                      # ---- one below what the windows need: refused, nothing written
            d_score, d_pairs = _vector_outputs(n, n_annot, pad)
            what = f"lag_ldscore_annot at max_lag {need - 1} where the windows need {need}"
            refused(lambda: d.lag_ldscore_annot(d_annot, need - 1, "r2", complete=complete, pos=pos, max_dist=max_dist,
                                                device=(d_score, d_pairs)), str(need), what)
            refused(lambda: d.lag_ldscore_annot(annot, need - 1, "r2", complete=complete, pos=pos, max_dist=max_dist), str(need), what)
            torch.cuda.synchronize()
            assert (d_score.cpu().numpy() == np.float32(GUARD_F)).all() and (d_pairs.cpu().numpy() == GUARD_I).all(), \
                "a refused lag_ldscore_annot wrote something"
    finally:
        d.free()


# ------------------------------------------------------------------------------------------ f. pruning
def run_prune(rec, ctx, stats):
    import torch
    import stormbitmaps_amd as sb
    from tests import _prune
    n, S, complete = rec["n"], rec["S"], rec["complete"]
    G = dosage_matrix(rec)
    pos, max_dist = (positions_of(rec, n), rec["max_dist"]) if rec["use_pos"] else (None, None)
    need = window_need(n, pos, max_dist) if rec["use_pos"] else 0
    lag = _window_lag(rec, need) if rec["use_pos"] else rec["max_lag"]
    kw = {"pos": pos, "max_dist": max_dist} if rec["use_pos"] else {}
    r2, nan, _ = _r2_of(G, S, complete)
    pairs = ld_window(n, lag, pos, max_dist) & upper(n) & ~nan
    min_r2 = prune_threshold(r2[pairs], rec["target"])
    margin = prune_margin(r2[pairs], min_r2)
    stats.min_margin = min(stats.min_margin, margin)
    assert margin >= PRUNE_MARGIN, f"an in-window r^2 lies {margin:.3g} (relative) from min_r2 {float(min_r2)!r}: below 2^-20"
    edge = pairs & (r2 > float(min_r2))
    nb = [[] for _ in range(n)]
    for i, j in np.argwhere(edge):
        nb[int(i)].append(int(j))
        nb[int(j)].append(int(i))
    priority = priority_of(rec, n)
    ref_keep, ref_owner = _prune.greedy(nb, n, priority)
    d = _dosage_container(sb, G)
    try:
        what = f"lag_prune complete={complete} min_r2={float(min_r2)!r} max_lag={lag} pos={rec['use_pos']} priority={rec['priority']}"
        keep, owner = d.lag_prune(float(min_r2), lag, priority=priority, complete=complete, owner=True, **kw)
        equal(keep, ref_keep, f"{what}: keep")
        equal(owner, ref_owner, f"{what}: owner")
        equal(d.lag_prune(float(min_r2), lag, priority=priority, complete=complete, **kw), ref_keep, f"{what}: keep without owner")
        d_keep = torch.full((n + GUARD,), GUARD_K, dtype=torch.uint8, device="cuda:0")
        d_owner = torch.full((n + GUARD,), GUARD_I, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        assert d.lag_prune(float(min_r2), lag, priority=priority, complete=complete, device=(d_keep, d_owner), **kw) is None
        dev_keep, dev_owner = d_keep.cpu().numpy(), d_owner.cpu().numpy().view(np.uint32)
        assert (dev_keep[n:] == GUARD_K).all() and (dev_owner[n:] == GUARD_I).all(), f"{what}: written behind row n"
        if n >= 2:
            equal(dev_keep[:n], ref_keep, f"{what}: keep (device form)")
            equal(dev_owner[:n], ref_owner, f"{what}: owner (device form)")
    finally:
        d.free()


_RUN = {"bits": run_bits, "topk": run_topk, "dosage": run_dosage, "dosage_lag": run_dosage_lag, "ldscore": run_ldscore,
        "prune": run_prune}


def run_case(family, rec, ctx):
    """one case on the GPU; AssertionError names (family, seed, index) and the record"""
    stats = Stats()
    try:
        _RUN[family](rec, ctx, stats)
    except Exception as e:
        raise AssertionError(f"sweep case (family={family!r}, seed={rec.get('seed')}, index={rec.get('index')}) failed: "
                             f"{type(e).__name__}: {e}\nrecord: {json.dumps(rec, sort_keys=True)}\n"
                             f"replay: python -m tests._sweep --family {family} --seed {rec.get('seed')} --case {rec.get('index')}") from e
    stats.cases = 1
    return stats


def run_family(family, seed, count, ctx):
    total = Stats()
    for rec in cases(family, seed, count):
        total.merge(run_case(family, rec, ctx))
    return total


def main(argv=None):
    ap = argparse.ArgumentParser(description="replay one case of the parity sweep on the GPU")
    ap.add_argument("--family", required=True, choices=FAMILIES)
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--case", type=int, required=True)
    args = ap.parse_args(argv)
    import stormbitmaps_amd as sb
    rec = list(cases(args.family, args.seed, args.case + 1))[args.case]
    print("record:", json.dumps(rec, sort_keys=True))
    ctx = sb.HipContext(0)
    try:
        stats = run_case(args.family, rec, ctx)
    except AssertionError as e:
        print(e)
        return 1
    finally:
        ctx.close()
    print("ok:", json.dumps(stats.as_dict()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
