"""The seeded parity sweep of the lag, dosage, LD and top-k calls: the case generator, the plain numpy references and the
runner tests/test_gpu_sweep_ld.py, tools/soak_ld.py and `python -m tests._sweep` share. The checker, never the thing under
test: nothing here imports the library at module level, and no reference reads anything the library computed.

    cases(family, seed, count)      parameter records from np.random.default_rng([family id, seed]); a record holds everything
                                    that rebuilds its inputs (shapes, lag, k, measure or stat, missing share, option draws and
                                    an input seed)
    run_case(family, rec, ctx)      the case on the GPU, host and _device forms, against the references below; raises
                                    AssertionError with got, want and the first differing positions; returns Stats
    python -m tests._sweep --family F --seed S --case I      replays exactly that case
    family "session" (section g)    lists of steps over live containers — mutations, option changes and queries interleaved —
                                    answered from a numpy model the runner mutates alongside the library; --upto K replays
                                    steps 0 .. K (tests/test_gpu_sweep_sessions.py)

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
    if family == SESSION:
        yield from _session_cases(seed, count)
        return
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


def check_topk(stats, idx, val, c, v64, nan, k, score, cross, what):
    """one top-k result (idx, val) of [n, k] against the counts c and the float64 values v64 (undefined where nan): by count
    numpy's ranking itself, by a float score the five properties of check_topk_floats"""
    n = c.shape[0]
    assert idx.shape == (n, k) and val.shape == (n, k), (what, idx.shape, val.shape)
    val_bits = bits_of(val)
    if score == "count":                                   # integers: numpy's ranking itself
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
            check_topk(stats, idx, val, c, v64, nan, k, score, cross, f"{form} topk {score} k={k} ({name})")
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


# ------------------------------------------------------------------------------------------ g. sessions
# A session record is a list of steps over a few LIVE containers: mutations, option changes and queries interleaved, every
# query answered from a numpy model of the containers that the runner mutates alongside the library. What is under test is
# the state that survives from one call to the next: the context's shared workspace and the containers' device mirrors.
SESSION = "session"
SESSION_ID = len(FAMILIES)                     # the family id in default_rng([family id, seed])
SESSION_KINDS = ("storm", "hip")               # record `index` even: storm.h containers on the library's own context; odd: HipMatrix
SESSION_THEMES = 3
STORM_BLOCKS, STORM_SPAN, STORM_NEAR = 3, 6144, 600   # a Storm's model: the first 6144 positions of 3 blocks of 65536 bits
STORM_BITS = STORM_BLOCKS * 65536
MUTATIONS = ("add", "clear", "upload", "resize", "set_rows_from_positions", "import_device", "free_new")
TOUR_MAX_ROWS = 160                            # the hand-over tour runs while every container is this small

# The query kinds, what each runs on ("bit": one bit container, "bit2": two, "dosage", "dosage2") and the buffers of
# storm_hip_ctx_s its launchers may touch, read from stormbitmaps_amd/csrc at the lines named. A Storm whose matrix comes
# from its lists (K5, K5x) touches none of the K2h buffers, and a Storm's total comes from its arena (K3 / K4), not from the
# strip list: the generator counts a hand-over as done only when both queries are off those paths (a StormContig, a
# dosage container, a HipMatrix; a Storm other than for "total" under matrix_lists 0 or, alone, with a bitmap block), and
# tests/test_sweep_cases.py counts the same way from the model.
_K2H = ("items", "d_parts", "d_tickets")       # the per-pair launchers through K2h: storm_hip_mfma.hip 2135 - 2158 (the 256 x 256 tiles: 2008 - 2038)
_OUT = _K2H + ("d_band",)                      # ... and the host form's staging, pair_matrix_out: storm_hip_internal.h 534
_CNT = ("d_counts",)
_SPLIT = ("d_dosage_rows", "d_dosage_sums")
QUERY_KINDS = {
    "total": ("bit", ("strips", "items")),               # storm_hip_mfma.hip 1671 (the strip list), 1756 (forgets the tile list)
    "square_total": ("bit2", ("strips",)),               # storm_hip_mfma.hip 1915: launch_square_mfma overwrites the strips, no key
    "pairw_matrix": ("bit", _OUT),
    "band": ("bit", _K2H),                               # storm_hip_pairw_matrix_band_device (hip sessions; device form only)
    "pairw_similarity": ("bit", _OUT + _CNT),            # storm_hip_similarity.hip 208
    "lag_matrix": ("bit", _OUT),
    "lag_similarity": ("bit", _OUT + _CNT),              # storm_hip_similarity.hip 316
    "topk": ("bit", _OUT + _CNT),                        # storm_hip_topk.hip 188 (the count panel in d_band), 194, 208
    "square_matrix": ("bit2", _OUT),
    "square_similarity": ("bit2", _OUT + _CNT),          # storm_hip_similarity.hip 208
    "square_topk": ("bit2", _OUT + _CNT),                # storm_hip_topk.hip 188, 194, 208
    "row_sums": ("dosage", _CNT),                        # storm_hip_dosage.hip 1118
    "row_missing": ("dosage", _CNT),                     # storm_hip_dosage.hip 1197
    "pairw_dot": ("dosage", _OUT),
    "pairw_corr": ("dosage", _OUT + _CNT),               # storm_hip_dosage.hip 306
    "pairw_nobs": ("dosage", _OUT + _SPLIT),             # storm_hip_dosage.hip 375, 397
    "pairw_corr_complete": ("dosage", _OUT + _SPLIT),
    "square_dot": ("dosage2", _OUT),
    "square_corr": ("dosage2", _OUT + _CNT + _SPLIT),    # storm_hip_dosage.hip 569; complete: 610, 647
    "square_nobs": ("dosage2", _OUT + _SPLIT),           # storm_hip_dosage.hip 610, 647
    "lag_dot": ("dosage", _OUT),
    "lag_corr": ("dosage", _OUT + _CNT),                 # storm_hip_dosage.hip 729
    "lag_nobs": ("dosage", _OUT + _SPLIT),               # storm_hip_dosage.hip 745, 793
    "lag_corr_complete": ("dosage", _OUT + _SPLIT),
    "lag_ldscore": ("dosage", _OUT + _CNT + _SPLIT),     # storm_hip_dosage.hip 818: the band of r^2 in d_band
    "lag_ldscore_annot": ("dosage", _OUT + _CNT + _SPLIT),
    "lag_prune": ("dosage", _OUT + _CNT + _SPLIT),       # storm_hip_prune.hip 348: masks, windows and order behind the band
}
SESSION_BUFFERS = ("items", "strips", "d_band", "d_tickets", "d_parts", "d_counts", "d_dosage_rows", "d_dosage_sums")
# (a HipMatrix answers the dosage kinds of the lag layout too: its rows read as 2-bit values, 32 samples per word)
HIP_QUERIES = ("total", "square_total", "pairw_matrix", "band", "pairw_similarity", "lag_matrix", "lag_similarity", "topk",
               "square_matrix", "square_topk", "lag_dot", "lag_corr", "lag_nobs", "lag_corr_complete", "lag_ldscore",
               "lag_ldscore_annot", "lag_prune")
STORM_QUERIES = tuple(k for k in QUERY_KINDS if k != "band")
# option, value: each one an existing GPU test sets while it asserts unchanged results — matrix_lists / matrix_lists_kernel:
# test_gpu_storm_edges.py COMBOS; k2_tile_shape: test_gpu_round5.py (2, 5), test_gpu_work_lists.py; k2_part_narrow:
# test_gpu_dosage.py, test_gpu_lag_matrix.py; k2_matrix_parts, k2_part_min_chunks, k2_strip_operands: test_gpu_work_lists.py;
# variant, keep_shadow: test_gpu_parity.py test_keep_shadow_follows_every_mutation
SESSION_OPTIONS = {
    "storm": (("matrix_lists", -1), ("matrix_lists", 0), ("matrix_lists", 1), ("matrix_lists_kernel", 0), ("matrix_lists_kernel", 1),
              ("matrix_lists_kernel", 2), ("k2_tile_shape", 0), ("k2_tile_shape", 2), ("k2_tile_shape", 5), ("k2_part_narrow", 0),
              ("k2_part_narrow", 1)),
    "hip": (("k2_tile_shape", 0), ("k2_tile_shape", 2), ("k2_tile_shape", 5), ("k2_matrix_parts", 0), ("k2_matrix_parts", 1),
            ("k2_part_min_chunks", 8), ("k2_part_min_chunks", 1), ("k2_part_min_chunks", 2), ("k2_strip_operands", 0),
            ("k2_strip_operands", 5), ("k2_strip_operands", 4), ("k2_strip_operands", 2), ("k2_part_narrow", 0), ("k2_part_narrow", 1),
            ("variant", -1), ("variant", 3), ("variant", 4), ("keep_shadow", 0), ("keep_shadow", 1)),
}
SESSION_DEFAULTS = {"matrix_lists": -1, "matrix_lists_kernel": 0, "k2_tile_shape": 0, "k2_part_narrow": 1, "k2_matrix_parts": 0,
                    "k2_part_min_chunks": 8, "k2_strip_operands": 0, "variant": -1, "keep_shadow": 0}


def session_queries(kind):
    return STORM_QUERIES if kind == "storm" else HIP_QUERIES


def session_handovers(kind):
    """{buffer: the ordered pairs of distinct query kinds of a session kind that both use it}"""
    names = session_queries(kind)
    return {buf: [(a, b) for a in names for b in names if a != b and buf in QUERY_KINDS[a][1] and buf in QUERY_KINDS[b][1]]
            for buf in SESSION_BUFFERS}


class _SessionGen:
    """draws the steps of one record; keeps the containers' row counts, nothing of their content"""

    def __init__(self, rng, kind, containers, todo, cursor):
        self.rng, self.kind, self.containers, self.todo, self.cursor = rng, kind, containers, todo, cursor
        self.steps, self.n, self.last = [], {cid: 0 for cid in containers}, None
        self.samples = next((c["S"] for c in containers.values() if c["type"] == "dosage"), 0) or \
            32 * next(c["words"] for c in containers.values() if c["type"] == "hip")
        self.lists, self.bitmap = -1, set()                # matrix_lists in force; the Storms that hold a bitmap block

    def of_type(self, *types):
        return [cid for cid, c in self.containers.items() if c["type"] in types]

    def option(self, key, value):
        self.steps.append({"op": "set_option", "key": key, "value": int(value)})
        if key == "matrix_lists":
            self.lists = int(value)

    def off_lists(self, kind, cid, other=None):
        """the query runs on the dense paths the table of buffers is about (see QUERY_KINDS)"""
        if self.containers[cid]["type"] != "storm":
            return True
        return kind != "total" and (self.lists == 0 or (other is None and cid in self.bitmap))

    def mutate(self, op, cid, witness=True, **kw):
        """a state-changing step and, right behind it, a query of `cid` whose shape or entries show it"""
        self.steps.append(dict(op=op, on=cid, **kw))
        ctype = self.containers[cid]["type"]
        if op == "add":
            self.n[cid] += kw["rows"]
            if kw.get("row_kind") == "bitmap":
                self.bitmap.add(cid)
        elif op in ("clear", "free_new") and ctype != "hip":
            self.n[cid] = 0
            self.bitmap.discard(cid)
        elif op in ("resize", "free_new"):
            self.n[cid] = kw["n"]
        if witness:
            wide = self.n[cid] > TOUR_MAX_ROWS
            if ctype == "dosage":
                kinds = ("pairw_dot", "pairw_corr", "lag_dot") if wide else ("pairw_dot", "pairw_corr", "pairw_nobs", "pairw_corr_complete")
            elif ctype == "hip" and self.n[cid] >= 2:      # the dosage launchers behind the mutations only a HipMatrix has
                kinds = ("pairw_matrix", "lag_matrix", "lag_nobs", "lag_corr_complete", "lag_corr") if wide else \
                    ("pairw_matrix", "pairw_similarity", "lag_nobs", "lag_corr_complete", "lag_corr", "lag_ldscore")
            else:
                kinds = ("pairw_matrix", "lag_matrix") if wide else ("pairw_matrix", "pairw_similarity")
            self.query(_pick(self.rng, kinds), cid, max_lag=int(self.n[cid]) + 1)

    def query(self, kind, cid=None, other=None, **fixed):
        rng, family = self.rng, QUERY_KINDS[kind][0]
        if cid is None:
            if self.kind == "storm" and family.startswith("bit") and self.lists != 0 and (family == "bit2" or rng.random() < 0.3):
                self.option("matrix_lists", 0)             # a Storm on its dense replica
            pool = self.of_type("dosage", "hip") if family.startswith("dosage") else \
                self.of_type("storm") if family == "bit2" and self.kind == "storm" else \
                [c for c in self.of_type("storm", "contig", "hip") if self.off_lists(kind, c)]
            picked = [pool[i] for i in rng.permutation(len(pool))[:2]]
            cid, other = picked[0], (picked[1] if family.endswith("2") else None)
        n = self.n[cid]
        st = {"op": "query", "kind": kind, "on": cid, "pad": int(rng.integers(1, 4)), "off": int(rng.integers(0, 2)),
              "max_lag": _draw_lag(rng, max(n, 1)), "bit_op": _pick(rng, OPS), "measure": _pick(rng, MEASURES),
              "k": int(_pick(rng, (1, 2, 8, 64))), "score": _pick(rng, SCORES), "world": int(rng.integers(1, 4)),
              "row0": int(rng.integers(0, max(n, 1))), "corr": _pick(rng, ("r", "r2")), "complete": bool(rng.random() < 0.5),
              "stat": _pick(rng, ("r2", "r2_adj")) if self.samples >= 3 else "r2", "n_annot": int(rng.integers(1, 6)),
              "target": float(_pick(rng, (0.1, 0.2, 0.5, 0.8))), "priority": _pick(rng, ("none", "random"))}
        if other is not None:
            st["other"] = other
        st.update(fixed)
        self.steps.append(st)
        off = self.off_lists(kind, cid, other)
        if self.last is not None and off:
            self.todo.discard((self.last, kind))
        self.last = kind if off else None

    def available(self, kind):
        family = QUERY_KINDS[kind][0]
        if family == "bit2":
            return len(self.of_type("storm" if self.kind == "storm" else "hip")) >= 2
        return True

    def tour(self, budget):
        """up to `budget` queries along hand-overs still to do, each from the kind the last query left behind where one
        starts there; now and then an option step or a small add in between"""
        rng = self.rng
        table = SESSION_OPTIONS[self.kind]
        for _ in range(budget):
            open_ = sorted(p for p in self.todo if self.available(p[0]) and self.available(p[1]))
            if not open_:
                return
            here = [p for p in open_ if p[0] == self.last]
            u = rng.random()
            if u < (0.35 if self.kind == "hip" else 0.10):  # the option table in its order, again and again
                self.option(*table[self.cursor[0] % len(table)])
                self.cursor[0] += 1                        # (carried from one session of a seed to the next, like the hand-overs)
            elif u < 0.14:
                cid = _pick(rng, sorted(self.n))
                if self.containers[cid]["type"] != "hip" and self.n[cid] < TOUR_MAX_ROWS - 8:
                    self.add(cid, int(rng.integers(1, 9)))
            elif u < 0.18 and self.kind == "storm":
                self.steps.append({"op": "hip_invalidate", "on": _pick(rng, self.of_type("storm", "contig"))})
            elif u < 0.45 and self.kind == "hip":
                cid = _pick(rng, sorted(self.n))
                if self.n[cid] >= 4:
                    self.mutate(_pick(rng, ("upload", "set_rows_from_positions", "import_device")), cid,
                                row0=int(rng.integers(0, self.n[cid] // 2)), rows=int(rng.integers(1, self.n[cid] // 2)))
            if here:
                self.query(_pick(rng, here)[1])
            else:
                self.query(_pick(rng, open_)[0])

    def add(self, cid, rows, row_kind="short", witness=True):
        rng, ctype = self.rng, self.containers[cid]["type"]
        kw = {"rows": int(rows)}
        if ctype == "storm":
            kw.update(row_kind=row_kind, block=int(rng.integers(1, STORM_BLOCKS)))
        elif ctype == "contig":
            kw["density"] = float(_pick(rng, (0.02, 0.3, 0.5)))
        elif ctype == "dosage":
            kw["missing"] = float(_pick(rng, MISSING_SET))
        self.mutate("add", cid, witness, **kw)


def _session_case(rng, index, todo, cursor):
    kind = SESSION_KINDS[index % 2]
    theme = (index // 2) % SESSION_THEMES
    fill = lambda: int(_pick(rng, (20, 31, 40, 63, 64, 65, 90, 127, 129)))
    if kind == "storm":
        samples = int(_pick(rng, S_SET))
        containers = {"s0": {"type": "storm"}, "c0": {"type": "contig", "width": int(_pick(rng, (64, 100, 1000, 4096)))},
                      "d0": {"type": "dosage", "S": samples}, "d1": {"type": "dosage", "S": samples}}
        if theme == 0 or rng.random() < 0.5:
            containers["s1"] = {"type": "storm"}
    else:
        words = int(_pick(rng, (1, 2, 5, 16, 33)))
        containers = {f"h{i}": {"type": "hip", "words": words, "n": fill()} for i in range(int(rng.integers(2, 4)))}
    g = _SessionGen(rng, kind, containers, todo, cursor)
    if kind == "storm":
        for cid in containers:
            g.add(cid, fill())
        _storm_theme(g, theme)
    else:
        for cid, c in containers.items():
            g.n[cid] = c["n"]
            g.mutate("upload", cid, row0=0, rows=c["n"])
        _hip_theme(g, theme)
    g.tour(90 if kind == "storm" else 50)
    return {"kind": kind, "theme": theme, "containers": containers, "options": [list(o) for o in SESSION_OPTIONS[kind]],
            "input_seed": int(rng.integers(1 << 31)), "steps": g.steps}


def _storm_theme(g, theme):
    rng = g.rng
    # every session: a mutation of B between two equal queries of A, a container freed between two queries of another, a lag
    # call right behind an n x n call of one container and the reverse, a dosage add behind a query
    g.query("pairw_similarity", "c0", measure="jaccard")
    g.add("d1", int(rng.integers(1, 20)))
    g.query("pairw_similarity", "c0", measure="jaccard")
    g.query("pairw_corr", "d0", corr="r2")
    g.mutate("free_new", "s0")
    g.query("pairw_corr", "d0", corr="r2")
    g.add("s0", int(rng.integers(10, 60)))
    for cid, square, lag in (("d0", "pairw_dot", "lag_dot"), ("c0", "pairw_matrix", "lag_matrix")):
        g.query(square, cid)
        g.query(lag, cid)
        g.query(square, cid)
    g.add("d0", int(rng.integers(1, 30)))
    if "s1" in g.containers:                               # the strip list: a total, the rectangle that overwrites it without a key, the total again
        g.option("matrix_lists", 0)
        g.query("total", "c0")
        g.query("square_total", "s0", "s1")
        g.query("total", "c0")
        g.option("matrix_lists", -1)
    if theme == 0:
        # K5: eligible, a bitmap block, eligible again behind clear — a query in each phase under matrix_lists 1 and -1
        for phase in range(3):
            if phase == 1:
                g.add("s0", int(rng.integers(1, 4)), "bitmap")
            if phase == 2:
                before = g.n["s0"]
                g.mutate("clear", "s0")
                g.add("s0", int(rng.integers(5, max(6, before - 3))))
            for lists in (1, -1):
                g.option("matrix_lists", lists)
                g.query("pairw_matrix", "s0")
        # the dense replica: built narrow, widened by a square call against a wider container, queried alone, grown, squared
        g.add("s1", int(rng.integers(1, 5)), "far")
        g.option("matrix_lists", 0)
        g.query("pairw_matrix", "s0")
        g.query("square_matrix", "s0", "s1")
        g.query("pairw_matrix", "s0")
        g.add("s0", int(rng.integers(3, 40)))
        g.query("square_matrix", "s0", "s1")
        g.option("matrix_lists", -1)
    elif theme == 1:
        # growth across 256, 512 and 1024 rows — the first crossing reallocates the mirror made at the fill — a query right
        # before and right after each; then clear and fewer rows than before
        for cid in ("d0", "c0"):
            for edge in (256, 512, 1024):
                g.add(cid, edge - int(rng.integers(0, 12)) - g.n[cid])
                g.add(cid, edge + int(rng.integers(1, 12)) - g.n[cid])
            g.mutate("clear", cid)
            g.add(cid, int(rng.integers(20, 120)))
    else:
        for cid in ("d1", "c0", "s0"):
            before = g.n[cid]
            g.mutate("clear", cid)
            g.query("total" if cid != "d1" else "row_sums", cid)          # an empty container
            g.add(cid, 1)                                                 # ... and one row
            g.query("topk" if cid != "d1" else "lag_prune", cid)
            g.add(cid, int(rng.integers(4, max(5, before - 2))))
        g.mutate("free_new", "d1")
        g.add("d1", int(rng.integers(10, 70)))
        if "s1" in g.containers:
            g.add("s1", 1, "far")
            g.add("s1", 1, "bitmap")


def _hip_theme(g, theme):
    rng = g.rng
    a, b = "h0", "h1"
    # keep_shadow 1 across an upload into the middle; B mutated between two queries of A; a lag call around an n x n call
    g.option("keep_shadow", 1)
    g.option("k2_strip_operands", 4)
    g.query("total", a, world=1)
    g.mutate("upload", a, witness=False, row0=int(g.n[a] // 3), rows=max(1, int(g.n[a] // 4)))
    g.query("total", a, world=1)
    g.query("pairw_matrix", a)
    g.option("k2_strip_operands", 0)
    g.query("total", a)                                    # the strip list: a total, the rectangle that overwrites it without a key, the total again
    g.query("square_total", a, b)
    g.query("total", a)
    g.query("pairw_matrix", b, bit_op="and")
    g.mutate("set_rows_from_positions", a, row0=int(rng.integers(0, g.n[a] // 2)), rows=int(rng.integers(1, g.n[a] // 2)))
    g.query("pairw_matrix", b, bit_op="and")
    g.query("lag_matrix", b)
    g.query("pairw_matrix", b)
    g.query("lag_matrix", b)
    g.mutate("import_device", b, row0=int(rng.integers(0, g.n[b] // 2)), rows=int(rng.integers(1, g.n[b] // 2)))
    # resize down and up inside the allocation (256 rows), then past it: 256, 512 and 1024 rows with a query on either side
    g.mutate("resize", a, n=int(rng.integers(1, max(2, g.n[a] // 2))))
    g.mutate("resize", a, n=int(rng.integers(130, 250)))
    g.mutate("upload", a, row0=100, rows=g.n[a] - 100)
    if theme == 1:
        for edge in (256, 512, 1024):
            g.mutate("resize", a, n=edge - int(rng.integers(0, 9)))
            g.mutate("upload", a, row0=g.n[a] - 40, rows=40)
            g.mutate("resize", a, n=edge + int(rng.integers(1, 9)))
            g.mutate("upload", a, row0=g.n[a] - 20, rows=20)
    g.mutate("clear", a)
    g.mutate("free_new", a, n=int(rng.integers(20, 130)))
    g.mutate("upload", a, row0=0, rows=g.n[a])
    g.option("keep_shadow", 0)


def _session_cases(seed, count):
    rng = np.random.default_rng([SESSION_ID, int(seed)])
    todo, cursor = {}, {kind: [0] for kind in SESSION_KINDS}
    for kind in SESSION_KINDS:                             # a third of the hand-overs to each seed
        pairs = sorted({p for ps in session_handovers(kind).values() for p in ps})
        todo[kind] = {p for i, p in enumerate(pairs) if i % 3 == int(seed) % 3}
    for index in range(count):
        rec = _session_case(rng, index, todo[SESSION_KINDS[index % 2]], cursor[SESSION_KINDS[index % 2]])
        rec.update(family=SESSION, seed=int(seed), index=index)
        yield rec


# ---- the model: one dense matrix per container (bits 0 / 1; dosages 0 .. 3, 3 = missing), mutated step by step
def session_rows(rec, i):
    """the rows that step i of a record adds or writes, as the model holds them"""
    from tests._prune import ld_rows
    st = rec["steps"][i]
    c = rec["containers"][st["on"]]
    k = st["rows"]
    rng = np.random.default_rng([rec["input_seed"], i])
    if c["type"] == "dosage":
        return ld_rows(k, c["S"], [rec["input_seed"], i], missing=st["missing"])
    if c["type"] == "contig":
        D = (rng.random((k, c["width"])) < st["density"]).astype(np.uint8)
        for r in np.flatnonzero(D.sum(axis=1) == 0):       # a STORM_contiguous_t appends no empty row
            D[r, int(rng.integers(c["width"]))] = 1
        return D
    if c["type"] == "hip":
        words = rng.integers(0, 1 << 63, size=(k, c["words"]), dtype=np.uint64) * np.uint64(2) + \
            rng.integers(0, 2, size=(k, c["words"]), dtype=np.uint64)
        if st["op"] == "set_rows_from_positions":
            words &= rng.integers(0, 1 << 63, size=(k, c["words"]), dtype=np.uint64)
        return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")
    D = np.zeros((k, STORM_BLOCKS * STORM_SPAN), dtype=np.uint8)
    for r in range(k):
        special = r == 0 and st["row_kind"] != "short"
        base = st["block"] * STORM_SPAN if special and st["row_kind"] == "far" else 0
        if special and st["row_kind"] == "bitmap":         # 4096 positions or more in one block
            D[r, rng.choice(STORM_SPAN, size=int(rng.integers(4096, 5000)), replace=False)] = 1
        else:
            D[r, base + rng.choice(STORM_NEAR, size=int(rng.integers(0 if r % 7 == 3 else 1, 61)), replace=False)] = 1
    return D


def storm_positions(row):
    """the sorted positions a row of a Storm's model stands for"""
    cols = np.flatnonzero(row)
    return ((cols // STORM_SPAN) * 65536 + cols % STORM_SPAN).astype(np.uint32)


class SessionModel:
    """the numpy state of a session's containers; every array is replaced, never written, so a snapshot is a dict copy"""

    def __init__(self, rec):
        self.rec, self.m, self.version, self.cache = rec, {}, {}, {}
        for cid, c in rec["containers"].items():
            self.m[cid] = np.zeros((c.get("n", 0), self.width(cid)), dtype=np.uint8)
            self.version[cid] = 0

    def width(self, cid):
        c = self.rec["containers"][cid]
        return {"storm": STORM_BLOCKS * STORM_SPAN, "contig": c.get("width"), "dosage": c.get("S"), "hip": 64 * c.get("words", 0)}[c["type"]]

    def type(self, cid):
        return self.rec["containers"][cid]["type"]

    def n_bits(self, cid):
        return STORM_BITS if self.type(cid) == "storm" else self.width(cid)

    def snapshot(self):
        other = SessionModel.__new__(SessionModel)
        other.rec, other.m, other.version, other.cache = self.rec, dict(self.m), dict(self.version), self.cache
        return other

    def apply(self, i):
        st = self.rec["steps"][i]
        op, cid = st["op"], st.get("on")
        if op not in MUTATIONS:
            return
        old = self.m[cid]
        if op == "add":
            new = np.vstack([old, session_rows(self.rec, i)])
        elif op == "clear":
            new = np.zeros_like(old) if self.type(cid) == "hip" else old[:0]
        elif op == "free_new":
            new = np.zeros((st.get("n", 0), old.shape[1]), dtype=np.uint8)
        elif op == "resize":
            new = np.zeros((st["n"], old.shape[1]), dtype=np.uint8)
            keep = min(st["n"], old.shape[0])
            new[:keep] = old[:keep]
        else:                                              # upload, import_device: rows [row0, row0 + rows) replaced
            new = old.copy()
            rows = session_rows(self.rec, i)
            if op == "set_rows_from_positions":            # sets the listed bits and leaves the others (storm_hip.h: "replaces the
                rows = rows | old[st["row0"]:st["row0"] + st["rows"]]   # bit-setting loop of STORM_contig_add": set_bits_kernel)
            new[st["row0"]:st["row0"] + st["rows"]] = rows
        self.m[cid] = new
        self.version[cid] = i + 1

    def _cached(self, tag, a, b, make):
        key = (tag, a, self.version[a], b, self.version.get(b))
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]

    def counts(self, a, b=None):
        def make():
            Da, Db = self.m[a], self.m[a if b is None else b]
            used = Da.any(axis=0) | Db.any(axis=0)         # columns no row has add nothing to a count
            return bit_counts(Da[:, used], None if b is None else Db[:, used])
        return self._cached("counts", a, b, make)

    def sums(self, a, b=None):
        return self._cached("sums", a, b, lambda: dosage_sums(self.dosages(a), None if b is None else self.dosages(b)))

    def dosages(self, a):
        """the rows as values 0 .. 3: a dosage container's own, a HipMatrix's bits read two at a time"""
        return self.m[a] if self.type(a) == "dosage" else self.m[a][:, 0::2] + 2 * self.m[a][:, 1::2]

    def samples(self, a):
        return self.dosages(a).shape[1]


def session_annot(rec, i, n, c):
    a = np.random.default_rng([rec["input_seed"], i, 7]).normal(size=(n, c)).astype(np.float32)
    a[:, 0] = 1.0
    return a


def session_answer(model, i):
    """what query step i must return, from the model alone: {name: array}, a float entry as (float64 value, undefined, where)"""
    st = model.rec["steps"][i]
    kind, on, other = st["kind"], st["on"], st.get("other")
    n = model.m[on].shape[0]
    L = min(st["max_lag"], max(n - 1, 0))
    family = QUERY_KINDS[kind][0]
    if family.startswith("bit"):
        c, a, b = model.counts(on, other)
        where = np.ones(c.shape, dtype=bool) if other is not None else upper(n)
        M = max(model.n_bits(on), model.n_bits(other or on))
        if kind in ("total", "square_total"):
            return {"total": np.asarray(int(c[where].sum()))}
        if kind in ("pairw_matrix", "square_matrix"):
            return {"counts": np.where(where, bit_ops(c, a, b)[st["bit_op"]], 0).astype(np.uint32), "where": where}
        if kind == "band":
            r0 = min(st["row0"], max(n - 1, 0))
            rows = min(max(n - r0, 0), 1 + st["k"])
            return {"counts": np.where(where, bit_ops(c, a, b)[st["bit_op"]], 0).astype(np.uint32)[r0:r0 + rows],
                    "where": where[r0:r0 + rows]}
        if kind in ("pairw_similarity", "square_similarity"):
            v, nan = similarity64(st["measure"], c, a, b, M)
            return {"value": (v, nan, where)}
        if kind == "lag_matrix":
            return {"counts": to_lag(bit_ops(c, a, b)[st["bit_op"]], L).astype(np.uint32), "where": lag_mask(n, L)}
        if kind == "lag_similarity":
            v, nan = similarity64(st["measure"], c, a, b, M)
            return {"value": (to_lag(v, L), to_lag(nan, L, False), lag_mask(n, L))}
        v, nan = similarity64(st["score"], c, a, b, M)      # topk, square_topk
        return {"counts": c, "topk": (v, nan, np.ones(c.shape, dtype=bool))}
    S = model.samples(on)
    sums = model.sums(on, other)
    where = np.ones(sums["P"].shape, dtype=bool) if other is not None else upper(n)
    inside = lag_mask(n, L)
    if kind == "row_sums":
        return {"sum": sums["s_i"].astype(np.uint32), "sum_sq": sums["q_i"].astype(np.uint32)}
    if kind == "row_missing":
        return {"missing": sums["miss"].astype(np.uint32)}
    if kind in ("pairw_dot", "square_dot"):
        return {"counts": np.where(where, sums["P"], 0).astype(np.uint32), "where": where}
    if kind in ("pairw_nobs", "square_nobs"):
        return {"counts": np.where(where, sums["N"], 0).astype(np.uint32), "where": where}
    if kind in ("pairw_corr", "pairw_corr_complete", "square_corr"):
        complete = kind == "pairw_corr_complete" or (kind == "square_corr" and st["complete"])
        v, nan = corr_complete64(sums, st["corr"]) if complete else corr_plain64(sums, S, st["corr"])
        return {"value": (v, nan, where)}
    if kind in ("lag_dot", "lag_nobs"):
        return {"counts": to_lag(sums["P" if kind == "lag_dot" else "N"], L).astype(np.uint32), "where": inside}
    if kind in ("lag_corr", "lag_corr_complete"):
        v, nan = corr_complete64(sums, st["corr"]) if kind == "lag_corr_complete" else corr_plain64(sums, S, st["corr"])
        return {"value": (to_lag(v, L), to_lag(nan, L, False), inside)}
    complete = st["complete"]
    r2, nan = corr_complete64(sums, "r2") if complete else corr_plain64(sums, S, "r2")
    N = sums["N"] if complete else np.full(sums["P"].shape, S, dtype=np.int64)
    window = ld_window(n, st["max_lag"])
    if kind == "lag_ldscore":
        want, mag, pairs = ldscore_reference(r2, nan, N, st["stat"], window)
        return {"score": want, "bound": 2.0 ** -22 * (mag + 1.0), "pairs": pairs}
    if kind == "lag_ldscore_annot":
        annot = session_annot(model.rec, i, n, st["n_annot"])
        want, mag, pairs = ldscore_reference(r2, nan, N, st["stat"], window, annot)
        a_abs = np.abs(annot.astype(np.float64))
        a_max = np.array([a_abs[window[r]].max(axis=0, initial=0.0) for r in range(n)]).reshape(n, st["n_annot"])
        return {"score": want, "bound": 2.0 ** -22 * (mag + a_max), "pairs": pairs, "annot": annot}
    from tests import _prune                               # lag_prune
    pairs = window & upper(n) & ~nan
    min_r2 = prune_threshold(r2[pairs], st["target"])
    edge = pairs & (r2 > float(min_r2))
    nb = [[] for _ in range(n)]
    for a, b in np.argwhere(edge):
        nb[int(a)].append(int(b))
        nb[int(b)].append(int(a))
    priority = None if st["priority"] == "none" else np.random.default_rng([model.rec["input_seed"], i, 9]).random(n, dtype=np.float32)
    keep, owner = _prune.greedy(nb, n, priority)
    return {"keep": keep, "owner": owner, "min_r2": np.asarray(min_r2), "margin": np.asarray(prune_margin(r2[pairs], min_r2)),
            "priority": priority}


def answers_differ(a, b):
    """two answers of one query step differ in shape or in at least one entry"""
    flat = lambda ans: [np.asarray(x) for v in ans.values() if v is not None for x in (v if isinstance(v, tuple) else (v,))]
    fa, fb = flat(a), flat(b)
    return len(fa) != len(fb) or any(x.shape != y.shape or not np.array_equal(x, y) for x, y in zip(fa, fb))


def invisible_mutations(rec):
    """the state-changing steps of a record that no query shows: behind each there must be, before the same container's next
    such step, a query of that container whose answer from the model differs — in shape or in an entry — from the answer on
    the model with that one step undone. A session in which stale device state could pass is a generator bug."""
    model, pending, hidden = SessionModel(rec), {}, []
    for i, st in enumerate(rec["steps"]):
        if st["op"] in MUTATIONS:
            if st["on"] in pending:
                hidden.append(pending[st["on"]][0])
            pending[st["on"]] = (i, model.m[st["on"]], model.version[st["on"]])
            model.apply(i)
        elif st["op"] == "query":
            for cid in {st["on"], st.get("other")} & set(pending):
                undone = model.snapshot()
                undone.m[cid], undone.version[cid] = pending[cid][1], pending[cid][2]
                if answers_differ(session_answer(model, i), session_answer(undone, i)):
                    del pending[cid]
    return sorted(hidden + [v[0] for v in pending.values()])


# ---- the runner
def _rc(lib, rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc}: {(lib.storm_hip_last_error() or lib.STORM_hip_error() or b'').decode()}")   # (not a value mismatch)


def _session_container(sb, ctx, model, cid):
    """a fresh container that holds the model's rows of `cid`"""
    c, D = model.rec["containers"][cid], model.m[cid]
    if c["type"] == "hip":
        return ctx.matrix_from_host(pack_bits(D))
    if c["type"] == "dosage":
        d = sb.StormDosage(c["S"])
        if D.shape[0]:
            from tests.test_gpu_dosage import pack
            d.add_packed(pack(D))
        return d
    s = sb.StormContig(c["width"]) if c["type"] == "contig" else sb.Storm()
    for row in D:
        s.add(storm_positions(row) if c["type"] == "storm" else np.flatnonzero(row).astype(np.uint32))
    return s


def _session_mutate(sb, ctx, live, model, i):
    """step i on the library; the model still holds the state before it"""
    import torch
    rec = model.rec
    st = rec["steps"][i]
    op, cid = st["op"], st["on"]
    c, x = rec["containers"][cid], live[cid]
    if op == "add":
        rows = session_rows(rec, i)
        if c["type"] == "dosage":
            from tests.test_gpu_dosage import pack
            if i % 2:
                x.add_packed(pack(rows))
            else:
                for row in rows:
                    x.add(row)
        else:
            for row in rows:
                got = x.add(storm_positions(row) if c["type"] == "storm" else np.flatnonzero(row).astype(np.uint32))
                assert c["type"] == "storm" or got == int(row.sum()), ("add", cid, got)
    elif op == "clear":
        x.clear()
    elif op == "hip_invalidate":
        x.hip_invalidate()
    elif op == "free_new":
        _close(x)
        live[cid] = ctx.matrix(st["n"], c["words"]) if c["type"] == "hip" else \
            sb.StormDosage(c["S"]) if c["type"] == "dosage" else sb.StormContig(c["width"]) if c["type"] == "contig" else sb.Storm()
    elif op == "resize":
        x.resize(st["n"])
    elif op == "upload":
        x.upload(pack_bits(session_rows(rec, i)), row0=st["row0"])
    elif op == "set_rows_from_positions":
        x.set_rows_from_positions([np.flatnonzero(r).astype(np.uint32) for r in session_rows(rec, i)], row0=st["row0"])
    elif op == "import_device":
        words = pack_bits(session_rows(rec, i))
        t = torch.from_numpy(np.ascontiguousarray(np.pad(words, ((0, 0), (0, 3)))).view(np.int64)).to("cuda:0")
        torch.cuda.synchronize()
        x.import_device(t.data_ptr(), st["rows"], words.shape[1] + 3, row0=st["row0"])
        ctx.synchronize()
    if op != "free_new":
        want = model.m[cid].shape[0] + (st["rows"] if op == "add" else 0)
        want = st["n"] if op == "resize" else 0 if op == "clear" and c["type"] != "hip" else want
        assert live[cid].n_rows == want, (op, cid, live[cid].n_rows, want)


def _bit_forms(call_host, call_device, rows, cols, pad, off, inside, what, written=None):
    """the host form as uint32 — zero outside `inside` — and the device form in a sentinel-filled window with a guard row and
    pitch columns: equal on `inside`, untouched outside `written` (default: `inside`)"""
    host = bits_of(call_host())
    assert host.shape == (rows, cols), (what, host.shape, (rows, cols))
    equal(host, np.zeros(host.shape, dtype=np.uint32), f"{what}: outside the layout (host form)", ~inside)
    if call_device is not None:
        flat, view = device_words(rows + 2, cols + pad, off)
        call_device(view.data_ptr(), rows + 2, cols + pad)
        dev = read_words(flat, view, inside if written is None else written, f"{what} (device form)")
        equal(dev, host, f"{what}: the device form against the host form", inside)
    return host


def session_ask(sb, ctx, live, model, i, stats):
    """query step i on the live containers, host and _device form, against session_answer"""
    import ctypes as C
    import torch
    st = model.rec["steps"][i]
    kind, on, other, pad, off = st["kind"], st["on"], st.get("other"), st["pad"], st["off"]
    ans = session_answer(model, i)
    x, y = live[on], live.get(other)
    lib = sb.load()
    n = model.m[on].shape[0]
    hip = model.type(on) == "hip"
    L = min(st["max_lag"], max(n - 1, 0))
    what = f"step {i}: {kind} on {on}" + (f" x {other}" if other else "")
    family = QUERY_KINDS[kind][0]
    if family.startswith("bit"):
        M = max(model.n_bits(on), model.n_bits(other or on))
        nbits = M if model.type(on) != "contig" else 0
        op, ms = st["bit_op"], st["measure"]
        if kind == "total":
            got = sum(x.pairw(r, st["world"]) for r in range(st["world"])) if hip else x.pairw_intersect_cardinality()
            equal(np.asarray(got), ans["total"], what)
            if hip:                                        # storm_hip_pairw_dense_launch: one device word per shard, a guard word on either side
                words = torch.full((st["world"] + 2,), -2, dtype=torch.int64, device="cuda:0")
                torch.cuda.synchronize()
                for r in range(st["world"]):
                    x.pairw_launch(words[1 + r].data_ptr(), r, st["world"])
                ctx.synchronize()
                got = words.cpu().numpy()
                assert got[0] == -2 and got[-1] == -2, f"{what}: the launch form wrote beside its word"
                equal(np.asarray(int(got[1:-1].sum())), ans["total"], f"{what} (launch form)")
            return
        if kind == "square_total":
            return equal(np.asarray(x.square(y) if hip else x.intersect_cardinality_square(y)), ans["total"], what)
        if kind == "band":
            want, where = ans["counts"], ans["where"]
            r0 = min(st["row0"], max(n - 1, 0))
            flat, view = device_words(want.shape[0] + 2, n + pad, off)
            x.pairw_matrix_band_device(view.data_ptr(), n + pad, r0, want.shape[0], op)
            ctx.synchronize()
            return equal(read_words(flat, view, np.ones(want.shape, dtype=bool), what), want, what, where)
        if kind in ("pairw_matrix", "square_matrix", "lag_matrix"):
            want, where = ans["counts"], ans["where"]
            if kind == "lag_matrix":
                host_call = lambda: x.pairw_lag_matrix(st["max_lag"], op)
                dev_call = (lambda p, r, ld: x.pairw_lag_matrix_device(p, ld, st["max_lag"], op)) if hip else \
                    (lambda p, r, ld: x.pairw_lag_matrix_device(p, r, ld, st["max_lag"], op))
            elif kind == "pairw_matrix":
                host_call = lambda: x.pairw_matrix(op)
                dev_call = (lambda p, r, ld: x.pairw_matrix_device(p, ld, op)) if hip else (lambda p, r, ld: x.pairw_matrix_device(p, r, ld, op))
            else:
                host_call = lambda: x.square_matrix(y, op)
                dev_call = None if hip else (lambda p, r, ld: x.square_matrix_device(y, p, r, ld, op))
            whole = np.ones(want.shape, dtype=bool) if hip and kind == "pairw_matrix" else None   # (storm_hip.h: i >= j as the kernel left them)
            host = _bit_forms(host_call, dev_call, want.shape[0], want.shape[1], pad, off, where, what, whole)
            return equal(host, want, what, where)
        if kind in ("pairw_similarity", "square_similarity", "lag_similarity"):
            v, nan, where = ans["value"]
            code = MEASURES.index(ms)
            if kind == "lag_similarity":
                host_call = lambda: x.pairw_lag_similarity(st["max_lag"], ms, n_bits=M if hip else nbits)
                dev_call = (lambda p, r, ld: x.pairw_lag_similarity_device(p, ld, st["max_lag"], ms, M)) if hip else \
                    (lambda p, r, ld: x.pairw_lag_similarity_device(p, r, ld, st["max_lag"], ms, n_bits=nbits))
            elif kind == "square_similarity":
                host_call = lambda: x.square_similarity(y, ms, n_bits=nbits)
                dev_call = lambda p, r, ld: x.square_similarity_device(y, p, r, ld, ms, n_bits=nbits)
            elif hip:
                def host_call():
                    out = np.zeros((n, n), dtype=np.float32)
                    _rc(lib, lib.storm_hip_pairw_similarity(ctx._h, x._h, code, M, out.ctypes.data_as(C.c_void_p), n), what)
                    return np.where(where, bits_of(out), 0).astype(np.uint32)      # (i >= j: as the count kernel left them)

                def dev_call(p, r, ld):
                    _rc(lib, lib.storm_hip_pairw_similarity_device(ctx._h, x._h, code, M, C.c_void_p(p), ld), what)
                    ctx.synchronize()
            else:
                host_call = lambda: x.pairw_similarity(ms, n_bits=nbits)
                dev_call = lambda p, r, ld: x.pairw_similarity_device(p, r, ld, ms, n_bits=nbits)
            whole = np.ones(v.shape, dtype=bool) if hip and kind == "pairw_similarity" else None
            host = _bit_forms(host_call, dev_call, v.shape[0], v.shape[1], pad, off, where, what, whole)
            return close_floats(stats, host, v, nan, where, what)
        k, score = st["k"], st["score"]                    # topk, square_topk
        cross = kind == "square_topk"
        v, nan, _ = ans["topk"]
        if cross:
            host = x.cross_topk(y, k, score, n_bits=M) if hip else x.square_topk(y, k, score, n_bits=M)
        else:
            host = x.pairw_topk(k, score, n_bits=M)
        flat_i, view_i = device_words(n + 1, k + pad)
        flat_v, view_v = device_words(n + 1, k + pad)
        di, dv = view_i.data_ptr(), view_v.data_ptr()
        if cross and hip:
            _rc(lib, lib.storm_hip_cross_dense_topk_device(ctx._h, x._h, y._h, SCORES.index(score), M, k, 0, C.c_void_p(di), C.c_void_p(dv),
                                                           k + pad), what)
        elif cross:
            x.square_topk_device(y, di, dv, n + 1, k + pad, k, score, n_bits=M)
        elif hip:
            x.pairw_topk_device(di, dv, k + pad, k, score, n_bits=M)
        else:
            x.pairw_topk_device(di, dv, n + 1, k + pad, k, score, n_bits=M)
        if hip:
            ctx.synchronize()
        listed = np.ones((n, k), dtype=bool)
        dev = (read_words(flat_i, view_i, listed, f"{what}: idx (device form)"), read_words(flat_v, view_v, listed, f"{what}: val (device form)"))
        for (idx, val), name in ((host, "host"), (dev, "device")):
            check_topk(stats, idx, val, ans["counts"], v, nan, k, score, cross, f"{what} {score} k={k} ({name})")
        equal(dev[0], host[0], f"{what}: the device form's idx against the host form's")
        return equal(dev[1], bits_of(host[1]), f"{what}: the device form's val against the host form's")
    # ---- dosage containers
    if kind == "row_sums":
        s, q = x.row_sums()
        equal(s, ans["sum"], f"{what}: sum")
        return equal(q, ans["sum_sq"], f"{what}: sum of squares")
    if kind == "row_missing":
        return equal(x.row_missing(), ans["missing"], what)
    corr, lag, S = st["corr"], st["max_lag"], model.samples(on)

    def hip_forms(host, device):
        def call(t):
            if t is None:
                return host()
            device(t.data_ptr(), int(t.stride(0)))
            ctx.synchronize()
        return call
    hip_calls = {"lag_dot": hip_forms(lambda: x.pairw_lag_dosage_matrix(lag), lambda p, ld: x.pairw_lag_dosage_matrix_device(p, ld, lag)),
                 "lag_nobs": hip_forms(lambda: x.pairw_lag_dosage_nobs(lag, S), lambda p, ld: x.pairw_lag_dosage_nobs_device(p, ld, lag, S)),
                 "lag_corr": hip_forms(lambda: x.pairw_lag_dosage_corr(lag, S, corr),
                                       lambda p, ld: x.pairw_lag_dosage_corr_device(p, ld, lag, S, corr)),
                 "lag_corr_complete": hip_forms(lambda: x.pairw_lag_dosage_corr_complete(lag, S, corr),
                                                lambda p, ld: x.pairw_lag_dosage_corr_complete_device(p, ld, lag, S, corr))}
    calls = hip_calls if hip else {"pairw_dot": lambda t: x.pairw_dot(device=t), "pairw_nobs": lambda t: x.pairw_nobs(device=t),
             "square_dot": lambda t: x.square_dot(y, device=t), "square_nobs": lambda t: x.square_nobs(y, device=t),
             "lag_dot": lambda t: x.pairw_lag_dot(lag, device=t), "lag_nobs": lambda t: x.pairw_lag_nobs(lag, device=t),
             "pairw_corr": lambda t: x.pairw_corr(corr, device=t), "pairw_corr_complete": lambda t: x.pairw_corr_complete(corr, device=t),
             "square_corr": lambda t: x.square_corr(y, corr, complete=st["complete"], device=t),
             "lag_corr": lambda t: x.pairw_lag_corr(lag, corr, device=t),
             "lag_corr_complete": lambda t: x.pairw_lag_corr_complete(lag, corr, device=t)}
    if kind in calls:
        want, where = (ans["counts"], ans["where"]) if "counts" in ans else (ans["value"][0], ans["value"][2])
        host = _both_forms(calls[kind], want.shape[0], want.shape[1], pad, where, 0, what)
        if "counts" in ans:
            return equal(host, want, what, where)
        return close_floats(stats, host, want, ans["value"][1], where, what)
    rows = n if n >= 2 else 0                              # storm.h: fewer than two rows: 0, nothing written
    if kind in ("lag_ldscore", "lag_ldscore_annot"):
        c = st["n_annot"] if kind == "lag_ldscore_annot" else None
        d_score, d_pairs = _vector_outputs(n, c, pad)
        if hip and c is None:
            score, pairs = x.lag_dosage_ldscore(lag, S, st["stat"], st["complete"])
            x.lag_dosage_ldscore_device(d_score.data_ptr(), d_pairs.data_ptr(), lag, S, st["stat"], st["complete"])
            ctx.synchronize()
        elif hip:
            score, pairs = x.lag_dosage_ldscore_annot(ans["annot"], lag, S, st["stat"], st["complete"])
            d_annot = torch.from_numpy(ans["annot"]).to("cuda:0")
            x.lag_dosage_ldscore_annot_device(d_annot.data_ptr(), int(d_annot.stride(0)), c, d_score.data_ptr(), int(d_score.stride(0)),
                                              d_pairs.data_ptr(), lag, S, st["stat"], st["complete"])
        elif c is None:
            score, pairs = x.lag_ldscore(lag, st["stat"], complete=st["complete"])
            assert x.lag_ldscore(lag, st["stat"], complete=st["complete"], device=(d_score, d_pairs)) is None
        else:
            score, pairs = x.lag_ldscore_annot(ans["annot"], lag, st["stat"], complete=st["complete"])
            d_annot = torch.from_numpy(ans["annot"]).to("cuda:0")
            assert x.lag_ldscore_annot(d_annot, lag, st["stat"], complete=st["complete"], device=(d_score, d_pairs)) is None
        equal(pairs, ans["pairs"], f"{what}: n_pairs")
        within_bound(stats, score, ans["score"], ans["bound"], what)
        dev, dev_pairs = d_score.cpu().numpy(), d_pairs.cpu().numpy().view(np.uint32)
        assert (dev[rows:] == np.float32(GUARD_F)).all() and (dev_pairs[rows:] == GUARD_I).all(), f"{what}: written behind row {rows}"
        if c is not None:
            assert (dev[:, c:] == np.float32(GUARD_F)).all(), f"{what}: written in the pitch columns"
            dev = dev[:, :c]
        equal(bits_of(dev[:rows]), bits_of(np.ascontiguousarray(score[:rows])), f"{what}: the device form's bits")
        return equal(dev_pairs[:rows], ans["pairs"][:rows], f"{what}: the device form's n_pairs")
    stats.min_margin = min(stats.min_margin, float(ans["margin"]))     # lag_prune
    assert float(ans["margin"]) >= PRUNE_MARGIN, f"{what}: an in-window r^2 lies {float(ans['margin']):.3g} (relative) from min_r2"
    min_r2, priority, complete = float(ans["min_r2"]), ans["priority"], st["complete"]
    order = None if priority is None else np.argsort(-priority, kind="stable")   # a HipMatrix is walked in a host permutation
    if hip:
        keep, owner = x.lag_dosage_prune(min_r2, lag, S, complete, owner=True, order=order)
    else:
        keep, owner = x.lag_prune(min_r2, lag, priority=priority, complete=complete, owner=True)
    equal(keep, ans["keep"], f"{what}: keep")
    equal(owner, ans["owner"], f"{what}: owner")
    d_keep = torch.full((n + GUARD,), GUARD_K, dtype=torch.uint8, device="cuda:0")
    d_owner = torch.full((n + GUARD,), GUARD_I, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    if hip:
        x.lag_dosage_prune_device(d_keep.data_ptr(), d_owner.data_ptr(), min_r2, lag, S, complete, order=order)
    else:
        assert x.lag_prune(min_r2, lag, priority=priority, complete=complete, device=(d_keep, d_owner)) is None
    dev_keep, dev_owner = d_keep.cpu().numpy(), d_owner.cpu().numpy().view(np.uint32)
    assert (dev_keep[n:] == GUARD_K).all() and (dev_owner[n:] == GUARD_I).all(), f"{what}: written behind row n"
    if n >= 2:
        equal(dev_keep[:n], ans["keep"], f"{what}: keep (device form)")
        equal(dev_owner[:n], ans["owner"], f"{what}: owner (device form)")


def _set_session_option(sb, ctx, kind, key, value):
    if kind == "hip":
        ctx.set_option(key, value)
    else:
        _rc(sb.load(), sb.load().STORM_hip_set_option(key.encode(), value), f"STORM_hip_set_option({key}, {value})")


def run_session(rec, ctx, stats, upto=None):
    """The steps of a record, 0 .. upto, on live containers. A storm session runs on the library's own context; a hip session
    on a HipContext of its own, made and closed here (`ctx` is not used), so that its cache history is the record's.

    A value mismatch (AssertionError from equal / close_floats / within_bound with return code 0) is looked at a second
    time: fresh containers are built from the model's current state, the one query is repeated on them, and the message
    says whether "a fresh container agrees: the session's state is at fault" or "a fresh container differs too". A return
    code other than 0 or a HIP error is re-raised as it is, and nothing more is started on the GPU: the options are NOT put
    back then (a storm session leaves the library's own context under whatever it set last, so what runs behind it in the
    same process runs under those options), and the live containers are left to their finalizers."""
    import stormbitmaps_amd as sb
    kind, steps = rec["kind"], rec["steps"]
    model = SessionModel(rec)
    own = sb.HipContext(0) if kind == "hip" else None
    ctx = own if own is not None else ctx
    live, failed = {}, False
    try:
        for cid, c in rec["containers"].items():
            live[cid] = ctx.matrix(c["n"], c["words"]) if kind == "hip" else _session_container(sb, ctx, model, cid)
        for i, st in enumerate(steps[:len(steps) if upto is None else upto + 1]):
            try:
                if st["op"] == "set_option":
                    _set_session_option(sb, ctx, kind, st["key"], st["value"])
                elif st["op"] == "query":
                    session_ask(sb, ctx, live, model, i, stats)
                else:
                    _session_mutate(sb, ctx, live, model, i)
                    model.apply(i)
            except AssertionError as e:
                verdict = "no second look: the failing step is not a query"
                if st["op"] == "query":
                    fresh = {}
                    try:
                        for cid in (st["on"], st.get("other")):
                            if cid is not None:
                                fresh[cid] = _session_container(sb, ctx, model, cid)
                        session_ask(sb, ctx, fresh, model, i, Stats())
                        verdict = "a fresh container agrees: the session's state is at fault"
                    except AssertionError:
                        verdict = "a fresh container differs too"
                    except Exception:
                        failed = True
                        raise
                    finally:
                        for x in fresh.values():
                            _close(x)
                trail = "\n".join(f"  {j}: {json.dumps(s, sort_keys=True)}" for j, s in enumerate(steps[:i + 1]))
                raise AssertionError(f"{e}\n{verdict}\nsteps 0 .. {i}:\n{trail}\nreplay: python -m tests._sweep --family {SESSION} "
                                     f"--seed {rec.get('seed')} --case {rec.get('index')} --upto {i}") from e
            except Exception:
                failed = True                              # a return code or a HIP error: nothing more on the GPU
                raise
    finally:
        if not failed:
            for key in {o[0] for o in rec["options"]}:
                _set_session_option(sb, ctx, kind, key, SESSION_DEFAULTS[key])
            for x in live.values():
                _close(x)
            if own is not None:
                own.close()


_RUN = {"bits": run_bits, "topk": run_topk, "dosage": run_dosage, "dosage_lag": run_dosage_lag, "ldscore": run_ldscore,
        "prune": run_prune, SESSION: run_session}


def run_case(family, rec, ctx, upto=None):
    """one case on the GPU; AssertionError names (family, seed, index) and the record. upto: a session's steps 0 .. upto"""
    stats = Stats()
    try:
        if family == SESSION:
            run_session(rec, ctx, stats, upto)
        else:
            _RUN[family](rec, ctx, stats)
    except Exception as e:
        if family != SESSION:
            raise AssertionError(f"sweep case (family={family!r}, seed={rec.get('seed')}, index={rec.get('index')}) failed: "
                                 f"{type(e).__name__}: {e}\nrecord: {json.dumps(rec, sort_keys=True)}\n"
                                 f"replay: python -m tests._sweep --family {family} --seed {rec.get('seed')} --case {rec.get('index')}") from e
        if not isinstance(e, AssertionError):
            raise                                          # a return code or a HIP error: as it is
        raise AssertionError(f"sweep case (family={family!r}, seed={rec.get('seed')}, index={rec.get('index')}, kind={rec['kind']!r}) "
                             f"failed: {e}") from e          # (run_session added the steps and the replay command)
    stats.cases = 1
    return stats


def run_family(family, seed, count, ctx):
    total = Stats()
    for rec in cases(family, seed, count):
        total.merge(run_case(family, rec, ctx))
    return total


def main(argv=None):
    ap = argparse.ArgumentParser(description="replay one case of the parity sweep on the GPU")
    ap.add_argument("--family", required=True, choices=FAMILIES + (SESSION,))
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--case", type=int, required=True)
    ap.add_argument("--upto", type=int, default=None, help="session: steps 0 .. UPTO only")
    args = ap.parse_args(argv)
    import stormbitmaps_amd as sb
    rec = list(cases(args.family, args.seed, args.case + 1))[args.case]
    print("record:", json.dumps({k: v for k, v in rec.items() if k != "steps"} if args.family == SESSION else rec, sort_keys=True))
    ctx = sb.HipContext(0)
    try:
        stats = run_case(args.family, rec, ctx, args.upto)
    except AssertionError as e:
        print(e)
        return 1
    finally:
        ctx.close()
    print("ok:", json.dumps(stats.as_dict()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
