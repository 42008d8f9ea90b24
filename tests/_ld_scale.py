"""The references of tests/test_gpu_ld_scale.py: the lag-band calls at the row counts and lags README.md quotes them at, where
an n x n numpy matrix no longer fits. The checker, never the thing under test: nothing here imports the library, and no
reference reads anything the library computed. tests/test_ld_scale_refs.py checks every reference here against the n x n ones
of tests/_sweep.py, the plain greedy of tests/_prune.py and tests/_ldscore.py's band_sums at shapes where those run.

    lag_products(A, B, L)           sum_s A[i, s] B[i + 1 + d, s] as [n, L] int64, by blocks of 512 rows through
                                    _sweep.matmul_exact; the dosage sums, the bit counts and, with _sweep's own lines on those
                                    exact integers, the r / r^2 and similarity references in the lag layout come from it
    formula_band / formula_sums     a band whose entry is a closed formula of its two rows (multiples of 2^-10), and its
                                    per-row sums from the formula alone: exact in double, so the device's float must have
                                    the reference's bits
    clique_* / strided_*            prune graphs whose greedy answer has a closed form under the orders the tests use
    random_edges, neighbours_of     a sparse random graph as an edge list, and the neighbour lists _prune.greedy takes
"""
import numpy as np

from tests import _sweep

BLOCK = 512                                                                        # rows of A per matmul_exact call


# ------------------------------------------------------------------------------------------ products in the lag layout
def lag_products(A, B, L, r0=0, r1=None):
    """[r1 - r0, L] int64: out[i - r0, d] = sum_s A[i, s] * B[i + 1 + d, s] for the rows r0 <= i < r1 (all by default), 0 where
    i + 1 + d >= n. A, B: [n, W] small non-negative integers. 512 rows of A at a time against the 512 + L rows of B behind
    the first of them; entry (i, d) is then on diagonal d of that block's product."""
    A, B = np.asarray(A), np.asarray(B)
    n = A.shape[0]
    r1 = n if r1 is None else r1
    out = np.zeros((max(r1 - r0, 0), L), dtype=np.int64)
    if L == 0:
        return out
    d = np.arange(L)[None, :]
    for b0 in range(r0, r1, BLOCK):
        b1 = min(b0 + BLOCK, r1)
        behind = B[b0 + 1:min(b1 + L, n)]                                          # rows b0 + 1 .. b1 - 1 + L, as far as there are rows
        if behind.shape[0] == 0:
            break
        P = _sweep.matmul_exact(A[b0:b1], behind)                                  # P[ii, c] = row b0 + ii with row b0 + 1 + c
        col = np.arange(b1 - b0)[:, None] + d                                      # j = i + 1 + d is column ii + d
        ok = col < behind.shape[0]
        out[b0 - r0:b1 - r0] = np.where(ok, np.take_along_axis(P, np.minimum(col, behind.shape[0] - 1), axis=1), 0)
    return out


def inside(n, L, r0=0, r1=None):
    """[r1 - r0, L] bool: the pair (i, i + 1 + d) exists"""
    r1 = n if r1 is None else r1
    return (np.arange(r0, r1)[:, None] + 1 + np.arange(L)[None, :]) < n


def _pair_rows(n, L, r0, r1):
    """(i [rows, 1], j [rows, L] clipped to n - 1) of the layout's entries"""
    i = np.arange(r0, r1)[:, None]
    return i, np.minimum(i + 1 + np.arange(L)[None, :], n - 1)


def dosage_lag_sums(G, L, r0=0, r1=None):
    """_sweep.dosage_sums in the lag layout: the same (A, B) choices, every pair sum [r1 - r0, L] int64 (0 in the corner), the
    per-row sums s, q and miss over ALL n rows"""
    G = np.asarray(G)
    r1 = G.shape[0] if r1 is None else r1
    g = G.astype(np.int64)
    z, m = np.where(G == 3, 0, G), (G != 3).astype(np.uint8)
    lp = lambda A, B: lag_products(A, B, L, r0, r1)
    return {"P": lp(G, G), "s": g.sum(axis=1), "q": (g * g).sum(axis=1), "miss": (G == 3).sum(axis=1, dtype=np.int64),
            "N": lp(m, m), "Pc": lp(z, z), "sx": lp(z, m), "sy": lp(m, z), "qx": lp(z * z, m), "qy": lp(m, z * z)}


def corr_plain_lag(sums, samples, measure, L, r0=0, r1=None):
    """(float64 value, undefined) [r1 - r0, L] of pairw_lag_corr — _sweep.corr_plain64's numerator and denominators through
    _sweep._corr64; 0 / False in the corner"""
    n, S = len(sums["s"]), int(samples)
    r1 = n if r1 is None else r1
    i, j = _pair_rows(n, L, r0, r1)
    s, dd = sums["s"], S * sums["q"] - sums["s"] ** 2
    num = S * sums["P"] - s[i] * s[j]
    v, nan = _sweep._corr64(num, np.broadcast_to(dd[i], num.shape), dd[j], measure)
    ok = inside(n, L, r0, r1)
    return np.where(ok, v, 0.0), nan & ok


def corr_complete_lag(sums, measure, L, r0=0, r1=None):
    """(float64 value, undefined) [r1 - r0, L] of pairw_lag_corr_complete — _sweep.corr_complete64's lines; 0 / False in the
    corner"""
    n = len(sums["s"])
    N = sums["N"]
    num = N * sums["Pc"] - sums["sx"] * sums["sy"]
    v, nan = _sweep._corr64(num, N * sums["qx"] - sums["sx"] ** 2, N * sums["qy"] - sums["sy"] ** 2, measure)
    ok = inside(n, L, r0, n if r1 is None else r1)
    return np.where(ok, v, 0.0), nan & ok


def bit_lag_counts(D, L, r0=0, r1=None):
    """(c [r1 - r0, L], a [n]) int64 of 0 / 1 rows D: |row_i & row_{i+1+d}| and the rows' own counts"""
    D = np.asarray(D)
    return lag_products(D, D, L, r0, r1), D.sum(axis=1, dtype=np.int64)


def bit_lag_ops(c, a, L, r0=0, r1=None):
    """and / or / xor counts in the lag layout, 0 in the corner"""
    n = len(a)
    r1 = n if r1 is None else r1
    i, j = _pair_rows(n, L, r0, r1)
    ok = inside(n, L, r0, r1)
    s = a[i] + a[j]
    return {"and": c, "or": np.where(ok, s - c, 0), "xor": np.where(ok, s - 2 * c, 0)}


def similarity_lag(measure, c, a, M, L, r0=0, r1=None):
    """(float64 value, undefined) [r1 - r0, L] of pairw_lag_similarity: _sweep.similarity64's formulas on the exact integers, entry
    by entry; 0 / False in the corner"""
    n, M = len(a), int(M)
    r1 = n if r1 is None else r1
    i, j = _pair_rows(n, L, r0, r1)
    c = np.asarray(c, dtype=np.int64)
    A, B = np.broadcast_to(a[i], c.shape), a[j]
    with np.errstate(divide="ignore", invalid="ignore"):
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
            dd = np.abs(num).astype(np.float64)
            if measure == "ld_d":
                nan = np.zeros(c.shape, dtype=bool)
                v = np.where(num < 0, -1.0, 1.0) * (dd / (float(M) * float(M)))
            else:
                nan = (A == 0) | (A >= M) | (B == 0) | (B >= M)
                v = (dd * dd) / ((A * (M - A)).astype(np.float64) * (B * (M - B)).astype(np.float64))
    ok = inside(n, L, r0, r1)
    return np.where(nan | ~ok, 0.0, v), nan & ok


# ------------------------------------------------------------------------------------------ the formula band
FORMULA_CHUNK = 16384                                                              # rows per step: [16384, L] int64 temporaries


def _formula_hash(rows):
    return (rows * 2654435761) % 1024                                              # int64: rows < 2^20, the product < 2^52


def formula_band(n, L, ld, device, poison):
    """[n, ld] float32 torch tensor on `device`: entry (i, d), the pair (i, j = i + 1 + d), is ((h[i] + 3 h[j]) mod 1024) / 1024
    with h[r] = (r * 2654435761) mod 2^10; the corner and the pitch columns hold `poison`"""
    import torch
    band = torch.full((n, ld), float(poison), dtype=torch.float32, device=device)
    d = torch.arange(L, dtype=torch.int64, device=device)[None, :]
    for r0 in range(0, n, FORMULA_CHUNK):
        i = torch.arange(r0, min(r0 + FORMULA_CHUNK, n), dtype=torch.int64, device=device)[:, None]
        j = i + 1 + d
        v = ((_formula_hash(i) + 3 * _formula_hash(j)) % 1024).to(torch.float32) / 1024.0
        band[r0:r0 + i.shape[0], :L] = torch.where(j < n, v, torch.full_like(v, float(poison)))
    return band


def formula_sums(n, L, device):
    """(score float64 [n], n_pairs int64 [n]) numpy: per row the sum of the formula over the pairs ahead of it (i, i + d) and
    behind it (i - d, i), 1 <= d <= L, from the formula alone. Every term is a multiple of 2^-10 in [0, 1): the sum of their
    numerators is an int64, and one division by 1024 is exact."""
    import torch
    score, pairs = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.int64)
    d = torch.arange(1, L + 1, dtype=torch.int64, device=device)[None, :]
    for r0 in range(0, n, FORMULA_CHUNK):
        i = torch.arange(r0, min(r0 + FORMULA_CHUNK, n), dtype=torch.int64, device=device)[:, None]
        ahead, behind = i + d, i - d
        t = torch.where(ahead < n, (_formula_hash(i) + 3 * _formula_hash(ahead)) % 1024, torch.zeros_like(ahead))
        t = t + torch.where(behind >= 0, (_formula_hash(behind) + 3 * _formula_hash(i)) % 1024, torch.zeros_like(behind))
        m = (ahead < n).sum(dim=1) + (behind >= 0).sum(dim=1)
        score[r0:r0 + i.shape[0]] = t.sum(dim=1).to(torch.float64).cpu().numpy() / 1024.0
        pairs[r0:r0 + i.shape[0]] = m.cpu().numpy()
    return score, pairs


# ------------------------------------------------------------------------------------------ many annotation columns from few
ANNOT_BASE = 3


def scaled_annotations(n, n_cols, seed):
    """(annot [n, n_cols] float32, base [n, 3] float32, scale [n_cols]): column c is base column c mod 3 — normal floats, normal floats with a
    tenth of them exact zeros, 0 / 1 — times scale[c] = +-2^k, k = c // 3 - 8 with alternating sign: exact in float, so no two
    columns are equal and every column's sums are a base column's times a power of two"""
    rng = np.random.default_rng(seed)
    base = rng.normal(size=(n, ANNOT_BASE)).astype(np.float32)
    base[rng.random(n) < 0.1, 1] = 0.0
    base[:, 2] = rng.integers(0, 2, size=n)
    c = np.arange(n_cols)
    scale = np.where(c % 2 == 0, 1.0, -1.0) * 2.0 ** (c // ANNOT_BASE - 8)
    annot = base[:, c % ANNOT_BASE] * scale[None, :].astype(np.float32)
    return annot.astype(np.float32), base, scale


def scaled_annot_sums(base_result, scale):
    """_ldscore_annot.annot_sums' (ref, sum_abs, m, a_max) of the columns of scaled_annotations from its result over the three
    base columns. A product by +-2^k is exact in double and in float, and nothing here is near
    overflow or underflow: every double product of a scaled column is the base column's times the scale, math.fsum of them
    is the exactly rounded sum times the scale, and so are the magnitudes — what annot_sums itself returns for the
    scaled columns, at a twentieth of its Python loops (tests/test_ld_scale_refs.py compares the two)."""
    ref, sum_abs, m, a_max = base_result
    pick = np.arange(len(scale)) % ANNOT_BASE
    mag = np.abs(scale)[None, :]
    return ref[:, pick] * scale[None, :], sum_abs[:, pick] * mag, m, a_max[:, pick] * mag


# ------------------------------------------------------------------------------------------ prune graphs with a closed form
def descending(n):
    """the priorities under which the rows are walked from the last to the first"""
    return np.arange(n, dtype=np.float32)


def clique_runs(n, L, seed):
    """the first rows of consecutive runs of random length 1 .. min(L + 1, 24) that cut [0, n): every pair inside a run lies
    within the lag"""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(1, min(L + 1, 24) + 1, size=n)
    starts = np.concatenate([[0], np.cumsum(lengths)])
    return starts[starts < n].astype(np.int64)


def clique_ahead(n, starts):
    """[n] int64: how many rows of its own run lie ahead of row i — its edges are the lags d < ahead[i]"""
    ends = np.concatenate([starts[1:], [n]])
    return np.repeat(ends, ends - starts) - 1 - np.arange(n)


def clique_reference(n, starts, order=None):
    """(keep uint8, owner uint32): under any order the greedy keeps of every run the row that comes first in the order, and
    that row owns the run"""
    order = np.arange(n) if order is None else np.asarray(order, dtype=np.int64)
    rank = np.empty(n, dtype=np.int64)
    rank[order] = np.arange(n)
    head = order[np.minimum.reduceat(rank, starts)]                                # per run: the row of the smallest rank
    ends = np.concatenate([starts[1:], [n]])
    owner = np.repeat(head, ends - starts)
    return (owner == np.arange(n)).astype(np.uint8), owner.astype(np.uint32)


def strided_reference(n, L, from_the_end=False):
    """(keep uint8, owner uint32) of the graph whose only edges are (i, i + L): paths of rows L apart, walked from their first
    row (row order) or their last (descending): every other row of a path is kept, and a removed row's kept neighbours are
    the rows L before and L behind it, of which the one that came first in the order owns it"""
    i = np.arange(n, dtype=np.int64)
    k = ((n - 1 - i) if from_the_end else i) // L
    keep = k % 2 == 0
    return keep.astype(np.uint8), np.where(keep, i, i + L if from_the_end else i - L).astype(np.uint32)


def random_edges(n, L, seed, per_row=3):
    """(i, d) int64, unique: about per_row edges at every row (per_row * n / 2 pairs drawn), and always the lags 0 and L - 1 at
    the first 64 rows and at the rows whose partner is one of the last 64"""
    rng = np.random.default_rng(seed)
    m = per_row * n // 2
    i = rng.integers(0, n - 1, size=m)
    d = rng.integers(0, L, size=m)
    first = np.arange(min(64, n - 1))
    last = np.arange(max(n - 65, 0), n - 1)                                        # partner i + 1 is one of the last 64 rows
    far = np.arange(max(n - L - 64, 0), n - L) if n > L else np.zeros(0, np.int64)  # partner i + L is
    i = np.concatenate([i, first, first, last, far])
    d = np.concatenate([d, np.zeros_like(first), np.full_like(first, L - 1), np.zeros_like(last), np.full_like(far, L - 1)])
    ok = i + 1 + d < n
    key = np.unique(i[ok] * L + d[ok])
    return key // L, key % L


def neighbours_of(n, i, j):
    """the neighbour lists _prune.greedy takes, from the edges (i[k], j[k])"""
    nb = [[] for _ in range(n)]
    for a, b in zip(np.asarray(i).tolist(), np.asarray(j).tolist()):
        nb[a].append(b)
        nb[b].append(a)
    return nb


def edges_above(values, nan, min_r2, n, L):
    """(i, j) of the entries of a reference in the lag layout that are defined and > min_r2"""
    i, d = np.nonzero(inside(n, L) & ~nan & (values > float(min_r2)))
    return i, i + 1 + d
