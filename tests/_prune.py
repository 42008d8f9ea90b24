"""The reference of the prune / clump tests: the plain greedy — sort by (-priority, index), keep a row if it is not marked,
mark the kept row's neighbours — over the edges of a float band in the lag layout, in numpy. Also the one-round rule a wrong
implementation might compute instead, and the generator of rows with real LD the container tests and tools/bench_prune.py
share."""
import numpy as np


def mask_pitch(L):
    return 2 * ((L + 31) // 32) + 2


def neighbours(band, n, max_lag, min_r2, lo=None, hi=None):
    """nb[i] = the rows adjacent to row i: the pairs (i, j = i + 1 + d), d < L = min(max_lag, n - 1), j < n, with
    band[i, d] > min_r2 as float32 (a NaN is never an edge) and, with windows, j <= hi[i] and i >= lo[j]"""
    nb = [[] for _ in range(n)]
    if n < 2:
        return nb
    L = min(max_lag, n - 1)
    with np.errstate(invalid="ignore"):
        e = np.asarray(band, dtype=np.float32)[:n, :L] > np.float32(min_r2)
    for i, d in zip(*np.nonzero(e)):
        j = int(i) + 1 + int(d)
        if j < n and (lo is None or (j <= hi[i] and i >= lo[j])):
            nb[int(i)].append(j)
            nb[j].append(int(i))
    return nb


def walk_order(n, priority=None):
    """higher priority first, ties to the lower row"""
    if priority is None:
        return np.arange(n)
    return np.lexsort((np.arange(n), -np.asarray(priority, dtype=np.float32)))


def greedy(nb, n, priority=None):
    """(keep uint8, owner uint32): the lexicographically first maximal independent set and every row's clump"""
    keep, marked, owner = np.zeros(n, np.uint8), np.zeros(n, bool), np.arange(n, dtype=np.uint32)
    for v in walk_order(n, priority):
        if not marked[v]:
            keep[v] = 1
            for j in nb[v]:
                if not marked[j]:
                    marked[j], owner[j] = True, v
    return keep, owner


def one_round(nb, n, priority=None):
    """NOT the greedy: keep a row when no neighbour comes before it in the order"""
    rank = np.empty(n, np.int64)
    rank[walk_order(n, priority)] = np.arange(n)
    return np.array([all(rank[j] > rank[v] for j in nb[v]) for v in range(n)], dtype=np.uint8)


def window_bounds(pos, max_dist):
    """(lo, hi, lag) of storm_ldscore_window_plan for non-decreasing positions"""
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    lo, hi = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    for i in range(n):
        inside = [j for j in range(n) if (pos[i] - pos[j] if j < i else pos[j] - pos[i]) <= max_dist]
        lo[i], hi[i] = min(inside), max(inside)
    lag = int(max(max(np.arange(n) - lo), max(hi - np.arange(n)))) if n else 0
    return lo, hi, lag


def ld_rows(n, n_samples, seed, missing=0.0):
    """[n, n_samples] uint8 dosages 0 .. 2 in blocks of 1 to 24 rows; within a block every row is the PREVIOUS one with each
    sample redrawn with a probability of U(0.10, 0.35), so r^2 decays along the block and chains form. missing: the share of
    calls set to 3."""
    rng = np.random.default_rng(seed)
    rows = np.empty((n, n_samples), dtype=np.uint8)
    i = 0
    while i < n:
        size = int(rng.integers(1, 25))
        freq = rng.uniform(0.15, 0.5)
        cur = rng.binomial(2, freq, size=n_samples).astype(np.uint8)
        for _ in range(min(size, n - i)):
            rows[i] = cur
            i += 1
            redraw = rng.random(n_samples) < rng.uniform(0.10, 0.35)
            cur = np.where(redraw, rng.binomial(2, freq, size=n_samples), cur).astype(np.uint8)
    if missing:
        rows[rng.random(rows.shape) < missing] = 3
    return rows
