"""CPU tests of tests/_ld_scale.py, the references of tests/test_gpu_ld_scale.py: each of them against the reference the rest of
the suite already trusts, at shapes where that one runs — the lag-layout products, r / r^2 and similarity against the n x n
ones of tests/_sweep.py gathered by to_lag; the closed-form prune answers against the plain greedy of tests/_prune.py over
the same graph; the formula band's sums against tests/_ldscore.py's band_sums over the band's own floats. A checker that
drops the last lag, shifts a row or walks a path from the wrong end fails here."""
import numpy as np
import pytest

from tests import _ld_scale, _ldscore, _prune, _sweep

N_SET = (1, 2, 5, 130, 300, 700)


def lags_of(n):
    return sorted({1, 64, 129, n - 1, n + 5} - {0})


def small_rows(rng, n, width, top):
    return rng.integers(0, top + 1, size=(n, width)).astype(np.uint8)


@pytest.mark.parametrize("n", N_SET)
def test_lag_products_are_the_diagonals_of_the_full_product(n):
    rng = np.random.default_rng(n)
    A, B = small_rows(rng, n, 37, 3), small_rows(rng, n, 37, 9)
    full = _sweep.matmul_exact(A, B)
    for L in lags_of(n) + [0]:
        want = _sweep.to_lag(full, L)
        got = _ld_scale.lag_products(A, B, L)
        assert got.dtype == np.int64 and np.array_equal(got, want), (n, L)
        if n >= 130:                                                               # a row range is the rows of the whole
            for r0, r1 in ((0, 1), (3, 130), (n - 7, n), (100, 100)):
                assert np.array_equal(_ld_scale.lag_products(A, B, L, r0, r1), want[r0:r1]), (n, L, r0, r1)
    if n >= 2:                                                                     # not symmetric: A and B are not swapped
        assert not np.array_equal(_ld_scale.lag_products(A, B, n - 1), _ld_scale.lag_products(B, A, n - 1))


def test_lag_products_cross_the_row_blocks():
    """1100 rows, lag 600: three blocks of 512 rows, windows that reach over a whole block"""
    rng = np.random.default_rng(7)
    A = small_rows(rng, 1100, 20, 3)
    assert np.array_equal(_ld_scale.lag_products(A, A, 600), _sweep.to_lag(_sweep.matmul_exact(A, A), 600))


@pytest.mark.parametrize("missing", [0.0, 0.1])
@pytest.mark.parametrize("n", N_SET)
def test_dosage_references_in_the_lag_layout_are_the_n_by_n_ones(n, missing):
    S = 61
    G = _prune.ld_rows(n, S, 11 * n + 1, missing=missing)
    if n >= 5:
        G[n // 2] = 1                                                              # a constant row: every pair undefined
        if missing:
            G[n - 1] = 3
    full = _sweep.dosage_sums(G)
    for L in lags_of(n):
        sums = _ld_scale.dosage_lag_sums(G, L)
        for key in ("P", "N", "Pc", "sx", "sy", "qx", "qy"):
            assert np.array_equal(sums[key], _sweep.to_lag(full[key], L)), (n, L, key)
        for key, ref in (("s", "s_i"), ("q", "q_i"), ("miss", "miss")):
            assert np.array_equal(sums[key], full[ref]), (n, L, key)
        for measure in ("r", "r2"):
            for got, want in ((_ld_scale.corr_plain_lag(sums, S, measure, L), _sweep.corr_plain64(full, S, measure)),
                              (_ld_scale.corr_complete_lag(sums, measure, L), _sweep.corr_complete64(full, measure))):
                assert np.array_equal(got[0], _sweep.to_lag(want[0], L)), (n, L, measure)   # the same lines: the same doubles
                assert np.array_equal(got[1], _sweep.to_lag(want[1], L, False)), (n, L, measure)
        if n == 300:                                                               # a row range, as the large cases compare
            part = _ld_scale.dosage_lag_sums(G, L, 120, 260)
            for measure in ("r", "r2"):
                a, b = _ld_scale.corr_complete_lag(part, measure, L, 120, 260), _ld_scale.corr_complete_lag(sums, measure, L)
                assert np.array_equal(a[0], b[0][120:260]) and np.array_equal(a[1], b[1][120:260])
                a, b = _ld_scale.corr_plain_lag(part, S, measure, L, 120, 260), _ld_scale.corr_plain_lag(sums, S, measure, L)
                assert np.array_equal(a[0], b[0][120:260]) and np.array_equal(a[1], b[1][120:260])
    if n >= 130:
        undefined = _ld_scale.corr_plain_lag(_ld_scale.dosage_lag_sums(G, n - 1), S, "r2", n - 1)[1]
        assert undefined[n // 2, :n - 1 - n // 2].all() and not undefined.all() and (missing == 0 or (G == 3).any())


@pytest.mark.parametrize("n", N_SET)
def test_bit_references_in_the_lag_layout_are_the_n_by_n_ones(n):
    M = 100
    D = _sweep.random_bits_dense(np.random.default_rng(n + 3), n, M)
    if n >= 5:
        D[1], D[n - 2] = 0, 1                                                      # an empty and a full row
    c, a, _ = _sweep.bit_counts(D)
    ops = _sweep.bit_ops(c, a, a)
    for L in lags_of(n):
        cl, al = _ld_scale.bit_lag_counts(D, L)
        assert np.array_equal(al, a)
        got = _ld_scale.bit_lag_ops(cl, al, L)
        for op in _sweep.OPS:
            assert np.array_equal(got[op], _sweep.to_lag(ops[op], L)), (n, L, op)
        for measure in _sweep.MEASURES:
            v, nan = _ld_scale.similarity_lag(measure, cl, al, M, L)
            wv, wnan = _sweep.similarity64(measure, c, a, a, M)
            assert np.array_equal(v, _sweep.to_lag(wv, L)) and np.array_equal(nan, _sweep.to_lag(wnan, L, False)), (n, L, measure)


def orders_of(n, seed):
    return {"rows": None, "descending": _ld_scale.descending(n), "random": np.random.default_rng(seed).random(n, dtype=np.float32)}


@pytest.mark.parametrize("L", [1, 33, 70])
@pytest.mark.parametrize("n", [2, 65, 200, 1000])
def test_closed_form_prune_answers_are_the_greedys(n, L):
    lag = min(L, n - 1)
    starts = _ld_scale.clique_runs(n, lag, 5 * n + L)
    ahead = _ld_scale.clique_ahead(n, starts)
    assert starts[0] == 0 and (np.diff(starts) >= 1).all() and ahead.max() <= min(lag, 23) and (ahead >= 0).all()
    assert (ahead[np.concatenate([starts[1:], [n]]) - 1] == 0).all()               # a run's last row has nothing ahead
    i, d = np.nonzero(np.arange(lag)[None, :] < ahead[:, None])
    cliques = _ld_scale.neighbours_of(n, i, i + 1 + d)
    path = np.arange(max(n - lag, 0))
    paths = _ld_scale.neighbours_of(n, path, path + lag)
    for kind, priority in orders_of(n, n + L).items():
        order = _prune.walk_order(n, priority)
        want = _prune.greedy(cliques, n, priority)
        got = _ld_scale.clique_reference(n, starts, None if priority is None else order)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), ("cliques", n, L, kind)
        if kind != "random":
            want = _prune.greedy(paths, n, priority)
            got = _ld_scale.strided_reference(n, lag, kind == "descending")
            assert got[0].dtype == np.uint8 and got[1].dtype == np.uint32
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), ("paths", n, L, kind)
    if n >= 65 and lag > 1 and n % (2 * lag) not in (0, 1):                        # the two ends give different answers
        assert not np.array_equal(_ld_scale.strided_reference(n, lag)[0], _ld_scale.strided_reference(n, lag, True)[0])


@pytest.mark.parametrize("n,L", [(200, 33), (1000, 70), (300, 299)])
def test_random_edges_hold_the_lags_and_rows_they_promise(n, L):
    i, d = _ld_scale.random_edges(n, L, n + L)
    pairs = set(zip(i.tolist(), d.tolist()))
    assert len(pairs) == len(i) and (i + 1 + d < n).all() and (d < L).all() and (d >= 0).all() and (i >= 0).all()
    for r in range(min(64, n - 1)):
        assert (r, 0) in pairs and ((r, L - 1) in pairs or r + L >= n)
    for j in range(n - 64, n):
        assert (j - 1, 0) in pairs and (j - L < 0 or (j - L, L - 1) in pairs)
    degree = np.bincount(np.concatenate([i, i + 1 + d]), minlength=n)
    assert 2.0 <= degree.mean() <= 3 + 2 * 256 / n                                 # 3 n / 2 drawn pairs and up to 256 placed ones
    nb = _ld_scale.neighbours_of(n, i, i + 1 + d)
    assert [len(x) for x in nb] == degree.tolist() and all(v in nb[j] for v in range(n) for j in nb[v])


@pytest.mark.parametrize("L", [70, 299])
def test_the_formula_bands_sums_are_band_sums_of_its_floats(L):
    n, ld, poison = 300, L + 34, -3.0e4
    band = _ld_scale.formula_band(n, L, ld, "cpu", poison).numpy()
    ok = np.zeros((n, ld), dtype=bool)
    ok[:, :L] = _sweep.lag_mask(n, L)
    assert (band[~ok] == np.float32(poison)).all()
    h = (np.arange(n, dtype=np.int64) * 2654435761) % 1024
    i, d = 17, 5
    assert band[i, d] == np.float32(((h[i] + 3 * h[i + 1 + d]) % 1024) / 1024.0)  # the pair (i, j): h[i] + 3 h[j], not the reverse
    inside = band[ok]
    assert (inside >= 0).all() and (inside < 1).all() and (inside * 1024 == np.round(inside * 1024)).all() and np.unique(inside).size > 500
    score, pairs = _ld_scale.formula_sums(n, L, "cpu")
    ref, _, m = _ldscore.band_sums(band, n, L, _ldscore.R2)
    assert np.array_equal(score, ref) and np.array_equal(pairs, m)                 # exact on both sides: the same doubles
    rows = np.arange(n)
    assert np.array_equal(pairs, np.minimum(L, rows) + np.minimum(L, n - 1 - rows))
    assert np.array_equal(score.astype(np.float32).astype(np.float64), score)      # a float holds every sum exactly


@pytest.mark.parametrize("stat", [_ldscore.R2, _ldscore.ADJ])
def test_scaled_annotation_columns_have_the_scaled_sums_of_their_base_column(stat):
    from tests import _ldscore_annot
    n, L, C = 130, 70, 65
    rng = np.random.default_rng(3)
    band = rng.random((n, L + 3), dtype=np.float32)
    band[rng.random(band.shape) < 0.02] = np.nan
    nobs = rng.choice(np.array([0, 2, 3, 4, 77, 5000]), size=(n, L))
    annot, base, scale = _ld_scale.scaled_annotations(n, C, 9)
    assert annot.dtype == np.float32 and np.unique(annot, axis=1).shape[1] == C    # no two columns are equal
    assert np.array_equal(annot.astype(np.float64), base[:, np.arange(C) % 3].astype(np.float64) * scale[None, :])
    lo, hi = _ldscore_annot.windows(np.cumsum(rng.integers(0, 4, size=n)).astype(np.float64), 40.0)
    for kw in ({}, {"lo": lo, "hi": hi}):
        want = _ldscore_annot.annot_sums(band, n, L, stat, annot, nobs=nobs, **kw)
        got = _ld_scale.scaled_annot_sums(_ldscore_annot.annot_sums(band, n, L, stat, base, nobs=nobs, **kw), scale)
        for a, b in zip(got, want):
            assert a.shape == b.shape and np.array_equal(a, b)
