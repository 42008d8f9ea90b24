"""The parity sweep of tests/test_gpu_sweep_ld.py without a device: that the cases its seeds and counts draw reach the edges
(so the sweep is not hollow), that tests/_sweep.py's float64-BLAS references agree with per-sample Python loops on exact
integers and fractions (so they do not share a mistake with the matrix products), and that they agree with the bits the
headers' own lines give on the same integers when a host compiler builds them (storm_similarity_math.h, storm_dosage_math.h,
storm_ldscore_math.h: the restatements of tests/test_similarity_math.py, test_dosage_math.py and test_ldscore_math.py)."""
import ctypes as C
import math
import os
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import _sweep
from tests.test_gpu_sweep_ld import COUNT, SEEDS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAGGED = ("bits", "dosage_lag", "ldscore", "prune")
DOSAGE = ("dosage", "dosage_lag", "ldscore", "prune")


def drawn(family):
    return [rec for seed in SEEDS for rec in _sweep.cases(family, seed, COUNT[family])]


# ------------------------------------------------------------------------------------------ the sweep is not hollow
def test_every_family_runs_at_least_24_cases_per_seed():
    assert set(COUNT) == set(_sweep.FAMILIES) and all(c >= 24 for c in COUNT.values()) and SEEDS == (1, 2, 3)


@pytest.mark.parametrize("family", _sweep.FAMILIES)
def test_cases_are_deterministic(family):
    a, b = drawn(family), drawn(family)
    assert a == b and len(a) == 3 * COUNT[family]
    assert [r["index"] for r in a[:COUNT[family]]] == list(range(COUNT[family]))
    assert list(_sweep.cases(family, 1, 5)) == a[:5]                               # a prefix does not depend on the count
    assert a[:COUNT[family]] != a[COUNT[family]:2 * COUNT[family]]                 # ... and the seed matters


@pytest.mark.parametrize("family", _sweep.FAMILIES)
def test_rows_on_both_sides_of_every_block_edge(family):
    ns = [r["n"] for r in drawn(family)]
    assert 1 in ns and 2 in ns, sorted(set(ns))
    for edge in (64, 128, 256):
        assert any(edge // 2 < n <= edge for n in ns) and any(edge < n <= 2 * edge for n in ns), (edge, sorted(set(ns)))
    assert all(1 <= n <= _sweep.N_MAX for n in ns) and all(1 <= r.get("nb", 1) <= _sweep.N_MAX for r in drawn(family))


@pytest.mark.parametrize("family", LAGGED)
def test_lags_at_one_clipped_and_above_128(family):
    recs = drawn(family)
    assert any(r["max_lag"] == 1 for r in recs)
    assert any(r["n"] >= 2 and r["max_lag"] > r["n"] - 1 for r in recs)            # clipped to n - 1
    assert any(min(r["max_lag"], r["n"] - 1) > 128 for r in recs)
    assert all(r["max_lag"] >= 1 for r in recs)


@pytest.mark.parametrize("family", DOSAGE)
def test_samples_missing_shares_and_special_rows(family):
    recs = drawn(family)
    S = [r["S"] for r in recs]
    assert 1 in S and any(s % 32 == 0 for s in S) and any(s % 32 for s in S if s > 32), sorted(set(S))
    assert all(1 <= s <= 3000 for s in S)
    assert any(r["missing"] == 0 for r in recs) and any(r["missing"] > 0 for r in recs)
    assert any(r["const_row"] >= 0 for r in recs) and any(r["allmiss_row"] >= 0 for r in recs)
    assert any(r["shared_row"] >= 0 for r in recs)
    for r in recs[:12]:                                                            # the rows are what the record says
        G = _sweep.dosage_matrix(r)
        assert G.shape == (r["n"], r["S"]) and G.max(initial=0) <= 3
        if r["missing"] == 0:
            assert not (G == 3).any()
        if r["const_row"] >= 0:
            assert (G[r["const_row"]] == r["const_value"]).all()
        if r["allmiss_row"] >= 0:
            assert (G[r["allmiss_row"]] == 3).all()
        if r["shared_row"] >= 0:
            a, b = G[r["shared_row"]], G[r["shared_row"] + 1]
            both = (a != 3) & (b != 3)
            assert np.unique(a[both]).size <= 1


def test_bit_containers_of_every_kind_and_an_empty_row():
    recs = drawn("bits")
    kinds = {r["container"] for r in recs}
    assert kinds == {"contig", "storm_list", "storm_bitmap", "storm_rect", "hip"}
    assert any(r["empty_row"] >= 0 for r in recs) and any(r["full_row"] >= 0 for r in recs)
    assert all(r["empty_row"] < 0 for r in recs if r["container"] == "contig")
    rect = [r for r in recs if r["container"] == "storm_rect"]
    assert all(r["M"] != r["Mb"] for r in rect) and any(r["n"] == 1 or r["nb"] == 1 for r in rect)
    assert {r["gen"] for r in recs} == {"positions", "random_bits"}
    widths = [r["M"] for r in recs]
    assert any(m % 64 for m in widths) and any(m % 64 == 0 for m in widths) and any(m > 65536 for m in widths)
    assert all(64 <= m <= 70000 for m in widths)
    r = next(r for r in recs if r["container"] == "storm_bitmap" and r["n"] <= 130)
    assert _sweep.bit_matrix(r, r["n"], r["M"])[:, :65536].sum(axis=1).max() >= 4096
    r = next(r for r in recs if r["container"] == "storm_list" and r["n"] <= 130)
    D = _sweep.bit_matrix(r, r["n"], r["M"])
    assert max(D[:, b:b + 65536].sum(axis=1).max() for b in range(0, r["M"], 65536)) < 4096
    r = next(r for r in recs if r["empty_row"] >= 0 and r["n"] <= 130)
    assert _sweep.bit_matrix(r, r["n"], r["M"])[r["empty_row"]].sum() == 0


def test_topk_reaches_k_128_short_rows_and_every_form():
    recs = drawn("topk")
    assert {r["form"] for r in recs} == {"contig", "storm", "hip", "hip_cross", "storm_square"}
    assert {r["score"] for r in recs} == set(_sweep.SCORES) and {r["panel_rows"] for r in recs} == {0, 256, 512}
    assert {r["k"] for r in recs} <= set(_sweep.K_SET) and any(r["k"] == 128 for r in recs)
    columns = [r.get("nb", r["n"] - 1) for r in recs]                              # candidates at most: the other rows
    assert any(r["k"] > c for r, c in zip(recs, columns)) and any(r["k"] < c for r, c in zip(recs, columns))
    assert any(r["half_empty"] and r["score"] in ("cosine", "ld_r2") and r["n"] >= 4 for r in recs)   # half the rows: no candidate at all
    assert any(r.get("nb") == 1 for r in recs)


def test_dosage_rectangles_with_one_row_on_a_side():
    recs = drawn("dosage")
    assert any(r["nb"] == 1 for r in recs) and any(r["n"] == 1 for r in recs) and any(r["n"] > 256 and r["nb"] > 256 for r in recs)


@pytest.mark.parametrize("family", ["ldscore", "prune"])
def test_windows_from_positions(family):
    recs = [r for r in drawn(family) if r["use_pos"]]
    assert {r["lag_mode"] for r in recs} == {"auto", "exact", "more"}
    needs = []
    for r in recs:
        pos = _sweep.positions_of(r, r["n"])
        assert (np.diff(pos) >= 0).all() and (np.diff(pos) <= 4).all()
        needs.append(_sweep.window_need(r["n"], pos, r["max_dist"]))
    assert any((np.diff(_sweep.positions_of(r, r["n"])) == 0).any() for r in recs)   # equal positions
    assert any(n >= 2 for n in needs) and any(n > 64 for n in needs) and 0 in needs
    if family == "ldscore":
        counts = [r["n_annot"] for r in drawn(family)]
        assert any(c < 64 for c in counts) and any(c > 64 for c in counts) and 1 in counts and max(counts) <= 130
    else:
        assert any(not r["use_pos"] for r in drawn(family)) and {r["priority"] for r in drawn(family)} == {"none", "random", "ties"}
        assert {r["complete"] for r in drawn(family)} == {False, True}


# ------------------------------------------------------------------------------------------ references against loops
def tiny_bits(k):
    rec = {"gen": ("positions", "random_bits", "positions")[k], "draws": (3, 1, 20)[k], "input_seed": 50 + k,
           "empty_row": (0, -1, 2)[k], "full_row": (-1, 1, 4)[k]}
    return _sweep.bit_matrix(rec, (3, 6, 5)[k], (40, 17, 33)[k]), _sweep.bit_matrix(rec, (1, 4, 6)[k], (40, 17, 33)[k], salt=1)


def tiny_dosage(k):
    rec = {"n": (2, 5, 6)[k], "S": (1, 37, 40)[k], "missing": (0.0, 0.4, 0.1)[k], "input_seed": 60 + k,
           "shared_row": (-1, 0, 3)[k], "const_row": (-1, 3, 0)[k], "const_value": 2, "allmiss_row": (-1, 4, -1)[k]}
    return rec, _sweep.dosage_matrix(rec)


def frac_value(q, root=False, negative=False):
    v = math.sqrt(q) if root else float(q)
    return -v if negative else v


@pytest.mark.parametrize("k", range(3))
def test_bit_references_against_a_per_bit_loop(k):
    Da, Db = tiny_bits(k)
    for A, B in ((Da, Da), (Da, Db)):
        c, a, b = _sweep.bit_counts(A, None if B is A else B)
        M = A.shape[1]
        loop = [[sum(int(x) & int(y) for x, y in zip(ra, rb)) for rb in B] for ra in A]
        assert c.tolist() == loop and a.tolist() == [int(r.sum()) for r in A] and b.tolist() == [int(r.sum()) for r in B]
        ops = _sweep.bit_ops(c, a, b)
        assert ops["or"].tolist() == [[sum(int(x) | int(y) for x, y in zip(ra, rb)) for rb in B] for ra in A]
        assert ops["xor"].tolist() == [[sum(int(x) ^ int(y) for x, y in zip(ra, rb)) for rb in B] for ra in A]
        for measure in _sweep.MEASURES:
            v, nan = _sweep.similarity64(measure, c, a, b, M)
            for i in range(len(A)):
                for j in range(len(B)):
                    ci, ai, bj = loop[i][j], int(a[i]), int(b[j])
                    num = M * ci - ai * bj
                    if measure == "jaccard":
                        want = None if ai + bj - ci == 0 else float(Fraction(ci, ai + bj - ci))
                    elif measure == "cosine":
                        want = None if ai * bj == 0 else frac_value(Fraction(ci * ci, ai * bj), root=True)
                    elif measure == "ld_d":
                        want = float(Fraction(num, M * M))
                    else:
                        want = None if not (0 < ai < M and 0 < bj < M) else float(Fraction(num * num, ai * (M - ai) * bj * (M - bj)))
                    assert bool(nan[i, j]) == (want is None), (measure, i, j)
                    if want is not None:
                        assert v[i, j] == pytest.approx(want, rel=1e-13, abs=0), (measure, i, j)


def loop_sums(x, y):
    """the sums of two dosage rows, one sample at a time, in Python integers"""
    P = s_i = q_i = s_j = q_j = N = Pc = sx = sy = qx = qy = 0
    for a, b in zip((int(v) for v in x), (int(v) for v in y)):
        P, s_i, q_i, s_j, q_j = P + a * b, s_i + a, q_i + a * a, s_j + b, q_j + b * b
        if a != 3 and b != 3:
            N, Pc, sx, sy, qx, qy = N + 1, Pc + a * b, sx + a, sy + b, qx + a * a, qy + b * b
    return dict(P=P, s_i=s_i, q_i=q_i, s_j=s_j, q_j=q_j, N=N, Pc=Pc, sx=sx, sy=sy, qx=qx, qy=qy)


def loop_corr(t, S, complete, measure):
    """None (undefined) or the correlation from the loop's integers, through a Fraction"""
    if complete:
        num, d_i, d_j = t["N"] * t["Pc"] - t["sx"] * t["sy"], t["N"] * t["qx"] - t["sx"] ** 2, t["N"] * t["qy"] - t["sy"] ** 2
    else:
        num, d_i, d_j = S * t["P"] - t["s_i"] * t["s_j"], S * t["q_i"] - t["s_i"] ** 2, S * t["q_j"] - t["s_j"] ** 2
    if d_i == 0 or d_j == 0:
        return None
    q = Fraction(num * num, d_i * d_j)
    return float(q) if measure == "r2" else frac_value(q, root=True, negative=num < 0)


@pytest.mark.parametrize("k", range(3))
def test_dosage_references_against_a_per_sample_loop(k):
    rec, G = tiny_dosage(k)
    n, S = G.shape
    other = _sweep.dosage_matrix(dict(rec, missing=0.4), 3, salt=1)
    for Ga, Gb in ((G, G), (G, other)):
        sums = _sweep.dosage_sums(Ga, None if Gb is Ga else Gb)
        for i in range(len(Ga)):
            assert sums["miss"][i] == sum(int(v) == 3 for v in Ga[i])
            for j in range(len(Gb)):
                t = loop_sums(Ga[i], Gb[j])
                for key in ("P", "N", "Pc", "sx", "sy", "qx", "qy"):
                    assert sums[key][i, j] == t[key], (key, i, j)
                assert (sums["s_i"][i], sums["q_i"][i], sums["s_j"][j], sums["q_j"][j]) == (t["s_i"], t["q_i"], t["s_j"], t["q_j"])
                for measure in ("r", "r2"):
                    for complete, (v, nan) in ((False, _sweep.corr_plain64(sums, S, measure)), (True, _sweep.corr_complete64(sums, measure))):
                        want = loop_corr(t, S, complete, measure)
                        assert bool(nan[i, j]) == (want is None), (measure, complete, i, j)
                        if want is not None:
                            assert v[i, j] == pytest.approx(want, rel=1e-13, abs=0), (measure, complete, i, j)
                        if complete and t["N"] < 2:
                            assert nan[i, j]                                       # fewer than two shared samples: undefined


@pytest.mark.parametrize("k", range(3))
def test_lag_layout_ld_scores_and_pruning_against_loops(k):
    rec, G = tiny_dosage(k)
    n, S = G.shape
    pos = np.array([0.0, 0.0, 1.0, 4.0, 4.0, 9.0][:n])
    annot = np.random.default_rng(k).normal(size=(n, 3)).astype(np.float32)
    for complete in (False, True):
        r2, nan, N = _sweep._r2_of(G, S, complete)
        pair = [[loop_sums(G[i], G[j]) for j in range(n)] for i in range(n)]
        loop_r2 = [[loop_corr(pair[i][j], S, complete, "r2") for j in range(n)] for i in range(n)]
        for max_lag, use_pos, max_dist in ((1, False, None), (3, False, None), (100, False, None), (None, True, 1.0), (5, True, 4.0)):
            window = _sweep.ld_window(n, max_lag, pos if use_pos else None, max_dist)
            L = n - 1 if max_lag is None else min(max_lag, n - 1)
            for i in range(n):
                for j in range(n):
                    inside = i != j and abs(i - j) <= L and (not use_pos or abs(pos[i] - pos[j]) <= max_dist)
                    assert bool(window[i, j]) == inside
            if use_pos:
                from tests._prune import window_bounds
                assert _sweep.window_need(n, pos, max_dist) == window_bounds(pos, max_dist)[2]
            band = _sweep.to_lag(r2, L, fill=-1.0)                                 # entry (i, d) is the pair (i, i + 1 + d)
            for i in range(n):
                for d in range(L):
                    assert band[i, d] == (r2[i, i + 1 + d] if i + 1 + d < n else -1.0)
            for stat in ("r2", "r2_adj"):
                want, mag, pairs = _sweep.ldscore_reference(r2, nan, N, stat, window)
                want_a, mag_a, pairs_a = _sweep.ldscore_reference(r2, nan, N, stat, window, annot)
                assert np.array_equal(pairs, pairs_a)
                for i in range(n):
                    total, absolute, count, cols = Fraction(0), Fraction(0), 0, [Fraction(0)] * 3
                    for j in range(n):
                        Nij = pair[i][j]["N"] if complete else S
                        if not window[i, j] or loop_r2[i][j] is None or (stat == "r2_adj" and Nij < 3):
                            continue
                        r = Fraction(loop_r2[i][j])
                        t = r if stat == "r2" else r - (1 - r) / (Nij - 2)
                        total, absolute, count = total + t, absolute + abs(t), count + 1
                        cols = [c + t * Fraction(float(annot[j, col])) for col, c in enumerate(cols)]
                    assert pairs[i] == count
                    assert want[i] == pytest.approx(float(total), rel=1e-12, abs=1e-15) and mag[i] == pytest.approx(float(absolute), rel=1e-12)
                    for col in range(3):
                        assert want_a[i, col] == pytest.approx(float(cols[col]), rel=1e-9, abs=1e-13)
    # the threshold of the pruning cases: the midpoint of the widest gap, t itself without two values
    assert _sweep.prune_threshold([0.47, 0.48, 0.53, 0.9], 0.5) == np.float32(0.505)
    assert _sweep.prune_threshold([0.2, 0.9], 0.5) == np.float32(0.5) and _sweep.prune_threshold([0.3], 0.2) == np.float32(0.2)
    assert _sweep.prune_threshold([], 0.8) == np.float32(0.8)
    assert _sweep.prune_margin([0.5, 0.25], np.float32(0.25) * (1 + 2.0 ** -10)) == pytest.approx(2.0 ** -10, rel=1e-3)


def test_the_topk_properties_catch_a_wrong_list():
    v = np.array([[0.0, 0.5, 0.25, 0.75, 0.5], [0.5, 0.0, 0.1, 0.2, 0.3]])
    nan = np.zeros(v.shape, dtype=bool)
    nan[1, 4] = True
    f = lambda x: np.float32(x).view(np.uint32)
    good_i = np.array([[3, 1, 4], [0, 3, 2]], dtype=np.uint32)
    good_v = np.array([[f(0.75), f(0.5), f(0.5)], [f(0.5), f(0.2), f(0.1)]], dtype=np.uint32)
    stats = _sweep.Stats()
    _sweep.check_topk_floats(stats, good_i, good_v, v, nan.copy(), 3, True, "good")
    one_off = good_v.copy()
    one_off[0, 0] += 1                                                             # one ulp off is allowed
    _sweep.check_topk_floats(stats, good_i, one_off, v, nan.copy(), 3, True, "one ulp")
    assert stats.worst_ulp == 1
    for bad_i, bad_v in ((np.array([[3, 4, 1], [0, 3, 2]]), good_v),               # equal values by column descending
                         (np.array([[3, 1, 2], [0, 3, 2]]), np.array([[f(0.75), f(0.5), f(0.25)], good_v[1]])),   # a better one unlisted
                         (np.array([[3, 1, 1], [0, 3, 2]]), good_v),               # a column twice
                         (np.array([[3, 1, 4], [0, 3, 4]]), good_v),               # an undefined entry listed
                         (np.array([[0, 3, 1], [0, 3, 2]]), np.array([[f(0.0), f(0.75), f(0.5)], good_v[1]])),    # the row itself
                         (good_i, good_v + np.uint32(2))):                         # two ulps off
        with pytest.raises(AssertionError):
            _sweep.check_topk_floats(stats, np.asarray(bad_i, dtype=np.uint32), np.asarray(bad_v, dtype=np.uint32), v, nan.copy(), 3,
                                     True, "bad")
    short_i = np.array([[3, 1, 4, 2, _sweep.NO_INDEX], [0, 3, 2, _sweep.NO_INDEX, _sweep.NO_INDEX]], dtype=np.uint32)
    short_v = np.array([[f(0.75), f(0.5), f(0.5), f(0.25), _sweep.NAN_BITS], [f(0.5), f(0.2), f(0.1), _sweep.NAN_BITS, _sweep.NAN_BITS]],
                       dtype=np.uint32)
    _sweep.check_topk_floats(stats, short_i, short_v, v, nan.copy(), 5, True, "short")
    with pytest.raises(AssertionError):
        _sweep.check_topk_floats(stats, short_i[:, [0, 1, 2, 4]], short_v[:, [0, 1, 2, 4]], v, nan.copy(), 4, True,
                                 "padding where a candidate is left")


# ------------------------------------------------------------------------------------------ references against the headers
SOURCE = r"""
#include "storm_similarity_math.h"
#include "storm_dosage_math.h"
#include "storm_ldscore_math.h"
extern "C" void sim_bits(const uint32_t* c, const uint32_t* a, const uint32_t* b, uint64_t n, int measure, uint64_t M, uint32_t* out) {
    for (uint64_t i = 0; i < n; ++i) out[i] = storm::similarity_bits(c[i], a[i], b[i], measure, M);
}
extern "C" void corr_bits(const uint32_t* p, const uint32_t* si, const uint32_t* qi, const uint32_t* sj, const uint32_t* qj,
                          uint64_t n, int measure, uint64_t S, uint32_t* out) {
    for (uint64_t k = 0; k < n; ++k) out[k] = storm::dosage_corr_bits(p[k], si[k], qi[k], sj[k], qj[k], measure, S);
}
extern "C" void corr_complete_bits(const uint32_t* p, const uint32_t* N, const uint32_t* sx, const uint32_t* sy, const uint32_t* qx,
                                   const uint32_t* qy, uint64_t n, int measure, uint32_t* out) {
    for (uint64_t k = 0; k < n; ++k) out[k] = storm::dosage_corr_complete_bits(p[k], N[k], sx[k], sy[k], qx[k], qy[k], measure);
}
extern "C" void ld_terms(const float* rho, const uint32_t* N, uint64_t n, int stat, double* term, uint8_t* summed) {
    for (uint64_t k = 0; k < n; ++k) { term[k] = 0.0; summed[k] = storm::ldscore_term(rho[k], stat, N[k], &term[k]) ? 1 : 0; }
}
"""


@pytest.fixture(scope="module")
def headers(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "a host C++ compiler"
    d = tmp_path_factory.mktemp("sweepmath")
    src, so = d / "sweep.cpp", d / "libsweep.so"
    src.write_text(SOURCE)
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Werror",
                    "-I", os.path.join(ROOT, "stormbitmaps_amd", "csrc"), str(src), "-o", str(so), "-lm"], check=True)
    lib = C.CDLL(str(so))
    for f in (lib.sim_bits, lib.corr_bits, lib.corr_complete_bits, lib.ld_terms):
        f.restype = None
    return lib


def u32(x):
    return np.ascontiguousarray(np.asarray(x).ravel(), dtype=np.uint32)


def p(a):
    return C.c_void_p(a.ctypes.data)


def one_ulp(got_bits, v64, nan):
    got_bits = got_bits.reshape(v64.shape)
    assert np.array_equal(got_bits == _sweep.NAN_BITS, nan) and np.array_equal((got_bits & 0x7FFFFFFF) > 0x7F800000, nan)
    want = v64.astype(np.float32).view(np.uint32)
    return int(np.abs(_sweep.ordered(got_bits) - _sweep.ordered(want))[~nan].max(initial=0))


def header_bit_cases():
    for k in range(3):
        yield tiny_bits(k)
    rec = {"gen": "random_bits", "draws": 1, "input_seed": 5, "empty_row": 7, "full_row": 9}
    yield _sweep.bit_matrix(rec, 150, 1000), _sweep.bit_matrix(rec, 33, 1000, salt=1)
    rec = {"gen": "positions", "draws": 900, "input_seed": 6, "empty_row": -1, "full_row": 0}
    yield _sweep.bit_matrix(rec, 40, 70000), _sweep.bit_matrix(rec, 40, 70000, salt=1)


def test_similarity_reference_against_the_headers_lines(headers):
    worst = 0
    for Da, Db in header_bit_cases():
        c, a, b = _sweep.bit_counts(Da, Db)
        M = Da.shape[1]
        A, B = np.broadcast_to(a[:, None], c.shape), np.broadcast_to(b[None, :], c.shape)
        for code, measure in enumerate(_sweep.MEASURES):
            v, nan = _sweep.similarity64(measure, c, a, b, M)
            out = np.empty(c.size, dtype=np.uint32)
            cc, aa, bb = u32(c), u32(A), u32(B)
            headers.sim_bits(p(cc), p(aa), p(bb), C.c_uint64(c.size), code, C.c_uint64(M), p(out))
            worst = max(worst, one_ulp(out, v, nan))
    assert worst <= 1
    print(f"similarity64 against storm_similarity_math.h: worst {worst} ulp")


def header_dosage_cases():
    for k in range(3):
        yield tiny_dosage(k)[1]
    for seed, n, S, missing in ((1, 120, 257, 0.1), (2, 60, 1000, 0.4), (3, 90, 33, 0.0)):
        rec = {"n": n, "S": S, "missing": missing, "input_seed": seed, "shared_row": 5 if missing else -1, "const_row": 11,
               "const_value": 1, "allmiss_row": 20 if missing else -1}
        yield _sweep.dosage_matrix(rec)


def test_dosage_references_against_the_headers_lines(headers):
    worst = 0
    for G in header_dosage_cases():
        n, S = G.shape
        t = _sweep.dosage_sums(G)
        full = lambda x, axis: u32(np.broadcast_to(x[:, None] if axis == 0 else x[None, :], (n, n)))
        for code, measure in ((0, "r2"), (1, "r")):
            out = np.empty(n * n, dtype=np.uint32)
            args = [u32(t["P"]), full(t["s_i"], 0), full(t["q_i"], 0), full(t["s_j"], 1), full(t["q_j"], 1)]
            headers.corr_bits(*(p(x) for x in args), C.c_uint64(n * n), code, C.c_uint64(S), p(out))
            worst = max(worst, one_ulp(out, *_sweep.corr_plain64(t, S, measure)))
            args = [u32(t[key]) for key in ("Pc", "N", "sx", "sy", "qx", "qy")]
            headers.corr_complete_bits(*(p(x) for x in args), C.c_uint64(n * n), code, p(out))
            worst = max(worst, one_ulp(out, *_sweep.corr_complete64(t, measure)))
    assert worst <= 1
    print(f"corr_plain64 / corr_complete64 against storm_dosage_math.h: worst {worst} ulp")


def test_ld_score_terms_against_the_headers_lines(headers):
    """the header forms a term from the FLOAT r^2; the reference from the float64 one: the summed pairs must be the same and a
    term within what the float's half ulp (2^-24 r^2) becomes under the correction, (1 + 1 / (N - 2)) times that"""
    for G in header_dosage_cases():
        n, S = G.shape
        for complete in (False, True):
            r2, nan, N = _sweep._r2_of(G, S, complete)
            rho = np.where(nan, np.nan, r2).astype(np.float32).ravel()
            for code, stat in ((0, "r2"), (1, "r2_adj")):
                want, ok = _sweep.ldscore_terms(r2, nan, N, stat)
                term, summed = np.empty(n * n, dtype=np.float64), np.empty(n * n, dtype=np.uint8)
                NN = u32(N)
                headers.ld_terms(p(rho), p(NN), C.c_uint64(n * n), code, p(term), p(summed))
                assert np.array_equal(summed.reshape(n, n).astype(bool), ok), (stat, complete)
                scale = 1.0 + np.where(ok & (N >= 3), 1.0 / np.maximum(N - 2, 1), 0.0) * (stat == "r2_adj")
                err = np.abs(term.reshape(n, n) - want)[ok]
                assert (err <= (2.0 ** -24 * r2 * scale + 1e-15)[ok]).all(), (stat, complete, float(err.max()))


def test_the_float_rule_and_the_equality_report_catch_what_they_should():
    want = np.array([[0.25, 1.0 / 3.0, 0.0], [0.5, 0.0, -0.125]])
    nan = np.array([[False, False, True], [False, False, False]])
    where = np.array([[True, True, True], [True, False, True]])
    good = want.astype(np.float32).view(np.uint32).copy()
    good[0, 2] = _sweep.NAN_BITS
    good[1, 1] = 12345                                                             # outside `where`: not looked at
    stats = _sweep.Stats()
    _sweep.close_floats(stats, good, want, nan, where, "good")
    assert stats.worst_ulp == 0
    off = good.copy()
    off[0, 1] += 1
    off[1, 2] -= 1
    _sweep.close_floats(stats, off, want, nan, where, "one ulp")
    assert stats.worst_ulp == 1
    for r, c, bits in ((0, 1, good[0, 1] + 2), (0, 2, 0x7FC00001), (0, 2, 0), (0, 0, _sweep.NAN_BITS), (1, 2, good[1, 2] ^ 0x80000000)):
        bad = good.copy()
        bad[r, c] = bits
        with pytest.raises(AssertionError):
            _sweep.close_floats(_sweep.Stats(), bad, want, nan, where, "bad")
    with pytest.raises(AssertionError, match=r"first at \[\[1, 0\]\]: got \[7\], want \[5\]"):
        _sweep.equal(np.array([[1, 2], [7, 4]]), np.array([[1, 2], [5, 4]]), "x")
    _sweep.equal(np.array([[1, 2], [7, 4]]), np.array([[1, 2], [5, 4]]), "x", np.array([[True, True], [False, True]]))
    stats = _sweep.Stats()
    _sweep.within_bound(stats, np.float32([1.0, 2.0]), np.array([1.0, 2.0 + 2.0 ** -24]), np.array([0.0, 2.0 ** -22]), "b")
    assert stats.worst_ratio == 0.25
    with pytest.raises(AssertionError):
        _sweep.within_bound(stats, np.float32([1.0, 2.0]), np.array([1.0 + 2.0 ** -20, 2.0]), np.array([0.0, 1.0]), "b")
