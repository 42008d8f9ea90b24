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


# ------------------------------------------------------------------------------------------ the session family
from tests import test_gpu_sweep_sessions as _sessions  # noqa: E402

NXN = ("pairw_matrix", "pairw_similarity", "pairw_dot", "pairw_corr", "pairw_nobs", "pairw_corr_complete")


def session_records(seed=None):
    return [rec for s in (_sessions.SEEDS if seed is None else (seed,)) for rec in _sweep.cases(_sweep.SESSION, s, _sessions.COUNT)]


def trace(rec):
    """per step: the step, the rows of every container before and behind it, the options in force, the model behind it"""
    model, opts, out = _sweep.SessionModel(rec), dict(_sweep.SESSION_DEFAULTS), []
    for i, st in enumerate(rec["steps"]):
        before = {cid: m.shape[0] for cid, m in model.m.items()}
        if st["op"] == "set_option":
            opts[st["key"]] = st["value"]
        model.apply(i)
        out.append({"i": i, "st": st, "before": before, "after": {cid: m.shape[0] for cid, m in model.m.items()}, "opts": dict(opts),
                    "model": model.snapshot()})
    return out


def is_query(t, cid=None, kinds=None):
    st = t["st"]
    return st["op"] == "query" and (cid is None or cid in (st["on"], st.get("other"))) and (kinds is None or st["kind"] in kinds)


def test_sessions_are_deterministic():
    a, b = session_records(), session_records()
    assert a == b and len(a) == 3 * _sessions.COUNT and _sessions.SEEDS == (1, 2, 3)
    assert [r["kind"] for r in a[:4]] == ["storm", "hip", "storm", "hip"]
    assert list(_sweep.cases(_sweep.SESSION, 1, 3)) == a[:3]                       # a prefix does not depend on the count
    assert a[0]["steps"] != a[_sessions.COUNT]["steps"]                            # ... and the seed matters
    for rec in a[:4]:                                                              # the same model states, step by step
        for ta, tb in zip(trace(rec), trace(rec)):
            assert all(np.array_equal(ta["model"].m[cid], tb["model"].m[cid]) for cid in rec["containers"])
    for rec in a:
        assert all(tuple(o) in _sweep.SESSION_OPTIONS[rec["kind"]] for o in rec["options"])
        assert all((st["key"], st["value"]) in _sweep.SESSION_OPTIONS[rec["kind"]] for st in rec["steps"] if st["op"] == "set_option")


def test_session_shapes_stay_small_and_reach_the_edges():
    recs = session_records()
    rows = [n for rec in recs for t in trace(rec) if is_query(t) for n in [t["after"][t["st"]["on"]]]]
    assert max(rows) <= 1100 and sum(n < 300 for n in rows) > 0.9 * len(rows)
    assert 0 in rows and 1 in rows                                                 # a query of an empty and of a one-row container
    for edge in (64, 128, 256, 512, 1024):
        assert any(edge // 2 < n <= edge for n in rows) and any(edge < n <= 2 * edge for n in rows), edge
    storm = [rec for rec in recs if rec["kind"] == "storm"]
    assert {len([c for c in rec["containers"].values() if c["type"] == "storm"]) for rec in storm} == {1, 2}
    assert all(c["width"] <= 4096 and c["width"] in _sweep.M_SET for rec in storm for c in rec["containers"].values() if c["type"] == "contig")
    assert all(c["S"] in _sweep.S_SET for rec in storm for c in rec["containers"].values() if c["type"] == "dosage")
    kinds = {st.get("row_kind") for rec in storm for st in rec["steps"] if st["op"] == "add"}
    assert {"short", "bitmap", "far"} <= kinds
    ops = {st["op"] for rec in recs for st in rec["steps"]}
    assert set(_sweep.MUTATIONS) | {"set_option", "query", "hip_invalidate"} == ops
    for kind in _sweep.SESSION_KINDS:
        asked = {st["kind"] for rec in recs if rec["kind"] == kind for st in rec["steps"] if st["op"] == "query"}
        assert asked == set(_sweep.session_queries(kind)), (kind, set(_sweep.session_queries(kind)) - asked)
    margins = [float(_sweep.session_answer(t["model"], t["i"])["margin"]) for rec in storm for t in trace(rec) if is_query(t, kinds=("lag_prune",))]
    assert margins and min(margins) >= _sweep.PRUNE_MARGIN                          # min_r2 stands clear of every in-window r^2


def test_no_mutation_of_a_session_is_invisible():
    for rec in session_records():
        assert _sweep.invisible_mutations(rec) == [], (rec["seed"], rec["index"])


def test_an_invisible_mutation_is_rejected():
    """hand-made: an upload that no query of its matrix follows before the next upload, and a resize to the same row count"""
    q = {"op": "query", "kind": "pairw_matrix", "pad": 1, "off": 0, "max_lag": 3, "bit_op": "and", "measure": "jaccard", "k": 2,
         "score": "count", "world": 1, "row0": 0}
    rec = {"kind": "hip", "input_seed": 5, "options": [], "containers": {c: {"type": "hip", "words": 1, "n": 8} for c in ("h0", "h1")},
           "steps": [{"op": "upload", "on": "h0", "row0": 0, "rows": 8}, dict(q, on="h0"),
                     {"op": "upload", "on": "h1", "row0": 0, "rows": 8}, dict(q, on="h1"),
                     {"op": "upload", "on": "h0", "row0": 2, "rows": 3}, dict(q, on="h1"),     # step 4: only h1 is asked
                     {"op": "upload", "on": "h0", "row0": 4, "rows": 2}, dict(q, on="h0"),
                     {"op": "resize", "on": "h1", "n": 8}, dict(q, on="h1"),                   # step 8: nothing changes
                     {"op": "resize", "on": "h1", "n": 5}, dict(q, on="h1", kind="total"), dict(q, on="h1")]}
    assert _sweep.invisible_mutations(rec) == [4, 8]
    rec["steps"][5]["on"] = "h0"
    assert _sweep.invisible_mutations(rec) == [8]


def off_lists(t):
    """the query of this step runs on the dense paths QUERY_KINDS is about: not a Storm's total (its arena), not a Storm whose
    matrix comes from its lists — matrix_lists 1 or -1 on a container that test_gpu_storm_edges.py's rule calls K5-eligible;
    two Storms (K5x): only matrix_lists 0 counts"""
    from tests.test_gpu_storm_edges import _k5_eligible
    st, model = t["st"], t["model"]
    if model.type(st["on"]) != "storm":
        return True
    if st["kind"] == "total":
        return False
    if t["opts"]["matrix_lists"] == 0:
        return True
    return "other" not in st and not _k5_eligible([_sweep.storm_positions(row) for row in model.m[st["on"]]])


@pytest.mark.parametrize("kind", _sweep.SESSION_KINDS)
def test_every_hand_over_of_a_shared_buffer_occurs(kind):
    """consecutive queries (mutations and option steps may stand between them), both on the dense paths"""
    seen, per_seed = set(), {}
    for rec in session_records():
        if rec["kind"] == kind:
            asked = [(t["st"]["kind"], off_lists(t)) for t in trace(rec) if is_query(t)]
            pairs = {(a[0], b[0]) for a, b in zip(asked, asked[1:]) if a[1] and b[1]}
            seen |= pairs
            per_seed.setdefault(rec["seed"], set()).update(pairs)
    table = _sweep.session_handovers(kind)
    assert set(table) == set(_sweep.SESSION_BUFFERS)
    for buf, pairs in table.items():
        assert len(pairs) >= 2, buf
        missing = [p for p in pairs if p not in seen]
        assert not missing, (buf, len(missing), missing[:8])
    for seed, pairs in per_seed.items():                                           # the strip list's hand-over in every seed
        assert {("total", "square_total"), ("square_total", "total")} <= pairs, seed


@pytest.mark.parametrize("seed", _sessions.SEEDS)
def test_every_option_of_the_table_is_set(seed):
    for kind in _sweep.SESSION_KINDS:
        done = {(st["key"], st["value"]) for rec in session_records(seed) if rec["kind"] == kind for st in rec["steps"]
                if st["op"] == "set_option"}
        assert done == set(_sweep.SESSION_OPTIONS[kind]), (kind, set(_sweep.SESSION_OPTIONS[kind]) - done)


def _around(tr, i, cid):
    """a query of `cid` right before and right behind step i"""
    return i > 0 and i + 1 < len(tr) and is_query(tr[i - 1], cid) and is_query(tr[i + 1], cid)


@pytest.mark.parametrize("seed", _sessions.SEEDS)
def test_growth_across_the_pads_and_the_first_reallocation(seed):
    crossed, realloc = set(), False
    for rec in session_records(seed):
        tr = trace(rec)
        alloc, grown = {}, set()      # the mirror's allocated rows (storm_hip_matrix_create / _resize), made by the first query
        for t in tr:
            st, cid = t["st"], t["st"].get("on")
            ctype = rec["containers"][cid]["type"] if cid else None
            if st["op"] in ("clear", "free_new") and ctype != "hip":
                alloc.pop(cid, None)
                grown.discard(cid)
            if ctype == "hip" and (st["op"] == "free_new" or t["i"] == 0 or cid not in alloc):
                alloc[cid] = max(256, -(-t["after" if st["op"] == "free_new" else "before"][cid] // 256) * 256)
                grown.discard(cid) if st["op"] == "free_new" else None
            if st["op"] == "query" and ctype == "dosage" and cid not in alloc and t["after"][cid] >= 2:
                alloc[cid] = max(256, -(-t["after"][cid] // 256) * 256)
            if st["op"] in ("add", "resize") and _around(tr, t["i"], cid):
                for edge in (256, 512, 1024):
                    if t["before"][cid] <= edge < t["after"][cid]:
                        crossed.add(edge)
                if cid in alloc and t["after"][cid] > alloc[cid]:
                    realloc = realloc or cid not in grown
            if st["op"] in ("add", "resize") and cid in alloc and t["after"][cid] > alloc[cid]:
                grown.add(cid)
                alloc[cid] = max(-(-t["after"][cid] // 256) * 256, 2 * alloc[cid])
    assert crossed == {256, 512, 1024} and realloc


@pytest.mark.parametrize("seed", _sessions.SEEDS)
def test_a_storm_loses_k5_eligibility_and_regains_it_behind_clear(seed):
    from tests.test_gpu_storm_edges import _k5_eligible
    done = False
    for rec in session_records(seed):
        for cid in (c for c, v in rec["containers"].items() if v["type"] == "storm"):
            phase, lists, cleared = 0, set(), False                                # phases: eligible, not, eligible behind a clear
            for t in trace(rec):
                st = t["st"]
                if st.get("on") == cid and st["op"] == "clear":
                    cleared = phase == 2
                if phase == 3 or not is_query(t, kinds=("pairw_matrix",)) or st["on"] != cid:
                    continue
                eligible = _k5_eligible([_sweep.storm_positions(row) for row in t["model"].m[cid]])
                if eligible != (phase != 1) or (phase == 2 and not cleared):
                    lists = set()
                    continue
                lists.add(t["opts"]["matrix_lists"])                               # a query in the phase under matrix_lists 1 and -1
                if {1, -1} <= lists:
                    phase, lists = phase + 1, set()
            done = done or phase == 3
    assert done


def _steps_between(tr, i, k, cid, ops=_sweep.MUTATIONS):
    return [t for t in tr[i + 1:k] if t["st"]["op"] in ops and t["st"].get("on") == cid]


def _same_answer(tr, i, k):
    a, b = tr[i]["st"], tr[k]["st"]
    return a["kind"] == b["kind"] and a["on"] == b["on"] and a.get("other") == b.get("other") and \
        not _sweep.answers_differ(_sweep.session_answer(tr[i]["model"], i), _sweep.session_answer(tr[k]["model"], k))


@pytest.mark.parametrize("seed", _sessions.SEEDS)
def test_the_named_transitions_of_a_storm_session(seed):
    found = set()
    for rec in session_records(seed):
        if rec["kind"] != "storm":
            continue
        tr = trace(rec)
        blocks = lambda t, cid: int(np.flatnonzero(t["model"].m[cid].any(axis=0)).max(initial=-1)) // _sweep.STORM_SPAN + 1
        for i, t in enumerate(tr):
            st = t["st"]
            if st["op"] in _sweep.MUTATIONS and 0 < i and i + 3 < len(tr) and is_query(tr[i - 1]) and tr[i - 1]["st"]["on"] != st["on"]:
                for k in (i + 1, i + 2, i + 3):            # a mutation of B between two equal queries of an unchanged A
                    if is_query(tr[k]) and _same_answer(tr, i - 1, k) and not _steps_between(tr, i - 1, k, tr[k]["st"]["on"]):
                        found.add("free between" if st["op"] == "free_new" else "B between")
            if st["op"] == "add" and rec["containers"][st["on"]]["type"] == "dosage" and t["before"][st["on"]] >= 2:
                asked = [u for u in tr[:i] if is_query(u, st["on"]) or u["st"]["op"] in ("clear", "free_new") and u["st"]["on"] == st["on"]]
                if asked and asked[-1]["st"]["op"] == "query" and i + 1 < len(tr) and is_query(tr[i + 1], st["on"]):
                    found.add("incremental upload")        # rows [synced, n_rows) go up behind a query
            if st["op"] == "clear":
                later = [u for u in tr[i + 1:] if is_query(u, st["on"]) and u["after"][st["on"]] > 0]
                if later and later[0]["after"][st["on"]] < t["before"][st["on"]] and not _steps_between(tr, i, later[0]["i"], st["on"], ("clear", "free_new")):
                    found.add("clear, fewer rows")
            if i + 1 < len(tr) and is_query(t) and is_query(tr[i + 1]) and st["on"] == tr[i + 1]["st"]["on"]:
                a, b = st["kind"], tr[i + 1]["st"]["kind"]
                if a in NXN and b.startswith("lag_"):
                    found.add("lag behind n x n")
                if b in NXN and a.startswith("lag_"):
                    found.add("n x n behind lag")
            # the dense replica: A alone, A x a wider B, A alone, A grown, A x B again — under matrix_lists 0, A never cleared
            if is_query(t, kinds=("square_matrix",)) and t["opts"]["matrix_lists"] == 0 and blocks(t, st["other"]) > blocks(t, st["on"]):
                a = st["on"]
                rest = tr[i + 1:]
                alone = [u for u in rest if is_query(u, a, ("pairw_matrix",)) and u["st"]["on"] == a]
                grown = [u for u in rest if alone and u["i"] > alone[0]["i"] and u["st"]["op"] == "add" and u["st"]["on"] == a]
                again = [u for u in rest if grown and u["i"] > grown[0]["i"] and is_query(u, kinds=("square_matrix",)) and u["st"]["on"] == a
                         and u["st"]["other"] == st["other"] and u["opts"]["matrix_lists"] == 0]
                first = [u for u in tr[:i] if is_query(u, a, ("pairw_matrix",)) and u["opts"]["matrix_lists"] == 0]
                if first and again and not _steps_between(tr, first[-1]["i"], again[0]["i"], a, ("clear", "free_new")):
                    found.add("replica widened")
    assert found == {"B between", "free between", "incremental upload", "clear, fewer rows", "lag behind n x n", "n x n behind lag",
                     "replica widened"}


@pytest.mark.parametrize("seed", _sessions.SEEDS)
def test_the_named_transitions_of_a_hip_session(seed):
    found = set()
    for rec in session_records(seed):
        if rec["kind"] != "hip":
            continue
        tr = trace(rec)
        assert all(c["n"] <= 256 for c in rec["containers"].values())               # (the allocation a resize stays inside or leaves)
        for i, t in enumerate(tr):
            st = t["st"]
            if st["op"] == "upload" and 0 < st["row0"] and st["row0"] + st["rows"] < t["before"][st["on"]] and _around(tr, i, st["on"]):
                if all(u["opts"]["keep_shadow"] == 1 and u["st"].get("kind", "total") == "total" for u in tr[i - 1:i + 2]):
                    found.add("keep_shadow across an upload")
            if st["op"] == "resize":
                found.add("resize down" if t["after"][st["on"]] < t["before"][st["on"]] else
                          "resize up inside" if t["after"][st["on"]] <= 256 else "resize past the allocation")
            if st["op"] in _sweep.MUTATIONS and 0 < i and i + 2 < len(tr) and is_query(tr[i - 1]) and tr[i - 1]["st"]["on"] != st["on"]:
                if is_query(tr[i + 2]) and _same_answer(tr, i - 1, i + 2):
                    found.add("B between")
            if i + 1 < len(tr) and is_query(t) and is_query(tr[i + 1]) and st["on"] == tr[i + 1]["st"]["on"]:
                found |= {"lag behind n x n"} if st["kind"] in NXN and tr[i + 1]["st"]["kind"].startswith("lag_") else set()
                found |= {"n x n behind lag"} if tr[i + 1]["st"]["kind"] in NXN and st["kind"].startswith("lag_") else set()
    assert found == {"keep_shadow across an upload", "resize down", "resize up inside", "resize past the allocation", "B between",
                     "lag behind n x n", "n x n behind lag"}


def test_the_model_against_rows_kept_in_plain_lists():
    """the model's mutation functions, step by step, against Python lists written one row (one bit) at a time"""
    recs = session_records(1)
    for rec in (recs[4], recs[1], recs[3]):                                        # storm (the small theme), hip, hip with growth
        state = {cid: [[0] * (64 * c["words"]) for _ in range(c["n"])] if c["type"] == "hip" else [] for cid, c in rec["containers"].items()}
        for t in trace(rec):
            st = t["st"]
            if st["op"] not in _sweep.MUTATIONS:
                continue
            cid, rows = st["on"], state[st["on"]]
            hip = rec["containers"][cid]["type"] == "hip"
            width = t["model"].m[cid].shape[1]
            new = _sweep.session_rows(rec, t["i"]).tolist() if "rows" in st else []
            if st["op"] == "add":
                for row in new:
                    rows.append(row)
            elif st["op"] == "clear":
                state[cid] = [[0] * width for _ in rows] if hip else []
            elif st["op"] == "free_new":
                state[cid] = [[0] * width for _ in range(st.get("n", 0))]
            elif st["op"] == "resize":
                while len(rows) > st["n"]:
                    rows.pop()
                while len(rows) < st["n"]:
                    rows.append([0] * width)
            else:
                for r, row in enumerate(new):
                    if st["op"] == "set_rows_from_positions":                      # sets bits, clears none
                        for col, bit in enumerate(row):
                            if bit:
                                rows[st["row0"] + r][col] = 1
                    else:
                        rows[st["row0"] + r] = row
            want = np.array(state[cid], dtype=np.uint8).reshape(len(state[cid]), width)
            assert np.array_equal(t["model"].m[cid], want), (rec["index"], t["i"], st["op"])
