"""r / r^2 and the numbers of shared samples between TWO dosage containers on the device (storm.h: STORM_dosage_square_corr,
_square_nobs, _square_corr_complete): every row of A against every row of B — K2h in its dosage form over the rectangle, the
rows' sums of both containers or six products of their split rows, and a finishing pass in place. Everything goes through the
C-ABI, in the host and the _device forms, which must be bit-identical.

The reference is numpy on the unpacked rows (tests/_sweep.py: dosage_sums, corr_plain64, corr_complete64): N EQUAL, and for
the correlations close_floats' rule — the one NaN pattern exactly on the integer mask, elsewhere at most 1 float32 ulp from
the float64 value (tests/test_dosage_complete_math.py derives the bound on the CPU). Against the shipped pairw_* calls on the
stacked container the comparison is bit for bit. Outputs are pre-filled with a sentinel, have out_rows = n_a + 1 and
ld > n_b: every entry of the n_a x n_b window is written and nothing outside it."""
import ctypes as C

import numpy as np
import pytest

import stormbitmaps_amd as sb
from tests._sweep import Stats, close_floats, corr_complete64, corr_plain64, dosage_sums, equal
from tests.test_gpu_dosage import SENTINEL, SENTINEL_I32, Dosage, pack
from tests.test_gpu_dosage_complete import Complete

pytestmark = pytest.mark.gpu

MEASURES = {"r2": 0, "r": 1}
KINDS = ("corr", "complete", "nobs")
NAMES = {"corr": "STORM_dosage_square_corr", "complete": "STORM_dosage_square_corr_complete", "nobs": "STORM_dosage_square_nobs"}


# ------------------------------------------------------------------------------------------ helpers
def _args(kind, measure):
    return () if kind == "nobs" else (MEASURES[measure],)


def square_host(a, b, kind, measure="r2", ld=None):
    """the host form into a sentinel-filled [n_a + 1, ld] array, as uint32"""
    ld = b.n + 3 if ld is None else ld
    out = np.full((a.n + 1, ld), SENTINEL, dtype=np.uint32)
    a.ok(getattr(a.lib, NAMES[kind])(a.h, b.h, *_args(kind, measure), out.ctypes.data, a.n + 1, ld), NAMES[kind])
    return out


def square_device(a, b, kind, measure="r2", ld=None, off=0):
    """the _device form into a sentinel-filled device buffer of [n_a + 1, ld] words that starts `off` words behind a 16-byte
    boundary; the words in front of it must come back untouched"""
    import torch
    ld = b.n + 5 if ld is None else ld
    flat = torch.full((off + (a.n + 1) * ld,), SENTINEL_I32, dtype=torch.int32, device="cuda:0")
    assert flat.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    name = NAMES[kind] + "_device"
    a.ok(getattr(a.lib, name)(a.h, b.h, *_args(kind, measure), C.c_void_p(flat.data_ptr() + 4 * off), a.n + 1, ld), name)
    got = flat.cpu().numpy().view(np.uint32)
    assert (got[:off] == SENTINEL).all(), (name, "written in front of the output")
    return got[off:].reshape(a.n + 1, ld)


def window(got, na, nb, what):
    """the n_a x n_b window of an output once everything outside it still holds the sentinel"""
    outside = np.ones(got.shape, dtype=bool)
    outside[:na, :nb] = False
    equal(got, np.full(got.shape, SENTINEL, dtype=np.uint32), f"{what}: written outside the window", outside)
    return got[:na, :nb]


def both_forms(a, b, kind, measure="r2", ld_host=None, ld_dev=None, off=0):
    """the window from the host form, which the _device form must equal bit for bit"""
    what = f"{NAMES[kind]} {measure} {a.n} x {b.n} S {a.S}"
    host = window(square_host(a, b, kind, measure, ld_host), a.n, b.n, what + " (host form)")
    dev = window(square_device(a, b, kind, measure, ld_dev, off), a.n, b.n, what + " (device form)")
    equal(dev, host, what + ": the device form against the host form")
    return host


def check_against_numpy(a, b, Ga, Gb, stats, **forms):
    """rule 1: r and r^2, plain and complete, and N of the rectangle against numpy on the unpacked rows; returns the windows"""
    sums = dosage_sums(Ga, Gb)
    everywhere = np.ones((a.n, b.n), dtype=bool)
    what = f"{a.n} x {b.n} S {a.S}"
    got = {"nobs": both_forms(a, b, "nobs", **forms)}
    equal(got["nobs"], sums["N"].astype(np.uint32), f"square_nobs {what}")
    for measure in ("r2", "r"):
        got["corr", measure] = both_forms(a, b, "corr", measure, **forms)
        close_floats(stats, got["corr", measure], *corr_plain64(sums, a.S, measure), everywhere, f"square_corr {measure} {what}")
        got["complete", measure] = both_forms(a, b, "complete", measure, **forms)
        close_floats(stats, got["complete", measure], *corr_complete64(sums, measure), everywhere,
                     f"square_corr_complete {measure} {what}")
    return got


def genotypes(rng, n, S, missing=0.1):
    """[n, S] uint8: 0 / 1 / 2 with allele frequencies of their own per row, 3 at `missing` of the samples"""
    p = rng.uniform(0.05, 0.95, size=(n, 1))
    G = (rng.random((n, S)) < p).astype(np.uint8) + (rng.random((n, S)) < p).astype(np.uint8)
    G[rng.random((n, S)) < missing] = 3
    return G


def containers(lib, *Gs):
    return [Complete(lib, G, packed_only=G.shape[0] > 64) for G in Gs]


def close_all(*ds):
    for d in ds:
        d.close()


# ------------------------------------------------------------------------------------------ 1. against numpy
# every shape pair of the list and every sample count of the list at least once: two sample counts per shape pair
SHAPES = ((1, 1), (1, 129), (2, 127), (127, 2), (128, 128), (129, 257), (257, 130))
SAMPLES = (1, 31, 32, 33, 255, 256, 257, 1000, 4097)
CASES = [(na, nb, SAMPLES[(2 * k + h) % len(SAMPLES)]) for k, (na, nb) in enumerate(SHAPES) for h in (0, 1)]
assert {s for _, _, s in CASES} == set(SAMPLES) and {(na, nb) for na, nb, _ in CASES} == set(SHAPES)


@pytest.mark.parametrize("na,nb,S", CASES)
def test_against_numpy(lib, na, nb, S):
    rng = np.random.default_rng([na, nb, S])
    Ga, Gb = genotypes(rng, na, S), genotypes(rng, nb, S)
    a, b = containers(lib, Ga, Gb)
    stats = Stats()
    try:
        check_against_numpy(a, b, Ga, Gb, stats)
    finally:
        close_all(a, b)
    print(f"\nsquare {na} x {nb} S {S}: worst {stats.worst_ulp} ulp")


# ------------------------------------------------------------------------------------------ 2. long rows
def test_long_rows_split_along_k(lib):
    """65536 samples: the launch cuts its few tiles along k, and the parts' sums meet inside it"""
    rng = np.random.default_rng(65536)
    Ga, Gb = genotypes(rng, 3, 65536), genotypes(rng, 5, 65536)
    a, b = containers(lib, Ga, Gb)
    stats = Stats()
    try:
        check_against_numpy(a, b, Ga, Gb, stats)
    finally:
        close_all(a, b)
    print(f"\nsquare 3 x 5 S 65536: worst {stats.worst_ulp} ulp")


@pytest.mark.parametrize("value,kind", [(3, "corr"), (2, "complete")])
def test_the_largest_sums(lib, value, kind):
    """1 x 1 at 2^24 samples, all 3s for the plain form and all 2s for the complete one: the largest P, s, q and N there are
    (S P = 9 x 2^48, N P = 2^50: every term below 2^64). Both rows are constant, so the float is the NaN pattern; N and the
    plain form's view of the all-2s row come along."""
    S = 1 << 24
    word = np.uint64(0xFFFFFFFFFFFFFFFF if value == 3 else 0xAAAAAAAAAAAAAAAA)
    words = np.full((1, S // 32), word, dtype=np.uint64)
    G = np.full((1, S), value, dtype=np.uint8)
    a, b = Complete(lib, None, words=words, n_samples=S), Complete(lib, None, words=words, n_samples=S)
    stats = Stats()
    try:
        sums = dosage_sums(G, G)
        assert int(sums["P"][0, 0]) == value * value * S
        one = np.ones((1, 1), dtype=bool)
        for measure in ("r2", "r"):
            got = both_forms(a, b, kind, measure)
            ref = corr_plain64(sums, S, measure) if kind == "corr" else corr_complete64(sums, measure)
            assert ref[1].all()
            close_floats(stats, got, *ref, one, f"square_{kind} {measure} at 2^24 samples of {value}")
        equal(both_forms(a, b, "nobs"), sums["N"].astype(np.uint32), "square_nobs at 2^24 samples")
        assert int(sums["N"][0, 0]) == (0 if value == 3 else S)
    finally:
        close_all(a, b)


def test_near_the_largest_sums_without_a_constant_row(lib):
    """the same 2^24 samples with one sample of each row changed, so that no row is constant and the float is a number"""
    S = 1 << 24
    Ga, Gb = np.full((1, S), 2, dtype=np.uint8), np.full((1, S), 2, dtype=np.uint8)
    Ga[0, 0], Gb[0, 0], Gb[0, S - 1] = 0, 1, 0
    a = Complete(lib, None, words=pack(Ga), n_samples=S)
    b = Complete(lib, None, words=pack(Gb), n_samples=S)
    stats = Stats()
    try:
        check_against_numpy(a, b, Ga, Gb, stats)
    finally:
        close_all(a, b)
    assert stats.worst_ulp <= 1


# ------------------------------------------------------------------------------------------ 3. the shipped calls' bits
@pytest.mark.parametrize("na,nb,S,missing", [(129, 130, 1000, 0.1), (5, 300, 33, 0.3), (130, 3, 257, 0.0)])
def test_bit_identity_with_the_stacked_container(lib, na, nb, S, missing):
    """square_*(a, b)[i, j] is pairw_* of the container [a ; b] at (i, n_a + j): no tolerance"""
    rng = np.random.default_rng([3, na, nb, S])
    Ga, Gb = genotypes(rng, na, S, missing), genotypes(rng, nb, S, missing)
    a, b, stacked = containers(lib, Ga, Gb, np.concatenate([Ga, Gb]))
    n = na + nb
    try:
        for measure, code in MEASURES.items():
            equal(both_forms(a, b, "corr", measure), stacked.corr_host(code)[:na, na:n], f"square_corr {measure} against pairw_corr")
            equal(both_forms(a, b, "complete", measure), stacked.complete_host(code)[:na, na:n],
                  f"square_corr_complete {measure} against pairw_corr_complete")
            if missing == 0.0:
                equal(both_forms(a, b, "complete", measure), both_forms(a, b, "corr", measure),
                      f"square_corr_complete {measure} against square_corr on rows without a 3")
        equal(both_forms(a, b, "nobs"), stacked.nobs_host()[:na, na:n], "square_nobs against pairw_nobs")
    finally:
        close_all(a, b, stacked)


@pytest.mark.parametrize("n,S", [(131, 300), (2, 31)])
def test_a_container_against_itself(lib, n, S):
    """square_*(a, a): pairw_*(a) at i < j, its transpose at i > j (bit for bit), the numpy reference on the diagonal"""
    rng = np.random.default_rng([33, n, S])
    G = genotypes(rng, n, S, 0.15)
    a, = containers(lib, G)
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    stats = Stats()
    try:
        got = check_against_numpy(a, a, G, G, stats)                  # (the diagonal included)
        for measure, code in MEASURES.items():
            for kind, tri in (("corr", a.corr_host(code)[:n, :n]), ("complete", a.complete_host(code)[:n, :n])):
                equal(got[kind, measure], tri, f"square_{kind} {measure}(a, a) above the diagonal", upper)
                equal(got[kind, measure].T, tri, f"square_{kind} {measure}(a, a) below the diagonal", upper)
        tri = a.nobs_host()[:n, :n]
        equal(got["nobs"], tri, "square_nobs(a, a) above the diagonal", upper)
        equal(got["nobs"].T, tri, "square_nobs(a, a) below the diagonal", upper)
    finally:
        close_all(a)


def test_complete_gives_the_plain_bits_without_a_missing_value(lib):
    rng = np.random.default_rng(34)
    Ga, Gb = genotypes(rng, 70, 515, 0.0), genotypes(rng, 133, 515, 0.0)
    Ga[3], Gb[7] = 1, 0                                                    # constant rows: NaN in both forms
    a, b = containers(lib, Ga, Gb)
    try:
        for measure in MEASURES:
            equal(both_forms(a, b, "complete", measure), both_forms(a, b, "corr", measure), f"complete against plain, {measure}")
        assert (both_forms(a, b, "nobs") == 515).all()
    finally:
        close_all(a, b)


# ------------------------------------------------------------------------------------------ 4. structured rows
def test_structured_rows(lib):
    """constant rows on either side (a NaN row, a NaN column), all-missing rows, pairs that share exactly 0, 1 and 2 samples, a
    row constant only on the samples it shares, and rows missing exactly the tail samples of the last word"""
    S = 70                                                                 # the last word holds samples 64 .. 69
    rng = np.random.default_rng(4)
    Ga, Gb = genotypes(rng, 9, S, 0.0), genotypes(rng, 8, S, 0.0)
    Ga[0] = 2                                                              # constant: a NaN row in both forms
    Gb[0] = 0                                                              # constant: a NaN column
    Ga[1] = 3                                                              # all missing: N = 0 along the row
    Gb[1] = 3
    Ga[2, 30:], Gb[2, :30] = 3, 3                                          # share no sample
    Ga[3, 31:], Gb[3, :30] = 3, 3                                          # share sample 30 alone
    Ga[4, 32:], Gb[4, :30] = 3, 3                                          # share samples 30 and 31
    Ga[4, 30:32], Gb[4, 30:32] = (0, 2), (1, 2)                            # ... on which neither is constant: r = 1
    Ga[5, :40], Ga[5, 40:] = np.arange(40) % 3, 1                          # constant on what it shares with ...
    Gb[5, :40] = 3                                                         # ... this row, and only there
    Ga[6, 64:], Gb[6, 64:] = 3, 3                                          # missing exactly the last word's samples
    Ga[7, :64] = 3                                                         # present in the last word's samples alone
    a, b = containers(lib, Ga, Gb)
    stats = Stats()
    try:
        got = check_against_numpy(a, b, Ga, Gb, stats)
        N = got["nobs"].astype(np.int64)
        assert (N[1] == 0).all() and (N[:, 1] == 0).all() and N[2, 2] == 0 and N[3, 3] == 1 and N[4, 4] == 2
        assert N[6, 6] == 64 and N[7, 6] == 0 and N[7, 7] == 6 and N[8, 7] == S
        for measure in MEASURES:
            plain, comp = got["corr", measure], got["complete", measure]
            nan = np.uint32(0x7FC00000)
            assert (plain[0] == nan).all() and (plain[:, 0] == nan).all() and (comp[0] == nan).all() and (comp[:, 0] == nan).all()
            assert (comp[1] == nan).all() and (comp[:, 1] == nan).all()
            assert comp[2, 2] == nan and comp[3, 3] == nan and comp[5, 5] == nan and plain[5, 5] != nan
            assert comp[4, 4] == np.float32(1.0).view(np.uint32)
    finally:
        close_all(a, b)


# ------------------------------------------------------------------------------------------ 5. store paths
@pytest.mark.parametrize("nb,ld,off", [
    (130, 135, 0),     # ld % 4 != 0: entry by entry
    (130, 136, 1),     # ld % 4 == 0 on a base 4 bytes behind a 16-byte boundary: entry by entry
    (129, 132, 0),     # aligned: 128-bit accesses, and a last lane with 1 of its 4 columns
    (130, 132, 0),     # ... with 2
    (131, 132, 0),     # ... with 3
    (260, 260, 0),     # aligned, no pitch columns, a second column tile of 4 columns
])
def test_vector_and_scalar_store_paths(lib, nb, ld, off):
    na, S = 67, 200
    rng = np.random.default_rng([5, nb, ld, off])
    Ga, Gb = genotypes(rng, na, S), genotypes(rng, nb, S)
    a, b = containers(lib, Ga, Gb)
    stats = Stats()
    try:
        check_against_numpy(a, b, Ga, Gb, stats, ld_host=ld, ld_dev=ld, off=off)
    finally:
        close_all(a, b)


# ------------------------------------------------------------------------------------------ 6. scratch reuse
def test_scratch_is_reused_across_shapes_and_callers(lib):
    """a large rectangle, a small one, the pairwise-complete triangle of one of the containers (one split in the scratch the
    rectangle keeps two in), and the large rectangle again: every result is still right"""
    rng = np.random.default_rng(6)
    S = 1500
    Ga, Gb, Gc, Gd = genotypes(rng, 300, S), genotypes(rng, 390, S), genotypes(rng, 3, S), genotypes(rng, 5, S)
    a, b, c, d = containers(lib, Ga, Gb, Gc, Gd)
    stats = Stats()
    try:
        first = check_against_numpy(a, b, Ga, Gb, stats)
        check_against_numpy(c, d, Gc, Gd, stats)
        check_against_numpy(c, b, Gc, Gb, stats)
        sums = dosage_sums(Gb)
        upper = np.triu(np.ones((b.n, b.n), dtype=bool), 1)
        for measure, code in MEASURES.items():
            host, dev = b.complete_host(code)[:b.n, :b.n], b.complete_device(code)[:b.n, :b.n]
            equal(dev, host, f"pairw_corr_complete {measure}: device against host", upper)
            close_floats(stats, host, *corr_complete64(sums, measure), upper, f"pairw_corr_complete {measure} after the rectangles")
            equal(both_forms(a, b, "complete", measure), first["complete", measure], f"square_corr_complete {measure} again")
            equal(both_forms(b, b, "complete", measure), host, f"square_corr_complete {measure}(b, b) against the triangle", upper)
        equal(b.nobs_host()[:b.n, :b.n], sums["N"].astype(np.uint32), "pairw_nobs after the rectangles", upper)
        equal(both_forms(a, b, "nobs"), first["nobs"], "square_nobs again")
    finally:
        close_all(a, b, c, d)


# ------------------------------------------------------------------------------------------ the Python methods; the report
def test_python_methods(lib):
    import torch
    rng = np.random.default_rng(7)
    S = 100
    Ga, Gb = genotypes(rng, 6, S), genotypes(rng, 9, S)
    d, other = sb.StormDosage(S), sb.StormDosage(S)
    for row in Ga:
        d.add(row)
    other.add_packed(pack(Gb))
    sums = dosage_sums(Ga, Gb)
    stats = Stats()
    everywhere = np.ones((6, 9), dtype=bool)
    try:
        equal(d.square_nobs(other), sums["N"].astype(np.uint32), "square_nobs")
        for measure in ("r2", "r"):
            for complete, ref in ((False, corr_plain64(sums, S, measure)), (True, corr_complete64(sums, measure))):
                host = d.square_corr(other, measure, complete=complete)
                assert host.dtype == np.float32 and host.shape == (6, 9)
                close_floats(stats, host.view(np.uint32), *ref, everywhere, f"square_corr {measure} complete={complete}")
                t = torch.full((7, 12), -7.5, dtype=torch.float32, device="cuda:0")
                assert d.square_corr(other, measure, complete=complete, device=t) is None
                got = t.cpu().numpy()
                equal(got[:6, :9].view(np.uint32), host.view(np.uint32), "device= against the host form")
                assert (got[6] == -7.5).all() and (got[:, 9:] == -7.5).all()
        t = torch.zeros((6, 9), dtype=torch.int32, device="cuda:0")
        assert d.square_nobs(other, device=t) is None
        equal(t.cpu().numpy().view(np.uint32), sums["N"].astype(np.uint32), "square_nobs device=")
        with pytest.raises(ValueError):
            d.square_corr(other, device=torch.zeros((5, 9), dtype=torch.float32, device="cuda:0"))
    finally:
        d.free()
        other.free()


def test_the_last_pass_report(lib, hip_ctx):
    """storm_hip_square_dosage_*: [0] has STORM_HIP_RAN_TILES_OUT (and _RAN_SIMILARITY for the correlations), [1] is
    n_a n_b n_words, six times that for the pairwise-complete form"""
    rng = np.random.default_rng(8)
    S, na, nb = 700, 5, 140
    n_words = (S + 31) // 32
    Ga, Gb = genotypes(rng, na, S), genotypes(rng, nb, S)
    ma, mb = hip_ctx.matrix_from_host(pack(Ga)), hip_ctx.matrix_from_host(pack(Gb))
    flags = {"STORM_HIP_RAN_TILES_OUT": 128, "STORM_HIP_RAN_SIMILARITY": 512}     # (storm_hip.h)
    sums = dosage_sums(Ga, Gb)
    try:
        for name, args, dtype, factor, similarity in (("corr", (0, S), np.float32, 1, True), ("nobs", (S,), np.uint32, 1, False),
                                                      ("corr_complete", (1, S), np.float32, 6, True)):
            out = np.zeros((na, nb), dtype=dtype)
            rc = getattr(lib, "storm_hip_square_dosage_" + name)(hip_ctx._h, ma._h, mb._h, *args, out.ctypes.data, nb)
            assert rc == 0, (name, lib.storm_hip_last_error())
            report = (C.c_uint64 * 4)()
            assert lib.storm_hip_last_pass_report(hip_ctx._h, report) == 0
            assert report[0] & flags["STORM_HIP_RAN_TILES_OUT"], name
            assert bool(report[0] & flags["STORM_HIP_RAN_SIMILARITY"]) == similarity, name
            assert report[1] == factor * na * nb * n_words, (name, report[1])
            if name == "nobs":
                equal(out, sums["N"].astype(np.uint32), "storm_hip_square_dosage_nobs")
        # a leading dimension below B's rows, an unknown measure, a sample count that does not fill the rows: refused
        out = np.zeros((na, nb), dtype=np.float32)
        assert lib.storm_hip_square_dosage_corr(hip_ctx._h, ma._h, mb._h, 0, S, out.ctypes.data, nb - 1) == -1
        assert lib.storm_hip_square_dosage_corr_complete(hip_ctx._h, ma._h, mb._h, 2, S, out.ctypes.data, nb) == -1
        assert b"measure" in lib.storm_hip_last_error()
        assert lib.storm_hip_square_dosage_nobs(hip_ctx._h, ma._h, mb._h, S + 40, out.ctypes.data, nb) == -1
        assert (out == 0).all()
    finally:
        ma.close()
        mb.close()
