"""The dosage container's pairwise calls in the lag layout on the device (storm.h: STORM_dosage_pairw_lag_dot, _lag_corr,
_lag_nobs, _lag_corr_complete; storm_hip.h: storm_hip_pairw_lag_dosage_*): K2h in its lag and dosage form
(tile128_kernel<true, 2>), finish_lag_tiles_kernel<DosageStat>, and for rows with missing genotypes the interleaved split (G, H, M as
one matrix of 3 n rows), one launch at lag 3 L + 2 and dosage_complete_finish_lag_kernel. Everything goes through the
C-ABI, in the host and the _device forms.

Expected values: the dot products and the shared-sample counts from numpy on the unpacked values (EQUAL); the correlations
from the n x n calls of this library on the same container, bit for bit and NaN for NaN (no tolerance), and once against
numpy's float64 value at the 1 ulp of tests/test_gpu_dosage.py and tests/test_gpu_dosage_complete.py. Device outputs are
pre-filled with a sentinel: the lower-right corner (i + 1 + d >= n), the pitch columns [L, ld) and the row behind the last
must not change; host forms write 0 into the corner."""
import ctypes as C

import numpy as np
import pytest

import stormbitmaps_amd as sb
from stormbitmaps_amd import dist
from tests.test_gpu_dosage import NAN_BITS, SENTINEL, WEIGHT, Dosage, genotypes, ordered, pack  # noqa: F401
from tests.test_gpu_dosage_complete import Complete, complete_reference, complete_sums
from tests.test_gpu_lag_matrix import device_buffer, lag_mask, lag_of, read_back, report, to_lag

pytestmark = pytest.mark.gpu

RAN_TILES_OUT, RAN_SIMILARITY = 128, 512   # STORM_HIP_RAN_* (storm_hip.h)
LAGS = (1, 63, 64, 65, 127, 128, 129, 299, 1000)


# ------------------------------------------------------------------------------------------ helpers
class Lag(Complete):
    """tests/test_gpu_dosage_complete.py's container with the lag calls: every call returns the [n, L] window of an
    [n + 1, ld] uint32 buffer after asserting that nothing outside the layout was written"""

    def lag(self, what, max_lag, measure=None, device=False, ld=None):
        n, L = self.n, lag_of(self.n, max_lag)
        ld = L + 3 if ld is None else ld
        f = getattr(self.lib, "STORM_dosage_pairw_lag_" + what + ("_device" if device else ""))
        args = (self.h,) if measure is None else (self.h, measure)
        if device:
            flat, view = device_buffer(n + 1, ld)
            self.ok(f(*args, max_lag, C.c_void_p(view.data_ptr()), n + 1, ld), what)
            got = read_back(view, n + 1, ld)
        else:
            got = np.full((n + 1, ld), SENTINEL, dtype=np.uint32)
            self.ok(f(*args, max_lag, got.ctypes.data, n + 1, ld), what)
        inside = np.zeros(got.shape, dtype=bool)
        inside[:n, :L] = True if not device else lag_mask(n, L)
        assert (got[~inside] == SENTINEL).all(), (what, n, max_lag, device, np.argwhere(~inside & (got != SENTINEL))[:5].tolist())
        if not device:
            assert (got[:n, :L][~lag_mask(n, L)] == 0).all(), (what, n, max_lag)           # 0 / +0.0f in the corner
        return got[:n, :L]

    def both(self, what, max_lag, measure=None):
        """host and device form: equal inside the layout; the host form's window (0 in the corner)"""
        host, dev = self.lag(what, max_lag, measure), self.lag(what, max_lag, measure, device=True)
        ok = lag_mask(self.n, lag_of(self.n, max_lag))
        assert np.array_equal(host[ok], dev[ok]), (what, max_lag, measure)
        return host


def shim_lag_dot(m, max_lag, ld=None, off=0, row0=0, rows=None):
    """storm_hip_pairw_lag_dosage_matrix_device into a sentinel-filled buffer `off` words behind a 16-byte boundary:
    [rows, L], SENTINEL in the corner, after asserting that nothing outside the layout was written"""
    n = m.n_rows
    L = lag_of(n, max_lag)
    ld = L if ld is None else ld
    n_band = n - row0 if rows is None else rows
    flat, view = device_buffer(n_band + 1, ld, off)
    m.pairw_lag_dosage_matrix_device(view.data_ptr(), ld, max_lag, row0, rows)
    got = read_back(view, n_band + 1, ld)
    inside = np.zeros(got.shape, dtype=bool)
    inside[:n_band, :L] = lag_mask(n, L, row0, n_band)
    assert (got[~inside] == SENTINEL).all(), (n, max_lag, ld, off, row0, np.argwhere(~inside & (got != SENTINEL))[:5].tolist())
    if off:
        assert (flat[:off].cpu().numpy().view(np.uint32) == SENTINEL).all()
    return got[:n_band, :L]


def numpy_dot(G):
    """exact: every sum is far below 2^53"""
    g = G.astype(np.float64)
    return (g @ g.T).astype(np.int64)


@pytest.fixture(scope="module")
def hip_ctx():
    ctx = sb.HipContext(0)
    yield ctx
    ctx.close()


@pytest.fixture()
def options(lib, hip_ctx):
    """the K2h part options on the containers' context and on this file's, for the length of one test"""
    def set_options(**kw):
        for k, v in kw.items():
            assert lib.STORM_hip_set_option(k.encode(), v) == 0, k
            hip_ctx.set_option(k, v)
    yield set_options
    set_options(k2_part_min_chunks=8, k2_part_narrow=1)


# ------------------------------------------------------------------------------------------ 1. dot products
@pytest.fixture(scope="module")
def dot300(lib, hip_ctx):
    """300 rows of random values 0 .. 3 per S: the container, the same rows as a device matrix, numpy's products: once"""
    out = {}
    for S in (33, 257, 1000):
        G = np.random.default_rng(300 + S).integers(0, 4, size=(300, S), dtype=np.uint8)
        out[S] = (Lag(lib, G), hip_ctx.matrix_from_host(pack(G)), np.triu(numpy_dot(G), 1).astype(np.uint32))
    yield out
    for d, m, _ in out.values():
        d.close()
        m.close()


@pytest.mark.parametrize("max_lag", LAGS)
@pytest.mark.parametrize("S", [33, 257, 1000])
def test_dot_products_at_the_block_and_tile_edges(dot300, S, max_lag):
    """lags at every 32 / 64 / 128 block edge, the ragged last tile (300 = 2 x 128 + 44), the clipped L (1000 -> 299); one
    chunk short, one chunk and one value, four chunks; host and device forms; a base 4 bytes off 16 with ld > L"""
    d, m, P = dot300[S]
    L = lag_of(300, max_lag)
    assert L == min(max_lag, 299)
    ok = lag_mask(300, L)
    want = to_lag(P, L)
    host, dev = d.lag("dot", max_lag), d.lag("dot", max_lag, device=True)
    assert np.array_equal(host, want), (S, max_lag, np.argwhere(host != want)[:5].tolist())
    assert np.array_equal(dev[ok], want[ok]), (S, max_lag)
    ref = to_lag(P, L, fill=SENTINEL)
    for ld, off in ((L, 0), (L + 3, 1)):
        got = shim_lag_dot(m, max_lag, ld, off)
        assert np.array_equal(got, ref), (S, max_lag, ld, off, np.argwhere(got != ref)[:5].tolist())
    assert np.array_equal(m.pairw_lag_dosage_matrix(max_lag), want)


def test_tiles_that_hold_a_single_wanted_pair(lib, hip_ctx):
    """257 rows, lag 1: tiles (0, 1) and (1, 2) hold exactly one wanted pair each — (127, 128) and (255, 256) — so three of
    their four waves take the block skip and the fourth stores one element of 4096"""
    plan = dist.lag_dosage_plan(257, 32, 1)
    assert {(int(i), int(j)) for i, j in plan[:, :2]} == {(0, 0), (0, 1), (1, 1), (1, 2), (2, 2)}
    G = np.random.default_rng(257).integers(0, 4, size=(257, 1000), dtype=np.uint8)
    P = np.triu(numpy_dot(G), 1).astype(np.uint32)
    d, m = Lag(lib, G), hip_ctx.matrix_from_host(pack(G))
    try:
        assert np.array_equal(d.both("dot", 1), to_lag(P, 1))
        assert np.array_equal(shim_lag_dot(m, 1, ld=1), to_lag(P, 1, fill=SENTINEL))
        assert np.array_equal(shim_lag_dot(m, 1, ld=4, off=1), to_lag(P, 1, fill=SENTINEL))
    finally:
        d.close()
        m.close()


def test_row_bands_concatenate_to_the_whole(hip_ctx):
    """700 rows, lag 200, bands cut at 0 / 130 / 512 / 700 into buffers of their own: 130 is no multiple of 128, so tile
    row 1 is multiplied by two calls and each writes only its own rows; 512 is one"""
    n, max_lag, S = 700, 200, 1000
    G = np.random.default_rng(700).integers(0, 4, size=(n, S), dtype=np.uint8)
    P = np.triu(numpy_dot(G), 1).astype(np.uint32)
    m = hip_ctx.matrix_from_host(pack(G))
    try:
        whole = shim_lag_dot(m, max_lag, ld=max_lag)
        assert np.array_equal(whole, to_lag(P, max_lag, fill=SENTINEL))
        bands = [shim_lag_dot(m, max_lag, ld=max_lag + k, off=k % 2, row0=a, rows=b - a)
                 for k, (a, b) in enumerate(((0, 130), (130, 512), (512, 700)))]
        assert np.array_equal(np.concatenate(bands), whole)
        assert report(hip_ctx)[:2] == [RAN_TILES_OUT, int(lag_mask(n, max_lag, 512, 188).sum()) * m.n_words]
        assert hip_ctx.get_option("k2_tile_shape_used") == 7
    finally:
        m.close()


def test_k_parts_meet_through_the_ticket_path(lib, hip_ctx, options):
    """200 rows x 65536 samples, lag 40: three tiles on a whole chip, so every tile is cut along k and its parts' sums meet
    inside the launch — through windows of 16-bit counts where a part is short enough and, with k2_part_narrow = 0, of
    32-bit counts. The second call of each pair finds the tickets the first one must have reset."""
    n, S, max_lag = 200, 65536, 40
    plan = dist.lag_dosage_plan(n, S // 32, max_lag, n_cus=hip_ctx.get_option("n_cus"))
    assert {(int(i), int(j)) for i, j in plan[:, :2]} == {(0, 0), (0, 1), (1, 1)}
    assert (plan[:, 6] > 1).all(), "a tile is not cut along k: the case would not reach the ticket path"
    G = np.random.default_rng(200).integers(0, 4, size=(n, S), dtype=np.uint8)
    want = to_lag(np.triu(numpy_dot(G), 1).astype(np.uint32), max_lag)
    ok = lag_mask(n, max_lag)
    d = Lag(lib, G, packed_only=True)
    try:
        for narrow in (1, 0):
            options(k2_part_narrow=narrow)
            for rep in range(2):
                got = d.lag("dot", max_lag, device=True)
                assert np.array_equal(got[ok], want[ok]), (narrow, rep, np.argwhere((got != want) & ok)[:5].tolist())
        assert np.array_equal(d.lag("dot", max_lag), want)
    finally:
        d.close()


@pytest.mark.parametrize("S,min_chunks,narrow_planned", [(14848, 29, 0), (14336, 28, 1)])
@pytest.mark.parametrize("narrow_option", [1, 0])
def test_sixteen_bit_windows_stop_where_a_part_could_overflow_them(lib, hip_ctx, options, S, min_chunks, narrow_planned,
                                                                   narrow_option):
    """130 rows of all 3s, lag 100: every product is 9, the most a part can hold. S = 14848 = 58 chunks as two parts of 29: a
    part sums to 66816, beyond 16 bits — wide windows. S = 14336 = 56 chunks as two parts of 28: 64512, just inside — narrow
    windows. Both again with k2_part_narrow = 0. The plan is asserted as well as the result."""
    n, max_lag = 130, 100
    plan = dist.lag_dosage_plan(n, (S + 31) // 32, max_lag, n_cus=hip_ctx.get_option("n_cus"), min_chunks=min_chunks)
    assert len(plan) == 6 and (plan[:, 6] == 2).all() and (plan[:, 3] == min_chunks).all(), plan.tolist()
    assert (plan[:, 7] == narrow_planned).all(), plan.tolist()
    assert (min_chunks * WEIGHT > 65535) == (narrow_planned == 0)
    options(k2_part_min_chunks=min_chunks, k2_part_narrow=narrow_option)
    d = Lag(lib, np.full((n, S), 3, dtype=np.uint8), packed_only=True)
    try:
        want = np.where(lag_mask(n, max_lag), 9 * S, 0).astype(np.uint32)
        assert np.array_equal(d.both("dot", max_lag), want)
        assert 9 * S == {14848: 133632, 14336: 129024}[S]
    finally:
        d.close()


# ------------------------------------------------------------------------------------------ 2. correlations
@pytest.fixture(scope="module")
def corr200(lib, genotypes):  # noqa: F811
    """tests/test_gpu_dosage.py's 200 variants x 1000 samples (three constant rows): the container and the n x n call's bits"""
    G, want, nan, upper = genotypes
    d = Lag(lib, G)
    tri = {measure: d.corr_host(measure)[:200, :200].copy() for measure in (0, 1)}
    yield d, G, tri, want, nan
    d.close()


@pytest.mark.parametrize("max_lag", [1, 65, 128, 199, 1000])
@pytest.mark.parametrize("measure", [0, 1])
def test_lag_corr_is_pairw_corr_bit_for_bit(corr200, measure, max_lag):
    """every entry (i, d) equals STORM_dosage_pairw_corr's at (i, i + 1 + d), the NaN pattern against the constant rows 17,
    128 and 199 included; host and device forms"""
    d, G, tri, want, nan = corr200
    L = lag_of(200, max_lag)
    ref = to_lag(tri[measure], L)
    got = d.both("corr", max_lag, measure)
    assert np.array_equal(got, ref), (measure, max_lag, np.argwhere(got != ref)[:5].tolist())
    ok = lag_mask(200, L)
    assert np.array_equal((got == NAN_BITS) & ok, to_lag(nan, L, fill=False) & ok)
    assert ((got == NAN_BITS) & ok).sum() > 0 and ((got != NAN_BITS) & ok).sum() > 0.9 * ok.sum()


def test_lag_corr_against_numpy(corr200):
    """once against the float64 value itself: at most 1 ulp (the bound of tests/test_gpu_dosage.py, derived in
    tests/test_dosage_math.py)"""
    d, G, tri, want, nan = corr200
    ok = lag_mask(200, 199) & ~to_lag(nan, 199, fill=True)
    for measure in (0, 1):
        got = d.lag("corr", 199, measure, device=True)
        ref = to_lag(want[measure].astype(np.float32).view(np.uint32), 199)
        ulps = np.abs(ordered(got[ok]) - ordered(ref[ok]))
        print(f"measure {measure}: worst error {int(ulps.max())} ulp over {int(ok.sum())} entries")
        assert int(ulps.max()) <= 1


@pytest.mark.parametrize("measure", ["r2", "r"])
def test_finish_pass_alone_on_a_matrix_of_the_callers(hip_ctx, corr200, measure):
    """storm_hip_dosage_finish_lag_device over a caller's matrix of dot products and sums (numpy's, uploaded): the bits of
    the whole call, on an unaligned base with ld > L (the entry-by-entry path) and an aligned one (128-bit accesses), and
    on a row band"""
    import torch
    d, G, tri, _, _ = corr200
    n, S, max_lag = 200, 1000, 70
    g = G.astype(np.int64)
    P = np.triu(g @ g.T, 1).astype(np.uint32)
    s = torch.from_numpy(g.sum(axis=1).astype(np.int32)).to("cuda:0")
    q = torch.from_numpy((g * g).sum(axis=1).astype(np.int32)).to("cuda:0")
    ref = to_lag(tri[("r2", "r").index(measure)], max_lag, fill=SENTINEL)
    m = hip_ctx.matrix_from_host(pack(G))
    try:
        for ld, off, row0, rows in ((max_lag + 2, 0, 0, n), (max_lag + 3, 1, 0, n), (max_lag + 2, 0, 66, 100)):
            counts = np.full((rows + 1, ld), SENTINEL, dtype=np.uint32)
            counts[:rows, :max_lag] = to_lag(P, max_lag, row0, rows, fill=SENTINEL)
            flat, view = device_buffer(rows + 1, ld, off)
            view[:counts.size].copy_(torch.from_numpy(counts.view(np.int32).ravel()))
            m.dosage_finish_lag_device(view.data_ptr(), ld, max_lag, s.data_ptr(), q.data_ptr(), S, measure, row0, rows)
            hip_ctx.synchronize()
            assert report(hip_ctx)[0] == RAN_SIMILARITY
            got = read_back(view, rows + 1, ld)
            assert (got[rows] == SENTINEL).all() and (got[:, max_lag:] == SENTINEL).all()
            assert np.array_equal(got[:rows, :max_lag], ref[row0:row0 + rows]), (ld, off, row0)
    finally:
        m.close()


# ------------------------------------------------------------------------------------------ 3. missing genotypes
@pytest.fixture(scope="module")
def missing300(lib):
    """300 variants x 1000 samples in the style of tests/test_gpu_dosage_complete.py's genotypes_with_missing: neighbours
    correlated, 5 % missing, and the special rows — all inside the shortest lag of their partner:
      3 complete; 40 all 3s; 60 / 61 share exactly sample 500 (N = 1); 62 = 1 except 2 on samples 0 - 99 and complete, 63
      missing exactly there: 62 is constant on what they share; 128 constant.
    The container, numpy's shared-sample counts and the n x n call's bits under both measures: once."""
    rng = np.random.default_rng(2026)
    n, S = 300, 1000
    G = np.zeros((n, S), dtype=np.uint8)
    for i in range(n):
        fresh = rng.binomial(2, rng.uniform(0.05, 0.5), size=S).astype(np.uint8)
        G[i] = np.where(rng.random(S) < 0.6, G[i - 1], fresh) if i and i % 10 else fresh
    G[128] = 1
    X = G.copy()
    X[rng.random((n, S)) < 0.05] = 3
    X[3] = G[3]
    X[40] = 3
    X[60], X[61] = np.where(np.arange(S) <= 500, G[60], 3), np.where(np.arange(S) >= 500, G[61], 3)
    X[62] = 1
    X[62, :100] = 2
    X[63, :100] = 3
    X[63, 100:] = np.where(G[63, 100:] == 1, 2, G[63, 100:])          # (row 63 itself is not constant on the shared part)
    X[63, 100], X[63, 101] = 0, 2
    N = complete_sums(X)[0]
    want, nan, _ = complete_reference(X)
    assert N[60, 61] == 1 and (N[40] == 0).all() and nan[62, 63] and nan[60, 61] and nan[40, 41] and not nan[62, 64] \
        and not nan[63, 64]
    d = Lag(lib, X)
    n_ = d.n
    tri = {measure: d.complete_host(measure)[:n_, :n_].copy() for measure in (0, 1)}
    yield d, X, N, tri, want, nan
    d.close()


@pytest.mark.parametrize("max_lag", [41, 42, 43, 85, 86, 299, 1000])
def test_missing_genotypes_nobs_and_corr_complete(missing300, max_lag):
    """lags at the edges of the interleaved layout (3 L + 2 = 125, 128, 131 and 257, 260 against the 128-row tile; the whole
    matrix; a clipped L). _lag_nobs equals numpy's shared-sample counts; _lag_corr_complete equals
    STORM_dosage_pairw_corr_complete bit for bit at the same pair, NaNs in the same places; host and device forms"""
    d, X, N, tri, want, nan = missing300
    n = d.n
    L = lag_of(n, max_lag)
    ok = lag_mask(n, L)
    nobs = d.both("nobs", max_lag)
    want_nobs = to_lag(np.triu(N, 1).astype(np.uint32), L)
    assert np.array_equal(nobs, want_nobs), (max_lag, np.argwhere(nobs != want_nobs)[:5].tolist())
    for measure in (0, 1):
        got = d.both("corr_complete", max_lag, measure)
        ref = to_lag(tri[measure], L)
        assert np.array_equal(got, ref), (measure, max_lag, np.argwhere(got != ref)[:5].tolist())
        assert np.array_equal((got == NAN_BITS) & ok, to_lag(nan, L, fill=False) & ok)
        assert got[62, 0] == NAN_BITS and got[60, 0] == NAN_BITS and got[40, 0] == NAN_BITS and got[39, 0] == NAN_BITS
        assert ((got != NAN_BITS) & ok).sum() > 0.9 * ok.sum()


def test_corr_complete_against_numpy(missing300):
    """once against the float64 value over the samples both rows have: at most 1 ulp (the bound of
    tests/test_gpu_dosage_complete.py, derived in tests/test_dosage_complete_math.py)"""
    d, X, N, tri, want, nan = missing300
    ok = lag_mask(d.n, 86) & ~to_lag(nan, 86, fill=True)
    for measure in (0, 1):
        got = d.lag("corr_complete", 86, measure, device=True)
        ref = to_lag(want[measure].astype(np.float32).view(np.uint32), 86)
        ulps = np.abs(ordered(got[ok]) - ordered(ref[ok]))
        print(f"measure {measure}: worst error {int(ulps.max())} ulp over {int(ok.sum())} entries")
        assert int(ulps.max()) <= 1


@pytest.mark.parametrize("max_lag", [42, 199])
def test_without_a_3_the_bits_are_lag_corr_s(corr200, max_lag):
    d, G, tri, _, _ = corr200
    ok = lag_mask(200, max_lag)
    for measure in (0, 1):
        a, b = d.both("corr_complete", max_lag, measure), d.both("corr", max_lag, measure)
        assert np.array_equal(a, b), (measure, np.argwhere(a != b)[:5].tolist())
    assert (d.both("nobs", max_lag)[ok] == 1000).all()


def test_scratch_grows_with_n_times_lag_not_with_n_squared(lib):
    """4096 rows x 2048 samples, lag 64: device memory in use (hipMemGetInfo) before and after the first pairwise-complete
    lag call of the process on such rows — upload, interleaved operand (3 n rows), sums (3 n x 196 uint32), work list — grows
    by less than ONE 4096 x 4096 uint32 matrix; the n x n call keeps three of those. Eight rows are checked against numpy."""
    import torch
    n, S, max_lag = 4096, 2048, 64
    rng = np.random.default_rng(4096)
    X = rng.integers(0, 3, size=(n, S), dtype=np.uint8)
    X[rng.random((n, S)) < 0.05] = 3
    small = Lag(lib, X[:4])
    small.lag("corr_complete", 2, 0, device=True)            # the containers' context and its fixed buffers exist
    small.close()
    d = Lag(lib, X, packed_only=True)
    try:
        out = torch.full((n, max_lag), -1, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        free_before = torch.cuda.mem_get_info()[0]
        d.ok(lib.STORM_dosage_pairw_lag_corr_complete_device(d.h, 0, max_lag, C.c_void_p(out.data_ptr()), n, max_lag), "complete")
        free_after = torch.cuda.mem_get_info()[0]
        grown = free_before - free_after
        print(f"device memory grown by {grown / 2**20:.1f} MiB (one n x n uint32 matrix: {n * n * 4 / 2**20:.0f} MiB)")
        assert grown < n * n * 4
        got = out.cpu().numpy().view(np.uint32)
        for i in (0, 1, 127, 128, 2047, 4000, 4031, 4094):
            rows = X[i:min(n, i + 1 + max_lag)]
            want, nan, _ = complete_reference(rows)
            k = rows.shape[0] - 1
            ref = want[0][0, 1:].astype(np.float32).view(np.uint32)
            ok = ~nan[0, 1:]
            assert ok.all() and np.abs(ordered(got[i, :k]) - ordered(ref)).max() <= 1, i
            assert (got[i, k:] == 0xFFFFFFFF).all()                                         # the corner stays
    finally:
        d.close()


# ------------------------------------------------------------------------------------------ 4. the shim's refusals
def test_shim_refusals_and_empty_shapes(hip_ctx, lib):
    G = np.random.default_rng(5).integers(0, 4, size=(20, 100), dtype=np.uint8)
    m = hip_ctx.matrix_from_host(pack(G))
    one = hip_ctx.matrix_from_host(pack(G[:1]))
    flat, view = device_buffer(21, 32)
    p, c, mh, oh = C.c_void_p(view.data_ptr()), hip_ctx._h, m._h, one._h
    try:
        f = lib.storm_hip_pairw_lag_dosage_matrix_device
        assert f(c, mh, 0, 0, 20, p, 32) == -1 and f(c, mh, 5, 0, 20, p, 4) == -1 and f(c, mh, 5, 0, 20, None, 32) == -1
        assert f(c, mh, 5, 21, 0, p, 32) == -1 and f(c, mh, 5, 10, 11, p, 32) == -1 and b"band" in lib.storm_hip_last_error()
        assert f(c, mh, 5, 20, 0, p, 32) == 0 and f(c, oh, 5, 0, 1, p, 32) == 0              # an empty band; one row
        for name in ("corr", "corr_complete"):
            f = getattr(lib, f"storm_hip_pairw_lag_dosage_{name}_device")
            assert f(c, mh, 2, 100, 5, p, 32) == -1 and b"measure" in lib.storm_hip_last_error()
            assert f(c, mh, 0, 64, 5, p, 32) == -1 and f(c, mh, 0, 129, 5, p, 32) == -1      # n_samples against the row width
            assert f(c, mh, 0, 100, 0, p, 32) == -1 and f(c, mh, 0, 100, 30, p, 18) == -1    # max_lag 0; ld < L = 19
            assert f(c, oh, 0, 100, 5, p, 32) == 0
        f = lib.storm_hip_pairw_lag_dosage_nobs_device
        assert f(c, mh, 0, 5, p, 32) == -1 and f(c, mh, 100, 0, p, 32) == -1 and f(c, mh, 100, 5, p, 4) == -1
        assert f(c, oh, 100, 5, p, 32) == 0
        f = lib.storm_hip_dosage_finish_lag_device
        assert f(c, p, 32, 20, 0, 20, 5, None, p, 0, 100) == -1 and f(c, p, 32, 20, 0, 20, 5, p, p, 2, 100) == -1
        assert f(c, p, 32, 20, 0, 20, 5, p, p, 0, 0) == -1 and f(c, p, 32, 20, 15, 6, 5, p, p, 0, 100) == -1
        assert f(c, p, 4, 20, 0, 20, 5, p, p, 0, 100) == -1 and f(c, p, 32, 20, 0, 20, 0, p, p, 0, 100) == -1
        hip_ctx.synchronize()
        assert (read_back(view, 21, 32) == SENTINEL).all()                                 # nothing above wrote anything
        # the report of a whole call: the pairs within the lag x n_words, K2h on 2-bit values
        assert lib.storm_hip_pairw_lag_dosage_corr_device(c, mh, 1, 100, 5, p, 32) == 0
        assert report(hip_ctx)[:2] == [RAN_TILES_OUT | RAN_SIMILARITY, int(lag_mask(20, 5).sum()) * m.n_words]
        assert hip_ctx.get_option("k2_tile_shape_used") == 7
        assert lib.storm_hip_pairw_lag_dosage_nobs_device(c, mh, 100, 5, p, 32) == 0
        assert report(hip_ctx)[:2] == [RAN_TILES_OUT, int(lag_mask(20, 5).sum()) * m.n_words]
        assert lib.storm_hip_pairw_lag_dosage_corr_complete_device(c, mh, 1, 100, 5, p, 32) == 0
        assert report(hip_ctx)[:2] == [RAN_TILES_OUT | RAN_SIMILARITY, int(lag_mask(60, 17).sum()) * m.n_words]
    finally:
        m.close()
        one.close()


# ------------------------------------------------------------------------------------------ 5. Python
def test_python_class_end_to_end():
    import torch
    n, S, max_lag = 129, 257, 50
    rng = np.random.default_rng(11)
    X = rng.integers(0, 3, size=(n, S), dtype=np.uint8)
    X[rng.random((n, S)) < 0.1] = 3
    X[5] = 3
    d = sb.StormDosage(S)
    for i in range(64):
        d.add(X[i])
    d.add_packed(pack(X[64:]))
    x = X.astype(np.int64)
    ok = lag_mask(n, max_lag)
    dot = d.pairw_lag_dot(max_lag)
    assert dot.dtype == np.uint32 and dot.shape == (n, max_lag)
    assert np.array_equal(dot, to_lag(np.triu(x @ x.T, 1).astype(np.uint32), max_lag))      # 3 is a value here
    assert d.pairw_lag_dot(1000).shape == (n, n - 1)
    t = torch.full((n + 2, max_lag + 4), -1, dtype=torch.int32, device="cuda:0")
    assert d.pairw_lag_dot(max_lag, device=t) is None
    t = t.cpu().numpy()
    assert np.array_equal(t[:n, :max_lag][ok], dot[ok]) and (t[:n, :max_lag][~ok] == -1).all() and (t[n:] == -1).all() and \
        (t[:, max_lag:] == -1).all()
    nobs = d.pairw_lag_nobs(max_lag)
    assert nobs.dtype == np.uint32 and np.array_equal(nobs, to_lag(np.triu(complete_sums(X)[0], 1).astype(np.uint32), max_lag))
    for measure in ("r2", "r"):
        r = d.pairw_lag_corr(max_lag, measure)
        assert r.dtype == np.float32 and np.array_equal(r.view(np.uint32), to_lag(d.pairw_corr(measure).view(np.uint32), max_lag))
        rc = d.pairw_lag_corr_complete(max_lag, measure)
        assert rc.dtype == np.float32
        assert np.array_equal(rc.view(np.uint32), to_lag(d.pairw_corr_complete(measure).view(np.uint32), max_lag))
        assert np.isnan(rc[5, :]).all() and np.isnan(rc[4, 0]) and (rc[~ok] == 0).all() and (~np.isnan(rc[ok])).sum() > 0.9 * ok.sum()
        f = torch.full((n, max_lag + 1), -7.5, dtype=torch.float32, device="cuda:0")
        assert d.pairw_lag_corr_complete(max_lag, measure, device=f) is None
        f = f.cpu().numpy()
        assert np.array_equal(f[:, :max_lag].view(np.uint32)[ok], rc.view(np.uint32)[ok]) and (f[:, :max_lag][~ok] == -7.5).all() \
            and (f[:, max_lag] == -7.5).all()
    with pytest.raises(RuntimeError):
        d.pairw_lag_dot(0)
    d.free()
