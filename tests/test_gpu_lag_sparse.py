"""The sparse LD report compacted on the device (storm.h: STORM_dosage_lag_corr_sparse, _complete and their _device forms;
storm_hip.h: storm_hip_lag_band_sparse_device): lag_band_sparse_count_kernel, the three launches of the scan and
lag_band_sparse_fill_kernel over a band in the lag layout. Everything goes through the C-ABI (HipContext.lag_band_sparse_device,
StormDosage.lag_corr_sparse, ctypes).

The answer is unique — the CSR list of the forward pairs whose float exceeds the threshold, in (i, j) order — so row_start and
col are compared EXACTLY, and val as 32-bit patterns, with the plain numpy of tests/_lag_sparse.py: over hand-made bands (NaN,
both zeros against thresholds of both zeros, a value at the threshold and the next float above it, +inf, a poisoned corner and
pitch, rows wholly listed and wholly empty, windows on both sides and on one), over counts laid out around the scan's block
boundaries, over a band whose last row starts beyond 2^32 elements, and over the library's own pairw_lag_corr[_complete] device
matrix of rows with real LD, where every case first shows that its reference lists something and not everything."""
import ctypes as C

import numpy as np
import pytest

import stormbitmaps_amd as sb
from tests import _lag_sparse, _prune
from tests.test_gpu_dosage import pack
# the fixtures (one instance per importing module) of the stream tests: Streams, Held and the backlog of Switching
from tests.test_gpu_streams import born, held, st, sw_module  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD = 5                                                                          # elements behind the end of a device output
ROWS_SENTINEL = -7
T = np.float32(0.5)
HIGH, LOW = np.float32(0.9), np.float32(0.1)
POISON = np.float32(1.0)                                                           # above every threshold used here
SCAN_ROWS = 1024                                                                   # storm_lag_sparse_math.h: kSparseScanRows


def device_list(call, n, capacity):
    """(row_start, col, val bits) of a _device form: `call(d_rows, d_col, d_val, capacity)` with sentinels in row_start, 0xFF
    bytes in col / val and GUARD elements behind n + 1 and behind `capacity`, all checked. capacity None: the offsets alone"""
    import torch
    d_rows = torch.full((n + 1 + GUARD,), ROWS_SENTINEL, dtype=torch.int64, device="cuda:0")
    cap = 0 if capacity is None else capacity
    d_col = torch.full((cap + GUARD,), -1, dtype=torch.int32, device="cuda:0")
    d_val = torch.full((cap + GUARD,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()                                                       # the guards are in place before the call's stream runs
    # (views of exactly `capacity` elements: a wrapper that takes the capacity from the tensors' length gets the right one)
    call(d_rows, None if capacity is None else d_col[:cap], None if capacity is None else d_val[:cap], cap)
    torch.cuda.synchronize()
    rows, col, val = d_rows.cpu().numpy(), d_col.cpu().numpy().view(np.uint32), d_val.cpu().numpy().view(np.uint32)
    assert (rows[n + 1:] == ROWS_SENTINEL).all()
    rows = rows[:n + 1].view(np.uint64)
    written = min(int(rows[n]), cap)
    assert (col[written:] == 0xFFFFFFFF).all() and (val[written:] == 0xFFFFFFFF).all()   # nothing at or behind min(total, capacity)
    return rows, col[:written], val[:written]


def band_sparse(ctx, d_vals, ld, n, max_lag, min_r2, lo=None, hi=None, capacity=None):
    return device_list(lambda r, c, v, cap: ctx.lag_band_sparse_device(
        d_vals.data_ptr(), ld, n, max_lag, float(min_r2), r.data_ptr(), None if c is None else c.data_ptr(),
        None if v is None else v.data_ptr(), cap, lo, hi), n, capacity)


def assert_same_list(got, want, where, written=None):
    rows, col, val = got
    w_rows, w_col, w_val = want
    assert np.array_equal(rows, w_rows), (where, np.flatnonzero(rows != w_rows)[:8].tolist())
    k = w_col.size if written is None else written
    assert col.size == k and np.array_equal(col, w_col[:k]), where
    assert np.array_equal(val, w_val[:k].view(np.uint32)), where


# ---- the generic entry over hand-made bands ---------------------------------------------------------------------------------
VALUES = np.float32([np.nan, 0.0, -0.0, T, np.nextafter(T, np.float32(1)), np.inf, LOW, HIGH, np.nextafter(T, np.float32(0))])


def make_band(n, max_lag, seed):
    """[n, L + 3] float32 of the values where a comparison can go wrong; one row wholly HIGH, one wholly LOW; the lower-right
    corner and the pitch columns at POISON, which must never be listed"""
    rng = np.random.default_rng(seed)
    L = min(max_lag, n - 1)
    band = np.full((n, L + 3), POISON, dtype=np.float32)
    band[:, :L] = rng.choice(VALUES, size=(n, L))
    band[0, :L] = HIGH                                                             # a row entirely listed: count = L
    if n > 2:
        band[n // 2, :L] = LOW                                                     # ... and one with nothing listed
    inside = (np.arange(n)[:, None] + 1 + np.arange(L)[None, :]) < n
    band[:, :L] = np.where(inside, band[:, :L], POISON)
    return band, L


@pytest.mark.parametrize("n", [2, 63, 64, 65, 129, 257])
def test_hand_made_bands_through_the_band_call(hip_ctx, n):
    import torch
    rng = np.random.default_rng(n)
    pos = np.cumsum(rng.integers(1, 5, size=n)).astype(np.float64)
    lo, hi, _ = _prune.window_bounds(pos, 9.0)
    everything_behind, everything_ahead = np.zeros(n, np.uint32), np.full(n, n - 1, np.uint32)
    windows = ((None, None), (lo, hi), (everything_behind, hi), (lo, everything_ahead))   # both sides, ahead only, behind only
    for max_lag in (1, 31, 32, 33, 63, 64, 65, 129, n - 1, n + 5):
        if max_lag == 0:
            continue
        band, L = make_band(n, max_lag, 1000 * n + max_lag)
        d_vals = torch.from_numpy(band).to("cuda:0")
        for min_r2, wins in ((T, windows), (np.float32(0.0), windows[:1]), (np.float32(-0.0), windows[:1]),
                             (np.float32(-1.0), windows[:2]), (np.float32(np.inf), windows[:1])):
            for w in wins:
                where = (n, max_lag, float(min_r2), w[0] is not None)
                want = _lag_sparse.sparse_list(band, n, max_lag, min_r2, *w)
                total = int(want[0][n])
                assert (want[1] < n).all()                                         # (the reference itself lists no corner entry)
                if w[0] is None and min_r2 == T:
                    assert int(want[0][1]) == L                                    # row 0 is wholly listed
                    if n > 2:
                        assert want[0][n // 2] == want[0][n // 2 + 1]              # row n / 2 not at all
                if min_r2 == np.inf:
                    assert total == 0                                              # a whole band with nothing listed
                got = band_sparse(hip_ctx, d_vals, L + 3, n, max_lag, min_r2, *w, capacity=total)
                assert_same_list(got, want, where)
                only = band_sparse(hip_ctx, d_vals, L + 3, n, max_lag, min_r2, *w)   # count-only: the same offsets
                assert np.array_equal(only[0], want[0]), where
        again = band_sparse(hip_ctx, d_vals, L + 3, n, max_lag, T, lo, hi, capacity=n * L)
        twice = band_sparse(hip_ctx, d_vals, L + 3, n, max_lag, T, lo, hi, capacity=n * L)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, twice))        # two calls, the same bytes


def test_the_values_at_the_threshold_one_by_one(hip_ctx):
    """one row against the next nine, each of VALUES once: what is listed under thresholds of 0.5, +0.0, -0.0 and -1"""
    import torch
    n = VALUES.size + 1
    band = np.full((n, n + 1), POISON, dtype=np.float32)
    band[0, :n - 1] = VALUES
    band[1:, :n - 1] = np.nan
    d_vals = torch.from_numpy(band).to("cuda:0")
    up = np.nextafter(T, np.float32(1))
    down = np.nextafter(T, np.float32(0))
    for min_r2, listed in ((T, [up, np.inf, HIGH]), (np.float32(0.0), [T, up, np.inf, LOW, HIGH, down]),
                           (np.float32(-0.0), [T, up, np.inf, LOW, HIGH, down]),
                           (np.float32(-1.0), [v for v in VALUES if not np.isnan(v)])):
        rows, col, val = band_sparse(hip_ctx, d_vals, n + 1, n, n, min_r2, capacity=n)
        assert rows.tolist() == [0] + [len(listed)] * n
        assert sorted(val.tolist()) == sorted(np.float32(listed).view(np.uint32).tolist())   # -0.0 and +0.0 by their own bits
        assert np.array_equal(val, band[0, col.astype(np.int64) - 1].view(np.uint32))
        assert_same_list((rows, col, val), _lag_sparse.sparse_list(band, n, n, min_r2), float(min_r2))


def test_the_band_call_refuses(hip_ctx):
    import torch
    n, L = 40, 7
    band, _ = make_band(n, L, 5)
    d_vals = torch.from_numpy(band).to("cuda:0")
    d_rows = torch.full((n + 1,), ROWS_SENTINEL, dtype=torch.int64, device="cuda:0")
    d_col = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    d_val = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    v, r, c, x = d_vals.data_ptr(), d_rows.data_ptr(), d_col.data_ptr(), d_val.data_ptr()
    ones = np.ones(n, np.uint32)
    for args, kw, word in (((None, L + 3, n, L, 0.5, r, c, x, n), {}, "NULL"), ((v, L + 3, n, L, 0.5, None, c, x, n), {}, "NULL"),
                           ((v, L + 3, n, 0, 0.5, r, c, x, n), {}, "max_lag"), ((v, L - 1, n, L, 0.5, r, c, x, n), {}, "leading dimension"),
                           ((v, L + 3, n, L, 0.5, r, c, x, n), {"lo": ones}, "lo and hi"), ((v, L + 3, n, L, 0.5, r, c, x, n), {"hi": ones}, "lo and hi"),
                           ((v, L + 3, n, L, 0.5, r, c, None, n), {}, "col and val"), ((v, L + 3, n, L, 0.5, r, None, x, n), {}, "col and val"),
                           ((v, L + 3, n, L, 0.5, r, None, None, n), {}, "capacity"), ((v, L + 3, n, L, float("nan"), r, c, x, n), {}, "NaN")):
        with pytest.raises(RuntimeError, match=word):
            hip_ctx.lag_band_sparse_device(*args, **kw)
    torch.cuda.synchronize()
    assert (d_rows.cpu().numpy() == ROWS_SENTINEL).all() and (d_col.cpu().numpy() == -1).all() and (d_val.cpu().numpy() == -1).all()
    for rows in (0, 1):                                                            # fewer than two rows: rows + 1 zeros, no list
        d_rows.fill_(ROWS_SENTINEL)
        hip_ctx.lag_band_sparse_device(v, L + 3, rows, L, 0.5, r, c, x, n)
        assert d_rows.cpu().tolist() == [0] * (rows + 1) + [ROWS_SENTINEL] * (n - rows)
    assert (d_col.cpu().numpy() == -1).all() and (d_val.cpu().numpy() == -1).all()


# ---- the scan's block boundaries and 64-bit indexing ------------------------------------------------------------------------
def pattern_band(torch, n, ld):
    """a band of lag 2 whose row i lists i % 3 pairs (0 / 1 / 2, fewer where the matrix ends): only the two live columns
    are ever written"""
    d_vals = torch.empty((n, ld), dtype=torch.float32, device="cuda:0")
    i = torch.arange(n, device="cuda:0")
    d_vals[:, 0] = torch.where(i % 3 >= 1, float(HIGH), float(LOW))
    d_vals[:, 1] = torch.where(i % 3 == 2, float(HIGH), float(LOW))
    counts = np.minimum(np.arange(n) % 3, np.maximum(n - 1 - np.arange(n), 0))
    return d_vals, counts


@pytest.mark.parametrize("n", [SCAN_ROWS - 1, SCAN_ROWS, SCAN_ROWS + 1, 2 * SCAN_ROWS - 1, 2 * SCAN_ROWS, 2 * SCAN_ROWS + 1, 70001])
def test_offsets_around_the_scans_block_boundaries(hip_ctx, n):
    import torch
    d_vals, counts = pattern_band(torch, n, 3)
    want_rows = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    rows, _, _ = band_sparse(hip_ctx, d_vals, 3, n, 2, T)
    assert np.array_equal(rows, want_rows), np.flatnonzero(rows != want_rows)[:8].tolist()
    total = int(want_rows[n])
    rows, col, val = band_sparse(hip_ctx, d_vals, 3, n, 2, T, capacity=total)
    assert np.array_equal(rows, want_rows)
    want_col = np.concatenate([np.arange(i + 1, i + 1 + c) for i, c in enumerate(counts.tolist())]).astype(np.uint32)
    assert np.array_equal(col, want_col) and (val == HIGH.view(np.uint32)).all()


def test_a_band_whose_last_row_starts_beyond_2_to_the_32_elements(hip_ctx):
    import torch
    n, ld = 70001, 65537
    assert (n - 1) * ld > 1 << 32
    torch.cuda.synchronize()
    if torch.cuda.mem_get_info()[0] < 40e9:
        pytest.skip("needs 40 GB of free device memory for an 18 GB band")
    try:
        d_vals, counts = pattern_band(torch, n, ld)
        want_rows = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        total = int(want_rows[n])
        rows, col, val = band_sparse(hip_ctx, d_vals, ld, n, 2, T, capacity=total)
        assert np.array_equal(rows, want_rows), np.flatnonzero(rows != want_rows)[:8].tolist()
        want_col = np.concatenate([np.arange(i + 1, i + 1 + c) for i, c in enumerate(counts.tolist())]).astype(np.uint32)
        assert np.array_equal(col, want_col) and (val == HIGH.view(np.uint32)).all()
        assert col[-1] == n - 1 and col[-2] == n - 2                               # rows n - 3 and n - 2: beyond 2^32 elements
    finally:
        d_vals = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ---- capacity ---------------------------------------------------------------------------------------------------------------
def test_a_capacity_below_the_total_writes_the_first_pairs_and_nothing_behind_them(hip_ctx):
    import torch
    n, max_lag = 257, 65
    band, L = make_band(n, max_lag, 99)
    d_vals = torch.from_numpy(band).to("cuda:0")
    want = _lag_sparse.sparse_list(band, n, max_lag, T)
    total = int(want[0][n])
    assert total > 300
    for capacity in (total, total - 1, 1, total + 7):
        got = band_sparse(hip_ctx, d_vals, L + 3, n, max_lag, T, capacity=capacity)    # (device_list checks the 0xFF behind it)
        assert_same_list(got, want, capacity, written=min(capacity, total))


# ---- containers: rows with real LD through StormDosage.lag_corr_sparse -----------------------------------------------------
SHAPES = [(300, 64), (1000, 200), (4200, 128)]
LAGS = {7: 6.0, 64: 40.0, 200: 150.0}                                              # max_lag -> a max_dist its windows fit in


def bounds(pos, max_dist):
    """_prune.window_bounds for many rows (the same definition by bisection)"""
    lo = np.searchsorted(pos, pos - max_dist, side="left").astype(np.uint32)
    hi = (np.searchsorted(pos, pos + max_dist, side="right") - 1).astype(np.uint32)
    return lo, hi


class Case:
    """one container per (shape, kind), its positions, and per lag the library's own band of r^2 from the existing _device corr
    call: fetched once, never modified"""

    def __init__(self, n, S, kind):
        self.n, self.S, self.kind, self.complete = n, S, kind, kind == "missing"
        self.G = _prune.ld_rows(n, S, 100 * n + S, missing=0.05 if self.complete else 0.0)
        self.d = sb.StormDosage(S)
        for row in self.G:
            self.d.add(row)
        self.pos = np.cumsum(np.random.default_rng(n).integers(1, 5, size=n)).astype(np.float64)
        self._bands = {}

    def band(self, max_lag):
        import torch
        if max_lag not in self._bands:
            L = min(max_lag, self.n - 1)
            out = torch.full((self.n, L + 2), float(POISON), dtype=torch.float32, device="cuda:0")
            (self.d.pairw_lag_corr_complete if self.complete else self.d.pairw_lag_corr)(max_lag, "r2", device=out)
            torch.cuda.synchronize()
            band = out.cpu().numpy()
            band.setflags(write=False)
            self._bands[max_lag] = band
        return self._bands[max_lag]


_cases = {}


def case_of(n, S, kind):
    if (n, S, kind) not in _cases:
        _cases[n, S, kind] = Case(n, S, kind)
    return _cases[n, S, kind]


def container_device(case, min_r2, capacity, **kw):
    return device_list(lambda r, c, v, cap: case.d.lag_corr_sparse(min_r2, complete=case.complete, device=(r, c, v), **kw),
                       case.n, capacity)


@pytest.mark.parametrize("kind", ["plain", "missing"])
@pytest.mark.parametrize("n,S", SHAPES)
def test_containers_against_the_list_of_the_librarys_own_band(n, S, kind):
    case = case_of(n, S, kind)
    assert _prune.window_bounds(case.pos[:200], 6.0)[0].tolist() == bounds(case.pos[:200], 6.0)[0].tolist()
    assert _prune.window_bounds(case.pos[:200], 6.0)[1].tolist() == bounds(case.pos[:200], 6.0)[1].tolist()
    for max_lag, max_dist in LAGS.items():
        band, L = case.band(max_lag), min(max_lag, n - 1)
        for with_pos in (False, True):
            kw = {"max_lag": max_lag, "pos": case.pos, "max_dist": max_dist} if with_pos else {"max_lag": max_lag}
            lo, hi = bounds(case.pos, max_dist) if with_pos else (None, None)
            for min_r2 in (0.2, 0.5):
                where = (n, S, kind, max_lag, with_pos, min_r2)
                want = _lag_sparse.sparse_list(band, n, max_lag, np.float32(min_r2), lo, hi)
                total = int(want[0][n])
                print(f"{where}: {total} of {n * L} entries listed")
                assert 0 < total < n * L, (where, total)                           # neither nothing nor everything passes
                got = case.d.lag_corr_sparse(min_r2, complete=case.complete, **kw)     # count-only, then the exact fill
                assert got[0].dtype == np.uint64 and got[1].dtype == np.uint32 and got[2].dtype == np.float32
                assert_same_list((got[0], got[1], got[2].view(np.uint32)), want, where)
                roomy = case.d.lag_corr_sparse(min_r2, complete=case.complete, capacity=total + 11, **kw)   # one call
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, roomy)), where   # two calls, the same bytes
                dev = container_device(case, min_r2, total, **kw)
                assert_same_list(dev, want, where + ("device",))                   # host and _device forms agree
                only = container_device(case, min_r2, None, **kw)
                assert np.array_equal(only[0], want[0]), where                     # count-only: the same row_start
                with pytest.raises(RuntimeError, match=f"{total} pairs are listed, capacity is {total - 1}"):
                    case.d.lag_corr_sparse(min_r2, complete=case.complete, capacity=total - 1, **kw)
            if with_pos:                                                           # max_lag None: the lag the windows need
                got = case.d.lag_corr_sparse(0.2, complete=case.complete, pos=case.pos, max_dist=max_dist)
                want = _lag_sparse.sparse_list(band, n, max_lag, np.float32(0.2), lo, hi)
                assert_same_list((got[0], got[1], got[2].view(np.uint32)), want, (n, S, kind, "the windows' own lag"))


def test_capacity_of_the_container_forms(lib):
    """the _device form writes the first `capacity` pairs and keeps the true offsets; the host form returns -4 with the offsets
    and the total for the same rows"""
    case = case_of(300, 64, "plain")
    max_lag, min_r2 = 64, 0.2
    want = _lag_sparse.sparse_list(case.band(max_lag), case.n, max_lag, np.float32(min_r2))
    total, n = int(want[0][case.n]), case.n
    for capacity in (total, total - 1, 1):
        got = container_device(case, min_r2, capacity, max_lag=max_lag)
        assert_same_list(got, want, capacity, written=capacity)
    for capacity in (total - 1, 1, 0):
        rows = np.full(n + 1, 0x77, dtype=np.uint64)
        col, val = np.zeros(total, dtype=np.uint32), np.zeros(total, dtype=np.float32)
        n_pairs = C.c_uint64(12345)
        rc = lib.STORM_dosage_lag_corr_sparse(case.d._h, min_r2, max_lag, None, 0.0, rows.ctypes.data, n + 1, col.ctypes.data,
                                              val.ctypes.data, capacity, C.byref(n_pairs))
        assert rc == -4 and n_pairs.value == total and np.array_equal(rows, want[0]), capacity
        assert f"{total} pairs are listed, capacity is {capacity}".encode() in lib.STORM_hip_error()
    # one row fewer than the windows need: refused, never clipped, nothing written
    lo, hi, need = _prune.window_bounds(case.pos, 12.0)
    rows = np.full(n + 1, 0x77, dtype=np.uint64)
    n_pairs = C.c_uint64(12345)
    for name in ("STORM_dosage_lag_corr_sparse", "STORM_dosage_lag_corr_sparse_complete"):
        assert getattr(lib, name)(case.d._h, min_r2, need - 1, case.pos.ctypes.data, 12.0, rows.ctypes.data, n + 1, None, None, 0,
                                  C.byref(n_pairs)) == -3
        assert f"lag of {need} rows, max_lag is {need - 1}".encode() in lib.STORM_hip_error()
    assert (rows == 0x77).all() and n_pairs.value == 12345
    got = case.d.lag_corr_sparse(min_r2, need, pos=case.pos, max_dist=12.0)        # exactly what the windows need
    want = _lag_sparse.sparse_list(case.band(max_lag), n, need, np.float32(min_r2), lo, hi)
    assert_same_list((got[0], got[1], got[2].view(np.uint32)), want, "need")


def test_small_containers_on_the_device():
    import torch
    d = sb.StormDosage(40)
    for n in (0, 1):
        for complete in (False, True):
            d_rows = torch.full((4,), ROWS_SENTINEL, dtype=torch.int64, device="cuda:0")
            d_col = torch.full((3,), -1, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            d.lag_corr_sparse(0.2, 3, complete=complete, device=(d_rows, d_col, d_col.clone()))
            torch.cuda.synchronize()
            assert d_rows.cpu().tolist() == [0] * (n + 1) + [ROWS_SENTINEL] * (3 - n) and (d_col.cpu().numpy() == -1).all()
            rows, col, val = d.lag_corr_sparse(0.2, 3, complete=complete)
            assert rows.tolist() == [0] * (n + 1) and col.size == 0 and val.size == 0
        d.add(np.arange(40, dtype=np.uint8) % 3)


def test_every_removed_rows_owner_is_its_neighbour_in_the_list():
    case = case_of(1000, 200, "plain")
    max_lag, min_r2 = 64, 0.2
    keep, owner = case.d.lag_prune(min_r2, max_lag, owner=True)
    rows, col, _ = case.d.lag_corr_sparse(min_r2, max_lag)
    nb = _lag_sparse.symmetrised(rows, col, case.n)
    removed = np.flatnonzero(keep == 0)
    assert 0 < removed.size < case.n
    for v in removed.tolist():
        assert int(owner[v]) in nb[v] and keep[owner[v]] == 1, v
    for v in np.flatnonzero(keep == 1).tolist():
        assert not any(keep[j] for j in nb[v]), v                                  # no two kept rows are adjacent in the list


# ---- a caller's stream -------------------------------------------------------------------------------------------------------
def test_the_shim_device_form_only_enqueues_on_a_callers_stream(born, held, st, sw_module):
    """as tests/test_gpu_streams_ld.py: a context born on s1; the call once on DECOY rows of the same shape (buffers grown, the
    work list cached, foreign data in the scratch); a backlog on s1; then, with no host wait, sentinel fills by torch, the
    call without positions through ctypes and clones of its outputs. The clones after s1 has run and the originals after the
    caller's own synchronise hold the list of the real rows: a step on another stream or a missing order would leave sentinels
    or the decoy's list"""
    torch = st.torch
    n, S, lag, min_r2 = 300, 96, 70, 0.2
    x = _prune.ld_rows(n, S, seed=n)
    m = held.matrix(born, pack(x.astype(np.int64)))
    decoy = held.matrix(born, pack(np.random.default_rng(1000 + n).integers(0, 3, size=(n, S))))
    band = m.pairw_lag_dosage_corr(lag, S, "r2")                                   # (complete on return: tests/test_gpu_streams_ld.py)
    want = _lag_sparse.sparse_list(band, n, lag, np.float32(min_r2))
    total = int(want[0][n])
    assert 0 < total < n * lag
    cap = total + GUARD

    def outputs():
        return (st.full(st.s1, (n + 1 + GUARD,), ROWS_SENTINEL, torch.int64), st.full(st.s1, (cap,), -1, torch.int32),
                st.full(st.s1, (cap,), -1, torch.int32))

    def enqueue(matrix, out):
        sb._lib.check(born._lib.storm_hip_lag_dosage_corr_sparse_device(
            born._h, matrix._h, S, lag, min_r2, None, None, C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()),
            C.c_void_p(out[2].data_ptr()), cap), "storm_hip_lag_dosage_corr_sparse_device")

    def check(tensors, what):
        rows, col, val = (st.read(t) for t in tensors)
        assert (rows[n + 1:] == ROWS_SENTINEL).all() and (col[total:] == -1).all() and (val[total:] == -1).all(), what
        assert_same_list((rows[:n + 1].view(np.uint64), col[:total].view(np.uint32), val[:total].view(np.uint32)), want, what)

    with torch.cuda.stream(st.s1):
        enqueue(decoy, outputs())
    st.drain()
    sw_module.backlog()
    with torch.cuda.stream(st.s1):
        out = outputs()
        enqueue(m, out)
        snap = [t.clone() for t in out]
    st.s1.synchronize()                                                            # the caller's own synchronise
    check(snap, "snapshot")
    check(out, "outputs")
    st.drain()
    got = m.lag_dosage_corr_sparse(min_r2, lag, S)                                 # the host form on the caller's stream
    assert_same_list((got[0], got[1], got[2].view(np.uint32)), want, "host form")
