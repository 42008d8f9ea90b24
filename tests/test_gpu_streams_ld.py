"""The lag-dosage, LD-score and pruning calls on a caller's stream and across storm_hip_ctx_set_stream (the stream contract of
include/storm_hip.h, continued from tests/test_gpu_streams.py, whose streams, sentinels, backlog and fixtures this file
imports).

What is pinned: storm_hip_pairw_lag_dosage_*_device (and the three dosage calls the older file left out) are COMPLETE ON
RETURN; storm_hip_dosage_finish_lag_device, the three storm_hip_lag_band_* primitives and the _device forms of
storm_hip_lag_dosage_ldscore / _ldscore_annot / _prune [_complete] ONLY ENQUEUE, keep reading the caller's host arrays
(h_lo, h_hi, h_order) until the stream has run, and share the context's band buffer, split rows, sums matrix, tickets and
cached work list in stream order — also across storm_hip_ctx_set_stream. The queued calls go through ctypes: the Python
wrappers of three of them wait on their own.

Inputs: tests/_prune.ld_rows(n, S, seed=n) for (n, S) = (300, 96) and (513, 4128) — 3 and 129 words — without missing calls
for the complete-case forms and with a tenth missing for the pairwise-complete ones; max_lag 70, output pitch 72; min_r2 0.2
and 0.5; random priorities, windows of distance 9 over steps of 1 .. 4, 65 annotation columns (device pitch 70 with NaN in
the pitch columns, score pitch 68).

References, in two steps; no result of the library is ever its own reference, and no bound is new:
  1. what the complete-on-return lag forms write against numpy in float64 (_check_correlation and _complete_reference of
     tests/test_gpu_streams.py on the lag layout): dot products and N equal, r and r^2 the one NaN exactly where a
     denominator is 0 and elsewhere within 1 float32 ulp; pitch columns and the lower-right corner keep the sentinel;
  2. over that checked band, on the host: tests/_ldscore.band_sums and tests/_ldscore_annot.annot_sums with their
     assert_scores (counts equal, scores within the derived bound), tests/_prune.neighbours + greedy (keep and owner equal;
     and equal to the greedy over the float64 r^2, whose kept share lies in [0.15, 0.75], which differs from the one-round
     rule on at least 2 rows, and which has no r^2 within 2^-20 relative of min_r2);
  3. a composite _device form must return the bits of the matching storm_hip_lag_band_* primitive run over the band of 1;
  4. and the bits of the same call's host form on a context of the NULL stream (made when the first result is compared).
`Checked` holds 1 and computes 2 - 4 once per (shape, rows, arguments); every scenario compares bytes with it.

A queued call can only show a missing order if it does not wait on its own. It waits (for its stream) when it plans and
uploads a work list — the context caches ONE list, keyed by rows, lag and form — or grows a buffer. So every scenario first
runs the same calls once on DECOY rows of the same shape (random values without LD: their band, masks and keep differ),
which leaves the list of the call under test cached, the buffers grown and foreign data in all shared scratch; then come
the backlog of tests/test_gpu_streams.py on s1 (BACKLOG_PASSES passes, 8 - 9 ms of device time, measured there against
host sequences of 0.1 ms) and the calls. A step on stream 0, a missing wait or scratch not ordered across set_stream is
then a sentinel, a decoy's answer or a mixture: a wrong answer, never a wait: none of these kernels polls another workgroup.
Measured once on one MI355X for the sequences of (b) — the outputs' sentinel fills (and the annotations) by torch, the call,
the clones — lists cached, buffers grown, 3 repeats of 5 calls x 2 shapes x 2 kinds of rows: 0.06 - 0.11 ms of host time
(perf_counter) behind a backlog of 7.9 - 8.9 ms (HIP events on s1), and every call, those with h_lo / h_hi / h_order
included, had returned while the backlog was still running (an event behind it not yet reached). The backlog outlasts the
sequence 70 times over; 4 times is the least that is wanted.

That the tests can fail, two one-line changes of the library, one at a time:
  * storm_hip_pairw_lag_dosage_corr_device without its final hipStreamSynchronize: both cases of
    test_lag_forms_are_complete_on_return fail in step 1 on the poison of complete_on_return (below), and with them every
    test that builds on the band of rows without missing calls: 16 of the 24;
  * lag_band_threshold_kernel launched on stream 0: wrong keep (a decoy's) in all four cases of test_queued_prune, in both of
    test_primitives_chained_on_one_stream, in test_four_queued_calls_back_to_back, in the two pairs of
    test_a_call_on_each_side_of_set_stream that prune, in test_back_to_the_first_stream_and_to_the_null_stream and in
    test_two_contexts_interleaved: 11 of the 24.

  scenario                                             test
  (a) complete on return, context born on s1           test_lag_forms_are_complete_on_return,
                                                       test_dosage_matrices_are_complete_on_return
  (b) producer, queued call, consumer on one stream    test_queued_ldscore, test_queued_ldscore_annot, test_queued_prune
  (c) the primitives chained on one stream             test_primitives_chained_on_one_stream
  (d) four queued calls back to back on one context    test_four_queued_calls_back_to_back
  (e) across storm_hip_ctx_set_stream                  test_a_call_on_each_side_of_set_stream,
                                                       test_back_to_the_first_stream_and_to_the_null_stream
  (f) two contexts on two streams, interleaved         test_two_contexts_interleaved

  call (storm_hip_...)                                           non-NULL stream in
  pairw_lag_dosage_matrix_device / _matrix                       (a) (c) / (a)
  pairw_lag_dosage_corr_device / _corr                           (a) / (a)
  pairw_lag_dosage_nobs_device / _nobs                           (a) / (a)
  pairw_lag_dosage_corr_complete_device / _corr_complete         (a) (e) / (a)
  pairw_dosage_matrix_device, pairw_dosage_nobs_device,
    square_dosage_matrix_device                                  (a)
  dosage_finish_lag_device                                       (c)
  lag_band_sums_device, lag_band_annot_sums_device,
    lag_band_prune_device                                        (c)
  lag_dosage_ldscore_device / _ldscore                           (b) (d) (e) (f) / (b)
  lag_dosage_ldscore_complete_device / _ldscore_complete         (b) (e) (f) / (b)
  lag_dosage_ldscore_annot_device / _ldscore_annot               (b) (d) (e) (f) / (b)
  lag_dosage_ldscore_annot_complete_device / _annot_complete     (b) / (b)
  lag_dosage_prune_device / _prune                               (b) (d) (e) (f) / (b)
  lag_dosage_prune_complete_device / _prune_complete             (b) (d) / (b)

No test asserts anything about time or about which stream finished first; every test drains the device before it releases
anything. No buffer grows while queued work uses it (the decoy round has grown them)."""
import ctypes as C

import numpy as np
import pytest

import stormbitmaps_amd as sb
from tests import _ldscore, _ldscore_annot, _prune
from tests.test_gpu_dosage import pack
from tests.test_gpu_ldscore_annot import annotations
from tests.test_gpu_streams import SENTINEL, SENTINEL_F, SENTINEL_F_BITS, _check_correlation, _complete_reference, _products
# the fixtures (one instance per importing module) and what they are made of: Streams, Held, Switching and its BACKLOG_PASSES
from tests.test_gpu_streams import born, held, st, sw, sw_module  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = ((300, 96), (513, 4128))       # rows x samples: 3 and 129 words of 32 two-bit samples
KINDS = ("plain", "missing")            # no missing calls (complete-case forms) / a tenth missing (pairwise-complete forms)
LAG, LD = 70, 72
N_ANNOT, ANNOT_LD, SCORE_LD = 65, 70, 68
MIN_R2 = (0.2, 0.5)
GUARD = 3                               # elements (annotation scores: one row) behind n of a queued call's output
KEEP_SENTINEL = 0x77
POISON = -3                             # what an output of (a) holds before its sentinel fill: no count, no N, no r, no r^2
STAT = {"r2": _ldscore.R2, "r2_adj": _ldscore.ADJ}
ALL_ROWS = (1 << 64) - 1


def _vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _hp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _call(ctx, name, *args):
    sb._lib.check(getattr(ctx._lib, name)(ctx._h, *args), name)


# ------------------------------------------------------------------------------------------ the host's side, once
def lagged(full, fill=0):
    """[n, LAG]: entry (i, d) = full[i, i + 1 + d], `fill` in the lower-right corner"""
    n = full.shape[0]
    out = np.full((n, LAG), fill, dtype=full.dtype)
    for d in range(LAG):
        i = np.arange(n - 1 - d)
        out[i, d] = full[i, i + 1 + d]
    return out


def inside(n, rows=None):
    """[rows, LAG] bool: the entries of the lag layout that are a pair"""
    rows = np.arange(n) if rows is None else rows
    return rows[:, None] + 1 + np.arange(LAG)[None, :] < n


class Truth:
    """rows with real LD, their arguments, and what numpy says about them in integers and float64"""

    def __init__(self, n, S, kind):
        self.n, self.S, self.kind, self.complete = n, S, kind, kind == "missing"
        self.x = _prune.ld_rows(n, S, seed=n, missing=0.1 if self.complete else 0.0).astype(np.int64)
        self.mat = pack(self.x)
        assert self.mat.shape == (n, (S + 31) // 32) and min(LAG, n - 1) == LAG
        x = self.x
        self.P = _products(x, x)
        if self.complete:
            assert 0.05 < (x == 3).mean() < 0.15
            present = (x != 3).astype(np.int64)
            self.N = _products(present, present)
            corr, nan = _complete_reference(x)
        else:
            assert x.max() == 2
            s, q = x.sum(axis=1), (x * x).sum(axis=1)
            num, dd = S * self.P - s[:, None] * s[None, :], S * q - s * s
            nan = (dd[:, None] == 0) | (dd[None, :] == 0)
            den = np.where(nan, 1, dd[:, None] * dd[None, :]).astype(np.float64)
            corr = {0: num.astype(np.float64) ** 2 / den, 1: num.astype(np.float64) / np.sqrt(den)}
            self.sums = (s, q)
        self.inside = inside(n)
        self.nan = lagged(nan, False)
        self.corr = {k: lagged(v) for k, v in corr.items()}                   # float64, the lag layout
        self.r2 = np.where(self.nan | ~self.inside, np.nan, self.corr[0])     # ... with NaN where the device writes NaN
        rng = np.random.default_rng(n + S)
        self.priority = rng.random(n, dtype=np.float32)
        self.order = _prune.walk_order(n, self.priority).astype(np.uint32)
        self.lo, self.hi, need = _prune.window_bounds(np.cumsum(rng.integers(1, 5, n)), 9.0)
        assert 0 < need <= LAG, need
        self.annot = np.ascontiguousarray(annotations(n, 7 * n + S)[:, :N_ANNOT])
        d = np.random.default_rng(1000 + n)                                   # the decoy: the same shape, no LD
        self.decoy = d.integers(0, 3, size=(n, S))
        if self.complete:
            self.decoy[d.random((n, S)) < 0.1] = 3
        self.decoy = pack(self.decoy)
        self._greedy = {}

    def greedy(self, min_r2, windows, order):
        """(keep, owner) of the plain greedy over the float64 r^2 — after the three conditions on this reference alone"""
        key = (min_r2, windows, order)
        if key not in self._greedy:
            ok = ~np.isnan(self.r2)
            assert (np.abs(self.r2[ok] - min_r2) > 2.0 ** -20 * min_r2).all(), key   # one float ulp cannot flip an edge
            lo, hi = (self.lo, self.hi) if windows else (None, None)
            nb = _prune.neighbours(self.r2, self.n, LAG, min_r2, lo, hi)
            priority = self.priority if order else None
            keep, owner = _prune.greedy(nb, self.n, priority)
            assert 0.15 <= keep.mean() <= 0.75, (key, keep.mean())
            differ = int((_prune.one_round(nb, self.n, priority) != keep).sum())
            assert differ >= 2, (key, differ)
            self._greedy[key] = (keep, owner)
        return self._greedy[key]


_truths = {}


def truth(shape, kind):
    if (shape, kind) not in _truths:
        _truths[shape, kind] = Truth(shape[0], shape[1], kind)
    return _truths[shape, kind]


# ------------------------------------------------------------------------------------------ the complete-on-return forms
def complete_on_return(st, sw, shape, fill, dtype, call, check):
    """(tensor, host copy): `call` once into a scratch tensor (its work list is cached afterwards), then behind the backlog on
    s1 into a tensor filled with the sentinel on s1, copied under the reader stream at once and handed to `check`. Two calls:
    the same bits.
    The sentinel fill waits behind the backlog like the call's kernels, so a form that returns too early hands back what the
    memory held BEFORE the fill — with torch's caching allocator often a freed tensor of an earlier call with the same
    arguments: the right answer (seen with the synchronise of storm_hip_pairw_lag_dosage_corr_device taken out: the first
    attempt of a shape failed on zeros, a later one passed on a recycled band). So the tensor is first filled with POISON and
    the device drained: an early return then hands back the poison, whatever the memory held"""
    warm = st.full(st.s1, shape, fill, dtype)
    call(warm)
    out = st.full(st.s1, shape, POISON, dtype)
    st.drain()
    sw.backlog()
    with st.torch.cuda.stream(st.s1):
        out.fill_(fill)
    call(out)
    got = st.read(out)
    st.drain()
    check(got)
    assert np.array_equal(got.view(np.uint8), st.read(warm).view(np.uint8))
    return out, got


def lag_corr_device(ctx, m, t, measure, out, ld=LD):
    name = "storm_hip_pairw_lag_dosage_corr_complete_device" if t.complete else "storm_hip_pairw_lag_dosage_corr_device"
    _call(ctx, name, m._h, measure, t.S, LAG, _vp(out), ld)


def check_lag_integers(got, want_full, n, rows, what):
    """got [len(rows), LD] int32: want_full[i, i + 1 + d] at the pairs of the rows, the sentinel everywhere else"""
    want = np.full(got.shape, SENTINEL, dtype=np.int64)
    ok = inside(n, rows)
    want[:, :LAG][ok] = lagged(want_full)[rows][ok]
    bad = np.argwhere(got.astype(np.int64) != want)
    assert len(bad) == 0, (what, len(bad), [(int(i), int(j), int(got[i, j]), int(want[i, j])) for i, j in bad[:5]])


def check_lag_floats(bits, t, measure, what):
    """bits [n, LD] uint32 of a float output: step 1 of the references, and the sentinel outside the pairs"""
    assert (bits[:, LAG:] == SENTINEL_F_BITS).all() and (bits[:, :LAG][~t.inside] == SENTINEL_F_BITS).all(), what
    _check_correlation(bits[:, :LAG], t.corr[measure], t.nan, t.inside, what)


# ------------------------------------------------------------------------------------------ the checked band and what follows
def same_bytes(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, want.shape)
    as_bits = "u%d" % want.dtype.itemsize
    bad = np.argwhere(got.view(as_bits) != want.view(as_bits))
    assert len(bad) == 0, (what, len(bad), [(i.tolist(), got[tuple(i)].item(), want[tuple(i)].item()) for i in bad[:5]])


class Checked:
    """One (shape, rows): the band of r^2 (and N) that a complete-on-return lag form wrote on s1 and step 1 has checked, on
    the host and still on the device, and from there steps 2 - 4 for every set of arguments, each computed once"""

    def __init__(self, t, st, ctx, sw, null_ctx):
        import torch
        self.t, self.st, self.null = t, st, null_ctx
        n = t.n
        m = ctx.matrix_from_host(t.mat)
        try:
            self.d_band, band = complete_on_return(st, sw, (n, LD), SENTINEL_F, torch.float32,
                                                   lambda out: lag_corr_device(ctx, m, t, 0, out),
                                                   lambda got: check_lag_floats(got.view(np.uint32), t, 0, ("band", n, t.kind)))
            self.d_nobs, self.nobs = None, None
            if t.complete:
                self.d_nobs, nobs = complete_on_return(
                    st, sw, (n, LD), SENTINEL, torch.int32,
                    lambda out: _call(ctx, "storm_hip_pairw_lag_dosage_nobs_device", m._h, t.S, LAG, _vp(out), LD),
                    lambda got: check_lag_integers(got, t.N, n, np.arange(n), ("nobs", n)))
                self.nobs = nobs.view(np.uint32)
        finally:
            st.drain()
            m.close()
        self.band = band
        self.band.setflags(write=False)
        self.m0 = null_ctx.matrix_from_host(t.mat)
        pitch = np.full((n, ANNOT_LD), np.nan, dtype=np.float32)
        pitch[:, :N_ANNOT] = t.annot
        self.d_annot = torch.from_numpy(pitch).to("cuda:0")
        self.d_annot_negated = torch.from_numpy(-pitch).to("cuda:0")          # (what a producer on the stream turns back)
        self.d_lo = torch.from_numpy(t.lo.view(np.int32)).to("cuda:0")
        self.d_hi = torch.from_numpy(t.hi.view(np.int32)).to("cuda:0")
        st.drain()
        self._memo = {}

    def close(self):
        self.st.drain()
        self.m0.close()

    def _once(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    def _nobs_view(self, stat):
        """the N of the adjusted statistic of rows with missing calls: the checked nobs matrix"""
        return dict(d_nobs=self.d_nobs.data_ptr(), nobs_row_pitch=LD, nobs_col_stride=1) if self.t.complete and stat == "r2_adj" else {}

    def ldscore(self, stat):
        """(score [n] float32, n_pairs [n] uint32)"""
        def make():
            torch, t, n = self.st.torch, self.t, self.t.n
            what = ("ldscore", n, t.kind, stat)
            score = torch.full((n,), SENTINEL_F, dtype=torch.float32, device="cuda:0")
            pairs = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            self.null.lag_band_sums_device(self.d_band.data_ptr(), LD, n, LAG, score.data_ptr(), pairs.data_ptr(), stat=stat,
                                           n_const=t.S, **self._nobs_view(stat))
            self.null.synchronize()
            s, p = score.cpu().numpy(), pairs.cpu().numpy().view(np.uint32)
            _ldscore.assert_scores(s, p, *_ldscore.band_sums(self.band, n, LAG, STAT[stat], n_const=t.S, nobs=self.nobs), what)
            hs, hp = self.m0.lag_dosage_ldscore(LAG, t.S, stat, t.complete)
            same_bytes(hs, s, what)
            same_bytes(hp, p, what)
            return s, p
        return self._once(("ldscore", stat), make)

    def annot(self, stat, windows):
        """(score [n, N_ANNOT] float32, n_pairs [n] uint32)"""
        def make():
            torch, t, n = self.st.torch, self.t, self.t.n
            what = ("ldscore_annot", n, t.kind, stat, windows)
            lo, hi = (t.lo, t.hi) if windows else (None, None)
            score = torch.full((n, SCORE_LD), SENTINEL_F, dtype=torch.float32, device="cuda:0")
            pairs = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            bounds = dict(d_lo=self.d_lo.data_ptr(), d_hi=self.d_hi.data_ptr()) if windows else {}
            self.null.lag_band_annot_sums_device(self.d_band.data_ptr(), LD, n, LAG, self.d_annot.data_ptr(), ANNOT_LD, N_ANNOT,
                                                 score.data_ptr(), SCORE_LD, pairs.data_ptr(), stat=stat, n_const=t.S,
                                                 **self._nobs_view(stat), **bounds)
            self.null.synchronize()
            s, p = score.cpu().numpy(), pairs.cpu().numpy().view(np.uint32)
            assert (s[:, N_ANNOT:].view(np.uint32) == SENTINEL_F_BITS).all(), what
            s = np.ascontiguousarray(s[:, :N_ANNOT])
            ref = _ldscore_annot.annot_sums(self.band, n, LAG, STAT[stat], t.annot, n_const=t.S, nobs=self.nobs, lo=lo, hi=hi)
            _ldscore_annot.assert_scores(s, p, *ref, what)
            hs, hp = self.m0.lag_dosage_ldscore_annot(t.annot, LAG, t.S, stat, t.complete, lo, hi)
            same_bytes(hs, s, what)
            same_bytes(hp, p, what)
            return s, p
        return self._once(("annot", stat, windows), make)

    def prune(self, min_r2, windows, order):
        """(keep [n] uint8, owner [n] uint32)"""
        def make():
            torch, t, n = self.st.torch, self.t, self.t.n
            what = ("prune", n, t.kind, min_r2, windows, order)
            lo, hi = (t.lo, t.hi) if windows else (None, None)
            walk = t.order if order else None
            keep, owner = _prune.greedy(_prune.neighbours(self.band, n, LAG, min_r2, lo, hi), n, t.priority if order else None)
            keep64, owner64 = t.greedy(min_r2, windows, order)
            assert np.array_equal(keep, keep64) and np.array_equal(owner, owner64), what
            d_keep = torch.full((n,), KEEP_SENTINEL, dtype=torch.uint8, device="cuda:0")
            d_owner = torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            _call(self.null, "storm_hip_lag_band_prune_device", _vp(self.d_band), LD, n, LAG, min_r2, _hp(lo), _hp(hi), _hp(walk),
                  _vp(d_keep), _vp(d_owner))
            self.null.synchronize()
            same_bytes(d_keep.cpu().numpy(), keep, what)
            same_bytes(d_owner.cpu().numpy().view(np.uint32), owner, what)
            hk, ho = self.m0.lag_dosage_prune(min_r2, LAG, t.S, t.complete, True, lo, hi, walk)
            same_bytes(hk, keep, what)
            same_bytes(ho, owner, what)
            return keep, owner
        return self._once(("prune", min_r2, windows, order), make)


class Oracle:
    def __init__(self, *args):
        self.args, self.made = args, {}

    def __call__(self, shape, kind):
        if (shape, kind) not in self.made:
            self.made[shape, kind] = Checked(truth(shape, kind), *self.args)
        return self.made[shape, kind]

    def close(self):
        for c in self.made.values():
            c.close()


@pytest.fixture(scope="module")
def oracle(st, born, sw_module, hip_ctx):
    o = Oracle(st, born, sw_module, hip_ctx)
    yield o
    st.drain()
    o.close()


# ------------------------------------------------------------------------------------------ one queued call
class Queued:
    """One call of a queued _device form: its arguments, its outputs (sentinels, GUARD elements behind n) and what must be in
    them. The host arrays are this object's own copies and live as long as it does"""

    def __init__(self, chk, family, stat="r2", windows=False, order=False, owner=True, pairs=True, min_r2=0.2):
        self.chk, self.t, self.family = chk, chk.t, family
        self.stat, self.windows, self.order, self.owner, self.pairs, self.min_r2 = stat, windows, order, owner, pairs, min_r2
        self.lo = self.t.lo.copy() if windows else None
        self.hi = self.t.hi.copy() if windows else None
        self.walk = self.t.order.copy() if order else None
        self.out = None

    def twin(self):
        return Queued(self.chk, self.family, self.stat, self.windows, self.order, self.owner, self.pairs, self.min_r2)

    def prepare(self, st, stream):
        """the outputs, and for the annotation forms the annotations, made by work on `stream`"""
        torch, n = st.torch, self.t.n
        ints = lambda: st.full(stream, (n + GUARD,), SENTINEL, torch.int32)   # noqa: E731
        if self.family == "ldscore":
            self.out = [st.full(stream, (n + GUARD,), SENTINEL_F, torch.float32), ints() if self.pairs else None]
        elif self.family == "annot":
            with torch.cuda.stream(stream):
                self.d_annot = torch.neg(self.chk.d_annot_negated)
            self.out = [st.full(stream, (n + 1, SCORE_LD), SENTINEL_F, torch.float32), ints() if self.pairs else None]
        else:
            self.out = [st.full(stream, (n + GUARD,), KEEP_SENTINEL, torch.uint8), ints() if self.owner else None]
        return self

    def enqueue(self, ctx, m):
        t, suffix = self.t, "_complete_device" if self.t.complete else "_device"
        if self.family == "ldscore":
            _call(ctx, "storm_hip_lag_dosage_ldscore" + suffix, m._h, STAT[self.stat], t.S, LAG, _vp(self.out[0]), _vp(self.out[1]))
        elif self.family == "annot":
            _call(ctx, "storm_hip_lag_dosage_ldscore_annot" + suffix, m._h, STAT[self.stat], t.S, LAG, _hp(self.lo), _hp(self.hi),
                  _vp(self.d_annot), ANNOT_LD, N_ANNOT, _vp(self.out[0]), SCORE_LD, _vp(self.out[1]))
        else:
            _call(ctx, "storm_hip_lag_dosage_prune" + suffix, m._h, t.S, LAG, self.min_r2, _hp(self.lo), _hp(self.hi), _hp(self.walk),
                  _vp(self.out[0]), _vp(self.out[1]))
        return self

    def host_form(self, m):
        """the host form of the same call through the Python wrapper (which adds nothing to it)"""
        t, lo, hi = self.t, self.lo, self.hi
        if self.family == "ldscore":
            return m.lag_dosage_ldscore(LAG, t.S, self.stat, t.complete)
        if self.family == "annot":
            return m.lag_dosage_ldscore_annot(t.annot, LAG, t.S, self.stat, t.complete, lo, hi)
        return m.lag_dosage_prune(self.min_r2, LAG, t.S, t.complete, True, lo, hi, self.walk)

    def expected(self):
        if self.family == "ldscore":
            return self.chk.ldscore(self.stat)
        if self.family == "annot":
            return self.chk.annot(self.stat, self.windows)
        return self.chk.prune(self.min_r2, self.windows, self.order)

    def snapshot(self):
        """copies of the outputs by the CURRENT stream: consumers of the call, no host wait"""
        return [None if o is None else o.clone() for o in self.out]

    def spoil_host_arrays(self):
        for a in (self.lo, self.hi, self.walk):
            if a is not None:
                a[:] = 0xFFFFFFFF

    def check(self, st, tensors=None, what=None):
        """the outputs (or their snapshot) hold the expected bits in their first n elements and the sentinel behind them"""
        n = self.t.n
        what = (what, self.family, n, self.t.kind, self.stat, self.windows, self.order, self.min_r2)
        tensors = self.out if tensors is None else tensors
        for i, (tensor, want) in enumerate(zip(tensors, self.expected())):
            if tensor is None:
                continue
            got = st.read(tensor)
            if got.ndim == 2:                                                  # the annotation scores: pitch SCORE_LD
                assert (got[:n, N_ANNOT:].view(np.uint32) == SENTINEL_F_BITS).all(), what
                assert (got[n:].view(np.uint32) == SENTINEL_F_BITS).all(), what
                same_bytes(got[:n, :N_ANNOT], want, what + (i,))
                continue
            guard = got[n:]
            if got.dtype == np.uint8:
                assert (guard == KEEP_SENTINEL).all(), what
            elif got.dtype == np.float32:
                assert (guard.view(np.uint32) == SENTINEL_F_BITS).all(), what
            else:
                assert (guard == SENTINEL).all(), what
                got = got.view(np.uint32)
            same_bytes(got[:n], want, what + (i,))


class CompleteOnReturn:
    """storm_hip_pairw_lag_dosage_corr[_complete]_device (r^2) where a Queued may stand: it is read at once, under the reader
    stream, when the call returns"""
    family = "corr"

    def __init__(self, chk):
        self.chk, self.t = chk, chk.t

    def twin(self):
        return CompleteOnReturn(self.chk)

    def prepare(self, st, stream):
        self.st, self.out = st, st.full(stream, (self.t.n, LD), SENTINEL_F, st.torch.float32)
        return self

    def enqueue(self, ctx, m):
        lag_corr_device(ctx, m, self.t, 0, self.out)
        self.got = self.st.read(self.out)
        return self

    def check(self, st, tensors=None, what=None):
        same_bytes(self.got, self.chk.band, (what, "read when the call returned"))
        same_bytes(st.read(self.out), self.chk.band, what)


def decoy_round(st, ctx, stream, held, calls):
    """Every call once on its DECOY rows into scratch outputs, in the order given and then the first one again, and a drain:
    the buffers are grown, the shared scratch holds the decoys' data, and the cached work list is the first call's.
    Returns the matrices of the calls' real rows under `ctx`; `held` releases them and the decoys"""
    made, scratch = {}, []
    for c in calls:
        if id(c.t) not in made:
            made[id(c.t)] = (held.matrix(ctx, c.t.mat), held.matrix(ctx, c.t.decoy))
    for c in list(calls) + [calls[0]]:
        scratch.append(c.twin().prepare(st, stream).enqueue(ctx, made[id(c.t)][1]))
    st.drain()
    return [made[id(c.t)][0] for c in calls]


# ------------------------------------------------------------------------------------------ (a) complete on return
@pytest.mark.parametrize("shape", SHAPES)
def test_lag_forms_are_complete_on_return(born, held, st, sw_module, oracle, shape):
    """behind the backlog on s1, each form into a sentinel tensor that is read under the reader stream as soon as the call
    returns: the dot products whole and as a row band, r^2 and r, N, r^2 and r over the shared samples; then the host forms
    on the same context"""
    torch = st.torch
    n = shape[0]
    plain, missing = truth(shape, "plain"), truth(shape, "missing")
    checked = {kind: oracle(shape, kind) for kind in KINDS}                    # (r^2 of both kinds and N: step 1, in Checked)
    for t in (plain, missing):
        m = held.matrix(born, t.mat)
        what = (shape, t.kind)
        complete_on_return(st, sw_module, (n, LD), SENTINEL, torch.int32, lambda out: _call(
            born, "storm_hip_pairw_lag_dosage_matrix_device", m._h, LAG, 0, ALL_ROWS, _vp(out), LD),
            lambda got: check_lag_integers(got, t.P, n, np.arange(n), what))
        row0, nb = n // 3 + 1, n // 2
        complete_on_return(st, sw_module, (nb, LD), SENTINEL, torch.int32, lambda out: _call(
            born, "storm_hip_pairw_lag_dosage_matrix_device", m._h, LAG, row0, nb, _vp(out), LD),
            lambda got: check_lag_integers(got, t.P, n, np.arange(row0, row0 + nb), what + ("band",)))
        for measure in (0, 1):
            _, got = complete_on_return(st, sw_module, (n, LD), SENTINEL_F, torch.float32,
                                        lambda out: lag_corr_device(born, m, t, measure, out),
                                        lambda got: check_lag_floats(got.view(np.uint32), t, measure, what + (measure,)))
            if measure == 0:
                same_bytes(got, checked[t.kind].band, what)
            host = (m.pairw_lag_dosage_corr_complete if t.complete else m.pairw_lag_dosage_corr)(LAG, t.S, ("r2", "r")[measure])
            same_bytes(host, np.where(t.inside, got[:, :LAG], np.float32(0)), what + ("host", measure))
        host = m.pairw_lag_dosage_matrix(LAG)
        assert np.array_equal(host.astype(np.int64), np.where(t.inside, lagged(t.P), 0)), what
        if t.complete:
            host = m.pairw_lag_dosage_nobs(LAG, t.S)
            assert np.array_equal(host.astype(np.int64), np.where(t.inside, lagged(t.N), 0)), what
            same_bytes(host[t.inside], checked["missing"].nobs[:, :LAG][t.inside], what)


@pytest.mark.parametrize("shape", SHAPES)
def test_dosage_matrices_are_complete_on_return(born, held, st, sw_module, shape):
    """storm_hip_pairw_dosage_matrix_device, storm_hip_pairw_dosage_nobs_device and storm_hip_square_dosage_matrix_device"""
    torch = st.torch
    n, ld = shape[0], shape[0] + 3
    plain, missing = truth(shape, "plain"), truth(shape, "missing")
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    for t, name, args, want in ((plain, "storm_hip_pairw_dosage_matrix_device", (), plain.P),
                                (missing, "storm_hip_pairw_dosage_nobs_device", (missing.S,), missing.N)):
        m = held.matrix(born, t.mat)
        full = np.full((n, ld), SENTINEL, dtype=np.int64)
        full[:, :n][upper] = want[upper]
        complete_on_return(st, sw_module, (n, ld), SENTINEL, torch.int32, lambda out: _call(born, name, m._h, *args, _vp(out), ld),
                           lambda got: same_bytes(got.astype(np.int64), full, name))
    nb_rows, ldb = 130, 135                                                    # B: the last 130 rows, last row first
    a, b = held.matrix(born, plain.mat), held.matrix(born, plain.mat[::-1][:nb_rows])
    full = np.full((n, ldb), SENTINEL, dtype=np.int64)
    full[:, :nb_rows] = _products(plain.x, plain.x[::-1][:nb_rows])
    complete_on_return(st, sw_module, (n, ldb), SENTINEL, torch.int32, lambda out: _call(
        born, "storm_hip_square_dosage_matrix_device", a._h, b._h, _vp(out), ldb),
        lambda got: same_bytes(got.astype(np.int64), full, "storm_hip_square_dosage_matrix_device"))


# ------------------------------------------------------------------------------------------ (b) producer, call, consumer
def queued_on_one_stream(st, sw, ctx, held, calls):
    """Each call alone: its decoy round; the backlog; then on s1 and with no host wait the outputs' sentinel fill (and the
    annotations) by torch, the call through ctypes, and clones of the outputs. The clones after s1 has run, the originals
    after storm_hip_ctx_synchronize, the originals again after the host arrays have been overwritten: the same bytes"""
    torch = st.torch
    for call in calls:
        mats = decoy_round(st, ctx, st.s1, held, [call])
        sw.backlog()
        with torch.cuda.stream(st.s1):
            call.prepare(st, st.s1).enqueue(ctx, mats[0])
            snap = call.snapshot()
        st.s1.synchronize()
        call.check(st, snap, "snapshot")
        ctx.synchronize()
        call.check(st, None, "outputs")
        call.spoil_host_arrays()
        st.drain()
        call.check(st, None, "after the host arrays were overwritten")
        for got, want in zip(call.twin().host_form(mats[0]), call.expected()):   # the host form on the caller's stream
            same_bytes(got, want, ("host form", call.family))
    return calls


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_queued_ldscore(born, held, st, sw_module, oracle, shape, kind):
    """both statistics; d_n_pairs NULL: the same scores"""
    chk = oracle(shape, kind)
    queued_on_one_stream(st, sw_module, born, held, [Queued(chk, "ldscore", stat="r2"), Queued(chk, "ldscore", stat="r2_adj"),
                                                    Queued(chk, "ldscore", stat="r2_adj", pairs=False)])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_queued_ldscore_annot(born, held, st, sw_module, oracle, shape, kind):
    """65 columns (one chunk of 64 and one more) from annotations a torch kernel on s1 has just written; with and without
    windows"""
    chk = oracle(shape, kind)
    queued_on_one_stream(st, sw_module, born, held, [Queued(chk, "annot", stat="r2"),
                                                    Queued(chk, "annot", stat="r2_adj", windows=True),
                                                    Queued(chk, "annot", stat="r2", windows=True, pairs=False)])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_queued_prune(born, held, st, sw_module, oracle, shape, kind):
    """with owner, windows and order, and with all three NULL, at both thresholds; keep is the same with and without d_owner"""
    chk = oracle(shape, kind)
    calls = []
    for min_r2 in MIN_R2:
        calls += [Queued(chk, "prune", min_r2=min_r2, windows=True, order=True), Queued(chk, "prune", min_r2=min_r2, owner=False),
                  Queued(chk, "prune", min_r2=min_r2, windows=True, order=True, owner=False), Queued(chk, "prune", min_r2=min_r2)]
    queued_on_one_stream(st, sw_module, born, held, calls)
    for k in (0, 4):
        for with_owner, without in ((calls[k], calls[k + 2]), (calls[k + 3], calls[k + 1])):
            assert np.array_equal(st.read(with_owner.out[0]), st.read(without.out[0]))


# ------------------------------------------------------------------------------------------ (c) the primitives, chained
@pytest.mark.parametrize("shape", SHAPES)
def test_primitives_chained_on_one_stream(born, held, st, sw_module, oracle, shape):
    """dot products into the caller's tensor (complete on return), the rows' sums by torch on s1, then with nothing between
    them but the stream: storm_hip_dosage_finish_lag_device, storm_hip_lag_band_sums_device (both statistics),
    storm_hip_lag_band_annot_sums_device (windows) and storm_hip_lag_band_prune_device (windows, order, owner) over that
    tensor. The band is storm_hip_pairw_lag_dosage_corr_device's, the three results are the composite forms' of (b).
    Twice: the first round grows the prune call's scratch"""
    torch = st.torch
    chk = oracle(shape, "plain")
    t, n = chk.t, shape[0]
    m = held.matrix(born, t.mat)
    x = torch.from_numpy(t.x.astype(np.int32)).to("cuda:0")
    lo, hi, walk = t.lo.copy(), t.hi.copy(), t.order.copy()
    st.drain()
    for _ in range(2):
        sw_module.backlog()
        band = st.full(st.s1, (n, LD), SENTINEL_F, torch.float32)          # (uint32 dot products, then floats, in place)
        _call(born, "storm_hip_pairw_lag_dosage_matrix_device", m._h, LAG, 0, ALL_ROWS, _vp(band), LD)
        sw_module.backlog()
        with torch.cuda.stream(st.s1):
            d_sum, d_sq = x.sum(dim=1, dtype=torch.int32), (x * x).sum(dim=1, dtype=torch.int32)
            d_annot = torch.neg(chk.d_annot_negated)
            d_lo, d_hi = chk.d_lo.clone(), chk.d_hi.clone()
            score = {stat: st.full(st.s1, (n + GUARD,), SENTINEL_F, torch.float32) for stat in STAT}
            pairs = {stat: st.full(st.s1, (n + GUARD,)) for stat in STAT}
            a_score, a_pairs = st.full(st.s1, (n + 1, SCORE_LD), SENTINEL_F, torch.float32), st.full(st.s1, (n + GUARD,))
            keep, owner = st.full(st.s1, (n + GUARD,), KEEP_SENTINEL, torch.uint8), st.full(st.s1, (n + GUARD,))
            _call(born, "storm_hip_dosage_finish_lag_device", _vp(band), LD, n, 0, ALL_ROWS, LAG, _vp(d_sum), _vp(d_sq), 0, t.S)
            vals = band
            for stat in STAT:
                born.lag_band_sums_device(vals.data_ptr(), LD, n, LAG, score[stat].data_ptr(), pairs[stat].data_ptr(), stat=stat,
                                          n_const=t.S)
            born.lag_band_annot_sums_device(vals.data_ptr(), LD, n, LAG, d_annot.data_ptr(), ANNOT_LD, N_ANNOT, a_score.data_ptr(),
                                            SCORE_LD, a_pairs.data_ptr(), stat="r2_adj", n_const=t.S, d_lo=d_lo.data_ptr(),
                                            d_hi=d_hi.data_ptr())
            _call(born, "storm_hip_lag_band_prune_device", _vp(vals), LD, n, LAG, 0.5, _hp(lo), _hp(hi), _hp(walk), _vp(keep),
                  _vp(owner))
            snap = [o.clone() for o in (vals, score["r2"], pairs["r2"], score["r2_adj"], pairs["r2_adj"], a_score, a_pairs, keep, owner)]
        st.s1.synchronize()
        got = [st.read(o) for o in snap]
        same_bytes(got[0], chk.band, "the finished band")
        for stat, s, p in (("r2", got[1], got[2]), ("r2_adj", got[3], got[4])):
            assert (s[n:].view(np.uint32) == SENTINEL_F_BITS).all() and (p[n:] == SENTINEL).all()
            same_bytes(s[:n], chk.ldscore(stat)[0], ("sums", stat))
            same_bytes(p[:n].view(np.uint32), chk.ldscore(stat)[1], ("sums", stat))
        want_score, want_pairs = chk.annot("r2_adj", True)
        assert (got[5][:, N_ANNOT:].view(np.uint32) == SENTINEL_F_BITS).all() and (got[5][n:].view(np.uint32) == SENTINEL_F_BITS).all()
        same_bytes(got[5][:n, :N_ANNOT], want_score, "annot sums")
        assert (got[6][n:] == SENTINEL).all() and (got[7][n:] == KEEP_SENTINEL).all() and (got[8][n:] == SENTINEL).all()
        same_bytes(got[6][:n].view(np.uint32), want_pairs, "annot pairs")
        want_keep, want_owner = chk.prune(0.5, True, True)
        same_bytes(got[7][:n], want_keep, "keep")
        same_bytes(got[8][:n].view(np.uint32), want_owner, "owner")
        st.drain()


# ------------------------------------------------------------------------------------------ (d) back to back
def test_four_queued_calls_back_to_back(born, held, st, sw_module, oracle):
    """ldscore on A (300 rows), prune on B (513 rows), ldscore_annot on A, prune_complete on B's rows with missing calls: no
    wait in between, each into its own tensors, all through one band buffer, one set of split rows, sums and tickets and one
    cached work list (which every change of shape or form plans anew)"""
    a, b, bm = oracle(SHAPES[0], "plain"), oracle(SHAPES[1], "plain"), oracle(SHAPES[1], "missing")
    calls = [Queued(a, "ldscore", stat="r2_adj"), Queued(b, "prune", min_r2=0.2, windows=True, order=True),
             Queued(a, "annot", stat="r2", windows=True), Queued(bm, "prune", min_r2=0.5)]
    mats = decoy_round(st, born, st.s1, held, calls)
    sw_module.backlog()
    for c in calls:
        c.prepare(st, st.s1)
    for c, m in zip(calls, mats):
        c.enqueue(born, m)
    st.drain()
    for i, c in enumerate(calls):
        c.check(st, None, i)


# ------------------------------------------------------------------------------------------ (e) across set_stream
PAIRS = {
    "ldscore_complete_adj+prune": (("missing", "ldscore", dict(stat="r2_adj")), ("plain", "prune", dict(min_r2=0.5))),
    "prune_order+annot_windows": (("plain", "prune", dict(min_r2=0.2, order=True)), ("plain", "annot", dict(stat="r2", windows=True))),
    "ldscore+corr_complete": (("plain", "ldscore", dict(stat="r2")), ("missing", "corr_complete", {})),
}


@pytest.mark.parametrize("pair", sorted(PAIRS))
def test_a_call_on_each_side_of_set_stream(sw, held, st, oracle, pair):
    """the backlog on s1; s2 gated behind it; a queued call on A (300 rows) through the context on s1; set_stream(s2); at
    once a second call on B (513 rows). The two share the band buffer, the split rows, the sums matrix, the masks and the
    work list (which the second call plans anew), and only the event of set_stream stands between them"""
    ctx = sw.ctx
    (kind_a, family_a, args_a), (kind_b, family_b, args_b) = PAIRS[pair]
    first = Queued(oracle(SHAPES[0], kind_a), family_a, **args_a)
    chk_b = oracle(SHAPES[1], kind_b)
    second = CompleteOnReturn(chk_b) if family_b == "corr_complete" else Queued(chk_b, family_b, **args_b)
    mats = decoy_round(st, ctx, st.s1, held, [first, second])                  # (the cached list is the first call's)
    first.prepare(st, st.s1)
    second.prepare(st, st.s1)                                                  # (on s1 too: the event of set_stream orders it)
    st.drain()
    sw.backlog()
    sw.gate()
    first.enqueue(ctx, mats[0])
    ctx.set_stream(st.s2.cuda_stream)
    second.enqueue(ctx, mats[1])
    st.drain()
    first.check(st, None, "before set_stream")
    second.check(st, None, "after set_stream")


def test_back_to_the_first_stream_and_to_the_null_stream(sw, held, st, oracle):
    """s1, s2, s1 again, the NULL stream: a queued call on each, nothing waited for until the end"""
    ctx = sw.ctx
    a, b, bm = oracle(SHAPES[0], "plain"), oracle(SHAPES[1], "plain"), oracle(SHAPES[1], "missing")
    calls = [Queued(b, "prune", min_r2=0.5, windows=True, order=True), Queued(a, "ldscore", stat="r2"),
             Queued(bm, "ldscore", stat="r2_adj"), Queued(a, "annot", stat="r2_adj")]
    mats = decoy_round(st, ctx, st.s1, held, calls)
    for c in calls:
        c.prepare(st, st.s1)                                                   # (ordered before every later stream by the events)
    st.drain()
    sw.backlog()
    sw.gate()
    for c, m, stream in zip(calls, mats, (None, st.s2.cuda_stream, st.s1.cuda_stream, 0)):
        if stream is not None:
            ctx.set_stream(stream)
        c.enqueue(ctx, m)
    st.drain()
    for i, c in enumerate(calls):
        c.check(st, None, ("stream", i))


# ------------------------------------------------------------------------------------------ (f) two contexts, one thread
@pytest.fixture(scope="module")
def two_contexts(st):
    x, y = sb.HipContext(0, st.s1.cuda_stream), sb.HipContext(0, st.s2.cuda_stream)
    yield x, y
    st.drain()
    x.close()
    y.close()


def test_two_contexts_interleaved(two_contexts, held, st, sw_module, oracle):
    """X on s1 with A, Y on s2 with B: X ldscore, Y prune, X ldscore_annot, Y ldscore_complete, all queued, then one drain:
    the workspaces are independent"""
    x, y = two_contexts
    a, b, bm = oracle(SHAPES[0], "plain"), oracle(SHAPES[1], "plain"), oracle(SHAPES[1], "missing")
    of_x = [Queued(a, "ldscore", stat="r2"), Queued(a, "annot", stat="r2_adj", windows=True)]
    of_y = [Queued(b, "prune", min_r2=0.2, order=True), Queued(bm, "ldscore", stat="r2_adj")]
    mats_x, mats_y = decoy_round(st, x, st.s1, held, of_x), decoy_round(st, y, st.s2, held, of_y)
    sw_module.backlog()
    sw_module.gate()
    for c in of_x:
        c.prepare(st, st.s1)
    for c in of_y:
        c.prepare(st, st.s2)
    for cx, mx, cy, my in zip(of_x, mats_x, of_y, mats_y):
        cx.enqueue(x, mx)
        cy.enqueue(y, my)
    st.drain()
    for i, c in enumerate(of_x + of_y):
        c.check(st, None, ("context", i))
