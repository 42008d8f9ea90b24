"""The lag-band calls at the row counts and lags README.md quotes them at: above 32768 rows, at lags of 993 to 4096, on 2^20
rows and on a band whose rows lie beyond 2^32 bytes. Everything goes through the C-ABI (HipContext.lag_band_prune_device,
lag_band_sums_device, lag_band_annot_sums_device, the HipMatrix.pairw_lag_dosage_* device forms, StormDosage, StormContig,
Storm). The references are tests/_ld_scale.py's, which work in the lag layout itself and which tests/test_ld_scale_refs.py
checks on the CPU. What each shape reaches is asserted from the shape at the top of its test.

  A. pruning over bands the test writes on the device: a sparse random graph (n = 33000: the second pass of the resolver's
     LDS clear, mask pitches of 66, 130 and 258 words, 65 forward chunks), cliques and strided paths with a closed-form answer
     (n = 2^20: the whole LDS state; lag 993 at pitch 1027: rows of the band beyond 2^32 bytes). keep and owner EXACTLY.
  B. sums over bands the test writes: a formula band of multiples of 2^-10 (n = 2^20, lag 993) whose sums are exact in
     double — the score's bits and the counts exactly; a random band (n = 2500, lag 1100: interior rows with 1100 pairs on
     each side) inside tests/_ldscore.py's and tests/_ldscore_annot.py's bounds, 65 annotation columns, both inner products.
  C. containers: StormDosage, HipMatrix (dosage rows), StormContig and Storm against exact integers and, for floats,
     _sweep.close_floats (the NaN mask from integers, else at most 1 ulp); LD scores inside _ldscore.bound over the
     library's own band once that band has met its reference; pruning EXACTLY against _prune.greedy over the reference's
     r^2 with min_r2 = _sweep.prune_threshold(values, 0.5).

Every device output has guard elements behind it; every band's corner and pitch columns are poisoned (HIGH for pruning, a
non-NaN sentinel for sums).

The prune comparison of part C needs every in-window reference r^2 to lie at least _sweep.PRUNE_MARGIN (relative) from
min_r2: a condition on the inputs, asserted. The seeds were tried on the CPU from the reference alone — for each shape
and missing share the first seed tried, 100 n + S as tests/test_gpu_prune.py draws it, met it (the margins are printed);
no other seed was tried."""
import numpy as np
import pytest

import stormbitmaps_amd as sb
from stormbitmaps_amd import dist
from tests import _ld_scale, _ldscore, _ldscore_annot, _prune, _sweep
from tests._ldscore import ADJ, R2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 5                                                                          # elements behind n of a device output
GUARD_K, GUARD_O, GUARD_F, GUARD_I = 0x77, 0x5EADBEEF, -77.5, 0x5EADBEEF
T = np.float32(0.5)                                                                # min_r2 of the written prune bands
HIGH, LOW = np.float32(0.9), np.float32(0.1)
JUST_ABOVE, JUST_BELOW = np.nextafter(T, np.float32(1)), np.nextafter(T, np.float32(0))
POISON_F = -3.0e4                                                                  # corner and pitch of a band that is summed
N_MAX = 1 << 20                                                                    # STORM_PRUNE_MAX_ROWS
STATS = {"r2": R2, "r2_adj": ADJ}


# ------------------------------------------------------------------------------------------ A. prune on written bands
def write_prune_band(n, L, ld, seed, edges=None, ahead=None):
    """[n, ld] float32 on the device, as tests/test_gpu_prune.py's make_band: non-edges drawn from {LOW, T, NaN, +-0, the float
    below T}, the corner and the pitch columns at HIGH; edges — the (i, d) of `edges`, and the lags d < ahead[i] — at HIGH or
    the float above T. Written in row chunks so that no temporary exceeds 2^24 entries."""
    import torch
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    table = torch.tensor([LOW, T, np.nan, 0.0, -0.0, JUST_BELOW], dtype=torch.float32, device=DEV)
    above = torch.tensor([HIGH, JUST_ABOVE], dtype=torch.float32, device=DEV)
    band = torch.full((n, ld), float(HIGH), dtype=torch.float32, device=DEV)
    d = torch.arange(L, device=DEV)[None, :]
    t_ahead = None if ahead is None else torch.from_numpy(ahead).to(DEV)
    chunk = max(1, (1 << 24) // L)
    for r0 in range(0, n, chunk):
        r1 = min(r0 + chunk, n)
        i = torch.arange(r0, r1, device=DEV)[:, None]
        v = table[torch.randint(0, 6, (r1 - r0, L), generator=gen, device=DEV)]
        if t_ahead is not None:
            v = torch.where(d < t_ahead[r0:r1, None], above[(i + d) % 2], v)
        band[r0:r1, :L] = torch.where(i + 1 + d < n, v, above[0])
    if edges is not None:
        ei, ed = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in edges)
        band[ei, ed] = above[(ei + ed) % 2]
    torch.cuda.synchronize()
    return band


def band_prune(ctx, band, n, L, priority=None, lo=None, hi=None, with_owner=True):
    """(keep, owner) of storm_hip_lag_band_prune_device over a band on the device, guards checked"""
    import torch
    d_keep = torch.full((n + GUARD,), GUARD_K, dtype=torch.uint8, device=DEV)
    d_owner = torch.full((n + GUARD,), GUARD_O, dtype=torch.int32, device=DEV)
    order = None if priority is None else _prune.walk_order(n, priority)
    torch.cuda.synchronize()                                                       # the guards are in place before the call's stream runs
    ctx.lag_band_prune_device(band.data_ptr(), band.stride(0), n, L, float(T), d_keep.data_ptr(),
                              d_owner.data_ptr() if with_owner else None, lo, hi, order)
    keep, owner = d_keep.cpu().numpy(), d_owner.cpu().numpy().view(np.uint32)
    assert (keep[n:] == GUARD_K).all() and (owner[n:] == GUARD_O).all()
    if not with_owner:
        assert (owner == GUARD_O).all()
    return keep[:n], owner[:n]


def assert_same(got, want, where):
    for name, g, w in zip(("keep", "owner"), got, want):
        assert np.array_equal(g, w), (where, name, int((g != w).sum()), np.flatnonzero(g != w)[:8].tolist())


@pytest.mark.parametrize("L,ld,pitch_above", [(993, 996, 64), (2017, 2020, 128), (4096, 4099, 256)])
def test_prune_above_32768_rows_at_mask_pitches_of_many_wave_trips(hip_ctx, L, ld, pitch_above):
    n = 33000
    assert (n + 31) // 32 > 1024                                                   # the resolver's 1024 threads clear the LDS state twice
    assert _prune.mask_pitch(L) > pitch_above and _prune.mask_pitch(L) <= pitch_above + 64   # one more trip of 64 lanes each
    if L == 4096:
        assert L // 64 + 1 == 65                                                   # forward chunks of the threshold kernel
    i, d = _ld_scale.random_edges(n, L, 7 * L)
    j = i + 1 + d
    assert {0, L - 1} <= set(d[i < 64].tolist()) and {0, L - 1} <= set(d[j >= n - 64].tolist())
    band = write_prune_band(n, L, ld, L, edges=(i, d))
    rng = np.random.default_rng(L)
    pos = np.cumsum(rng.integers(1, 5, size=n)).astype(np.float64)                 # steps of 1 to 4: about L / 2 rows on each side
    lo, hi = _ldscore_annot.windows(pos, 1.25 * L)
    assert _ldscore_annot.window_lag(lo, hi) <= L
    priorities = {"none": None, "random": rng.random(n, dtype=np.float32), "descending": _ld_scale.descending(n)}
    for windows in (None, (lo, hi)):
        inside = np.ones(len(i), bool) if windows is None else (j <= hi[i]) & (i >= lo[j])
        if windows is not None:
            assert 0.2 * len(i) < inside.sum() < 0.8 * len(i)                      # the windows cut edges, and leave some
        nb = _ld_scale.neighbours_of(n, i[inside], j[inside])
        kw = {} if windows is None else {"lo": lo, "hi": hi}
        for kind, priority in priorities.items():
            where = (n, L, windows is not None, kind)
            ref = _prune.greedy(nb, n, priority)
            assert 0.2 <= ref[0].mean() <= 0.8, (where, ref[0].mean())
            got = band_prune(hip_ctx, band, n, L, priority, **kw)
            assert_same(got, ref, where)
            only, _ = band_prune(hip_ctx, band, n, L, priority, with_owner=False, **kw)
            assert np.array_equal(only, ref[0]), where                             # the same with and without owner
            if kind == "random":
                again = band_prune(hip_ctx, band, n, L, priority, **kw)
                assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes(), where   # two calls, the same bytes
        if windows is None:
            assert (_prune.one_round(nb, n, None) != _prune.greedy(nb, n, None)[0]).sum() >= 100   # not a one-round answer


def test_prune_cliques_over_the_whole_lds_state(hip_ctx):
    n, L, ld = N_MAX, 33, 36
    assert n == 1 << 20 and (n + 31) // 32 == 32768 and (n + 63) // 64 == 16384    # every word of the state, 16384 batches
    starts = _ld_scale.clique_runs(n, L, 20)
    ahead = _ld_scale.clique_ahead(n, starts)
    assert ahead.max() == 23 and len(starts) > n // 16
    band = write_prune_band(n, L, ld, 20, ahead=ahead)
    rng = np.random.default_rng(20)
    for kind, priority in (("none", None), ("random", rng.random(n, dtype=np.float32)), ("descending", _ld_scale.descending(n))):
        ref = _ld_scale.clique_reference(n, starts, None if priority is None else _prune.walk_order(n, priority))
        assert ref[0].sum() == len(starts)
        got = band_prune(hip_ctx, band, n, L, priority)
        assert_same(got, ref, ("cliques", kind))
        if kind == "random":
            again = band_prune(hip_ctx, band, n, L, priority)
            assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
            only, _ = band_prune(hip_ctx, band, n, L, priority, with_owner=False)
            assert np.array_equal(only, ref[0])


@pytest.mark.parametrize("L,ld", [(33, 36), (993, 1027)])
def test_prune_strided_paths_on_2_20_rows(hip_ctx, L, ld):
    n = N_MAX
    assert (n + 31) // 32 == 32768
    if L == 993:
        assert n * ld * 4 > 1 << 32 and _prune.mask_pitch(L) > 64                  # rows of vals beyond 2^32 bytes
    rows = np.arange(n - L)
    band = write_prune_band(n, L, ld, L, edges=(rows, np.full_like(rows, L - 1)))  # the only edges: (i, i + L), the last lag
    for kind, priority in (("none", None), ("descending", _ld_scale.descending(n))):
        ref = _ld_scale.strided_reference(n, L, kind == "descending")
        got = band_prune(hip_ctx, band, n, L, priority)
        assert_same(got, ref, ("paths", L, kind))
    again = band_prune(hip_ctx, band, n, L, priority)
    assert again[0].tobytes() == got[0].tobytes() and again[1].tobytes() == got[1].tobytes()
    only, _ = band_prune(hip_ctx, band, n, L, priority, with_owner=False)
    assert np.array_equal(only, ref[0])


# ------------------------------------------------------------------------------------------ B. sums on written bands
def vector_outputs(n, n_cols=None, pad=0):
    import torch
    score = torch.full((n + GUARD,) if n_cols is None else (n + GUARD, n_cols + pad), GUARD_F, dtype=torch.float32, device=DEV)
    pairs = torch.full((n + GUARD,), GUARD_I, dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    return score, pairs


def test_sums_of_the_formula_band_on_2_20_rows_have_the_references_bits(hip_ctx):
    n, L, ld = N_MAX, 993, 1027
    assert n * ld * 4 > 1 << 32                                                    # rows of the band beyond 2^32 bytes
    band = _ld_scale.formula_band(n, L, ld, DEV, POISON_F)
    want, want_pairs = _ld_scale.formula_sums(n, L, DEV)
    rows = np.arange(n)
    assert np.array_equal(want_pairs, np.minimum(L, rows) + np.minimum(L, n - 1 - rows))
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want) and want.max() > L / 2
    first = None
    for _ in range(2):
        d_score, d_pairs = vector_outputs(n)
        hip_ctx.lag_band_sums_device(band.data_ptr(), ld, n, L, d_score.data_ptr(), d_pairs.data_ptr(), "r2")
        hip_ctx.synchronize()
        score, pairs = d_score.cpu().numpy(), d_pairs.cpu().numpy().view(np.uint32)
        assert (score[n:] == np.float32(GUARD_F)).all() and (pairs[n:] == GUARD_I).all()
        _sweep.equal(pairs[:n], want_pairs.astype(np.uint32), "n_pairs")
        _sweep.equal(_sweep.bits_of(score[:n]), _sweep.bits_of(want.astype(np.float32)), "the score's bits")
        first = score.tobytes() if first is None else first
        assert score.tobytes() == first                                            # two calls, the same bytes


class RandomBand:
    """n = 2500, lag 1100, pitch 1103: interior rows 1100 .. 1399 have all 1100 pairs on each side. A random float band in
    [0, 1] with 2 % NaN, N behind a strided view as the pairwise-complete call passes it, 65 annotation columns, windows
    from positions. Built once; the references are kept per configuration."""
    n, L, ld, C = 2500, 1100, 1103, 65
    annot_ld, score_ld = C + 5, C + 3

    def __init__(self):
        import torch
        n, L, ld, C = self.n, self.L, self.ld, self.C
        rng = np.random.default_rng(2500)
        ok = np.zeros((n, ld), bool)
        ok[:, :L] = _sweep.lag_mask(n, L)
        vals = rng.random((n, ld), dtype=np.float32)
        vals[rng.random((n, ld)) < 0.02] = np.nan
        self.band = np.where(ok, vals, np.float32(POISON_F))
        N = rng.choice(np.array([0, 1, 2, 3, 4, 77, 5000], dtype=np.uint32), size=(n, ld))
        self.lds = (3 * L + 2 + 3) // 4 * 4
        sums = np.full((3 * n, self.lds), 0xDEADBEEF, dtype=np.uint32)
        sums[2::3, 2:3 * L + 2:3] = np.where(ok, N, 0xDEADBEEF)[:, :L]
        self.nobs = sums[2::3, 2:3 * L + 2:3]
        self.annot, self.base, self.scale = _ld_scale.scaled_annotations(n, C, 65)
        padded = np.full((n, self.annot_ld), np.nan, dtype=np.float32)
        padded[:, :C] = self.annot
        pos = np.cumsum(rng.integers(1, 5, size=n)).astype(np.float64)
        self.lo, self.hi = _ldscore_annot.windows(pos, 1500.0)                     # about 600 rows on each side
        assert 400 < _ldscore_annot.window_lag(self.lo, self.hi) <= L
        self.d_band = torch.from_numpy(self.band).to(DEV)
        self.d_sums = torch.from_numpy(sums.view(np.int32)).to(DEV)
        self.d_annot = torch.from_numpy(padded).to(DEV)
        self.d_lo, self.d_hi = (torch.from_numpy(x.view(np.int32).copy()).to(DEV) for x in (self.lo, self.hi))
        for a in (self.band, self.nobs, self.annot):
            a.setflags(write=False)
        self._refs = {}

    def nobs_args(self, view):
        """(d_nobs, row pitch, column stride) of the strided N view, or of none"""
        return (self.d_sums.data_ptr() + 4 * (2 * self.lds + 2), 3 * self.lds, 3) if view else (None, 0, 1)

    def plain_reference(self, stat, n_const, view):
        key = ("plain", stat, n_const, view)
        if key not in self._refs:
            self._refs[key] = _ldscore.band_sums(self.band, self.n, self.L, STATS[stat], n_const, self.nobs if view else None)
        return self._refs[key]

    def annot_reference(self, stat, n_const, view, windowed):
        key = ("annot", stat, n_const, view, windowed)
        if key not in self._refs:
            base = _ldscore_annot.annot_sums(self.band, self.n, self.L, STATS[stat], self.base, n_const, self.nobs if view else None,
                                             self.lo if windowed else None, self.hi if windowed else None)
            self._refs[key] = _ld_scale.scaled_annot_sums(base, self.scale)
        return self._refs[key]


_random_band = []


def random_band():
    if not _random_band:
        _random_band.append(RandomBand())
    return _random_band[0]


CONFIGS = [("r2", 0, False), ("r2_adj", 900, False), ("r2_adj", 0, True)]          # (stat, n_const, N from the view)


def test_plain_sums_with_full_windows_of_1100_rows_on_both_sides(hip_ctx):
    b = random_band()
    n, L = b.n, b.L
    assert n - 2 * L >= 300                                                        # rows whose window is complete on both sides
    for stat, n_const, view in CONFIGS + [("r2", 0, True)]:
        d_score, d_pairs = vector_outputs(n)
        hip_ctx.lag_band_sums_device(b.d_band.data_ptr(), b.ld, n, L, d_score.data_ptr(), d_pairs.data_ptr(), stat, n_const,
                                     *b.nobs_args(view))
        hip_ctx.synchronize()
        score, pairs = d_score.cpu().numpy(), d_pairs.cpu().numpy().view(np.uint32)
        assert (score[n:] == np.float32(GUARD_F)).all() and (pairs[n:] == GUARD_I).all()
        ref, sum_abs, m = b.plain_reference(stat, n_const, view)
        _ldscore.assert_scores(score[:n], pairs[:n], ref, sum_abs, m, (stat, n_const, view))
        if stat == "r2":
            assert m[L:n - L].min() > 2 * L * 0.9 and m.max() <= 2 * L             # 2 % NaN: nearly the whole window


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("stat,n_const,view", CONFIGS)
def test_annotated_sums_of_65_columns_under_both_inner_products(hip_ctx, monkeypatch, stat, n_const, view, windowed):
    b = random_band()
    n, L, C = b.n, b.L, b.C
    assert C > 64                                                                  # two chunks of 64 columns
    ref, sum_abs, m, a_max = b.annot_reference(stat, n_const, view, windowed)
    assert ref.shape == (n, C)
    if windowed:
        assert m.max() < b.plain_reference(stat, n_const, view)[2].max()           # the windows cut pairs
    for inner in ("fma", "mfma"):
        monkeypatch.setenv("STORM_HIP_LDSCORE_ANNOT_INNER", inner)
        d_score, d_pairs = vector_outputs(n, C, b.score_ld - C)
        hip_ctx.lag_band_annot_sums_device(b.d_band.data_ptr(), b.ld, n, L, b.d_annot.data_ptr(), b.annot_ld, C, d_score.data_ptr(),
                                           b.score_ld, d_pairs.data_ptr(), stat, n_const, *b.nobs_args(view),
                                           b.d_lo.data_ptr() if windowed else None, b.d_hi.data_ptr() if windowed else None)
        hip_ctx.synchronize()
        score, pairs = d_score.cpu().numpy(), d_pairs.cpu().numpy().view(np.uint32)
        assert (score[n:] == np.float32(GUARD_F)).all() and (score[:, C:] == np.float32(GUARD_F)).all() and (pairs[n:] == GUARD_I).all()
        _ldscore_annot.assert_scores(score[:n, :C], pairs[:n], ref, sum_abs, m, a_max, (stat, n_const, view, windowed, inner))


# ------------------------------------------------------------------------------------------ C. containers
CHUNK = 2048                                                                       # rows of a reference held at a time


def chunks(n):
    return [(r0, min(r0 + CHUNK, n)) for r0 in range(0, n, CHUNK)]


def device_layout(call, n, L, what, pad=3):
    """the [n, L] uint32 words a device form left in a sentinel-filled buffer of n + 2 rows and pitch L + pad; nothing outside
    the layout — corner, pitch columns, guard rows — is written"""
    flat, view = _sweep.device_words(n + 2, L + pad)
    call(view)
    return _sweep.read_words(flat, view, _sweep.lag_mask(n, L), what)


def dosage_rows(n, S, missing):
    """tests/_prune.py's rows with real LD; a constant row, and with missing values a row that misses everything"""
    G = _prune.ld_rows(n, S, 100 * n + S, missing=missing)
    G[n // 3] = 1
    if missing:
        G[n // 2] = 3
    return G


class DosageCase:
    """one StormDosage per (shape, missing share); what the library says about its pairs is fetched once, compared with the
    reference in row chunks, and kept for the LD-score and prune tests along with the reference's r^2"""

    def __init__(self, n, S, L, missing):
        self.n, self.S, self.L, self.missing = n, S, L, missing
        self.G = dosage_rows(n, S, missing)
        self.d = sb.StormDosage(S)
        for row in self.G:
            self.d.add(row)
        self.got, self.ref_r2 = None, None

    def pairs(self):
        """the six lag matrices on the device against the references; returns the library's words"""
        if self.got is not None:
            return self.got
        n, S, L, d = self.n, self.S, self.L, self.d
        got = {"dot": device_layout(lambda t: d.pairw_lag_dot(L, device=t), n, L, "pairw_lag_dot"),
               "nobs": device_layout(lambda t: d.pairw_lag_nobs(L, device=t), n, L, "pairw_lag_nobs")}
        for ms in ("r", "r2"):
            got["corr", ms] = device_layout(lambda t: d.pairw_lag_corr(L, ms, device=t), n, L, f"pairw_lag_corr {ms}")
            got["complete", ms] = device_layout(lambda t: d.pairw_lag_corr_complete(L, ms, device=t), n, L, f"pairw_lag_corr_complete {ms}")
        stats = _sweep.Stats()
        ref_r2 = {"corr": (np.zeros((n, L)), np.zeros((n, L), bool)), "complete": (np.zeros((n, L)), np.zeros((n, L), bool))}
        for r0, r1 in chunks(n):
            sums = _ld_scale.dosage_lag_sums(self.G, L, r0, r1)
            inside = _ld_scale.inside(n, L, r0, r1)
            _sweep.equal(got["dot"][r0:r1], sums["P"].astype(np.uint32), f"pairw_lag_dot rows {r0}..", inside)
            _sweep.equal(got["nobs"][r0:r1], sums["N"].astype(np.uint32), f"pairw_lag_nobs rows {r0}..", inside)
            for ms in ("r", "r2"):
                for name, ref in (("corr", _ld_scale.corr_plain_lag(sums, S, ms, L, r0, r1)),
                                  ("complete", _ld_scale.corr_complete_lag(sums, ms, L, r0, r1))):
                    _sweep.close_floats(stats, got[name, ms][r0:r1], ref[0], ref[1], inside, f"pairw_lag_{name} {ms} rows {r0}..")
                    if ms == "r2":
                        ref_r2[name][0][r0:r1], ref_r2[name][1][r0:r1] = ref
        print(f"dosage {n} x {S}, lag {L}, missing {self.missing}: worst ulp {stats.worst_ulp}")
        self.got, self.ref_r2 = got, ref_r2
        return got


_dosage_cases = {}


def dosage_case(n, S, L, missing):
    key = (n, S, L, missing)
    if key not in _dosage_cases:
        _dosage_cases[key] = DosageCase(*key)
    return _dosage_cases[key]


DOSAGE_SHAPES = [(2300, 96, 1100), (33000, 64, 40)]


def assert_reaches(n, S, L):
    words = (S + 31) // 32
    if n > 32768:
        assert (n + 127) // 128 > 256                                              # tile indices past 255 ...
        assert int(dist.lag_dosage_plan(n, words, L)[:, :2].max()) > 255           # ... in the plan of the launch
        assert int(dist.lag_dosage_plan(3 * n, words, 3 * L + 2)[:, :2].max()) > 3 * 255
    else:
        plan = dist.lag_dosage_plan(n, words, L).astype(np.int64)
        assert int((plan[:, 1] - plan[:, 0]).max()) == 9                           # nine tile columns behind the diagonal's
        assert 3 * L + 2 == 3302                                                   # the scratch pitch of the pairwise-complete finish


@pytest.mark.parametrize("missing", [0.0, 0.1])
@pytest.mark.parametrize("n,S,L", DOSAGE_SHAPES)
def test_dosage_lag_matrices_against_the_lag_layout_references(n, S, L, missing):
    assert_reaches(n, S, L)
    c = dosage_case(n, S, L, missing)
    got = c.pairs()
    if not missing:                                                                # without a 3 the complete form is the plain one
        for ms in ("r", "r2"):
            _sweep.equal(got["complete", ms], got["corr", ms], f"pairw_lag_corr_complete {ms} against pairw_lag_corr")
        assert (got["nobs"][_sweep.lag_mask(n, L)] == S).all()
    else:
        assert (got["nobs"][n // 2] == 0).all()                                    # the row that misses everything
    assert (got["corr", "r2"][n // 3][_sweep.lag_mask(n, L)[n // 3]] == _sweep.NAN_BITS).all()   # the constant row


@pytest.mark.parametrize("missing", [0.0, 0.1])
@pytest.mark.parametrize("n,S,L", DOSAGE_SHAPES)
def test_dosage_ldscores_inside_the_bound_over_the_checked_band(n, S, L, missing):
    """lag_ldscore, both statistics, plain and pairwise-complete: tests/_ldscore.py's band_sums over the library's own r^2 and
    N — the words test_dosage_lag_matrices_.. holds against the reference — inside _ldscore.bound, the counts exactly; the
    device form gives the host form's bits"""
    import torch
    c = dosage_case(n, S, L, missing)
    got = c.pairs()
    for complete in (False, True):
        band = got["complete" if complete else "corr", "r2"].view(np.float32)
        for stat in ("r2", "r2_adj"):
            ref, sum_abs, m = _ldscore.band_sums(band, n, L, STATS[stat], n_const=S, nobs=got["nobs"] if complete else None)
            score, pairs = c.d.lag_ldscore(L, stat, complete=complete)
            _ldscore.assert_scores(score, pairs, ref, sum_abs, m, (n, S, L, missing, complete, stat))
            d_score, d_pairs = vector_outputs(n)
            assert c.d.lag_ldscore(L, stat, complete=complete, device=(d_score, d_pairs)) is None
            torch.cuda.synchronize()
            dev, dev_pairs = d_score.cpu().numpy(), d_pairs.cpu().numpy().view(np.uint32)
            assert (dev[n:] == np.float32(GUARD_F)).all() and (dev_pairs[n:] == GUARD_I).all()
            _sweep.equal(_sweep.bits_of(dev[:n]), _sweep.bits_of(score), "lag_ldscore: the device form's bits")
            _sweep.equal(dev_pairs[:n], pairs, "lag_ldscore: the device form's n_pairs")
            assert pairs[n // 3] == 0 and m.max() > min(L, 64)


@pytest.mark.parametrize("missing", [0.0, 0.1])
@pytest.mark.parametrize("n,S,L", DOSAGE_SHAPES)
def test_dosage_prune_is_the_greedy_over_the_references_r2(n, S, L, missing):
    import torch
    c = dosage_case(n, S, L, missing)
    c.pairs()
    priority = np.random.default_rng(n + S).random(n, dtype=np.float32)
    for complete in (False, True):
        r2, nan = c.ref_r2["complete" if complete else "corr"]
        values = r2[_ld_scale.inside(n, L) & ~nan]
        min_r2 = _sweep.prune_threshold(values, 0.5)
        margin = _sweep.prune_margin(values, min_r2)
        print(f"prune {n} x {S}, lag {L}, missing {missing}, complete {complete}: min_r2 {float(min_r2)!r}, margin {margin:.3g}")
        assert margin >= _sweep.PRUNE_MARGIN, (margin, float(min_r2))              # a condition on the inputs
        i, j = _ld_scale.edges_above(r2, nan, min_r2, n, L)
        nb = _ld_scale.neighbours_of(n, i, j)
        for pr in (None, priority):
            where = (n, S, L, missing, complete, pr is not None)
            ref = _prune.greedy(nb, n, pr)
            if complete or not missing:                                            # (a 3 read as a value leaves the plain r^2 few edges)
                assert 0.15 <= ref[0].mean() <= 0.85, (where, ref[0].mean())
            assert_same(c.d.lag_prune(float(min_r2), L, priority=pr, complete=complete, owner=True), ref, where)
            d_keep = torch.full((n + GUARD,), GUARD_K, dtype=torch.uint8, device=DEV)
            d_owner = torch.full((n + GUARD,), GUARD_O, dtype=torch.int32, device=DEV)
            torch.cuda.synchronize()
            assert c.d.lag_prune(float(min_r2), L, priority=pr, complete=complete, device=(d_keep, d_owner)) is None
            keep, owner = d_keep.cpu().numpy(), d_owner.cpu().numpy().view(np.uint32)
            assert (keep[n:] == GUARD_K).all() and (owner[n:] == GUARD_O).all()
            assert_same((keep[:n], owner[:n]), ref, where + ("device",))


def test_hip_matrix_of_dosage_rows_at_lag_4096(hip_ctx):
    """8300 rows of 64 samples with a tenth missing, lag 4096: full windows at the README's largest lag; the
    pairwise-complete finish reads its nine products at a scratch pitch of 3 L + 2 = 12290"""
    from tests.test_gpu_dosage import pack
    n, S, L = 8300, 64, 4096
    assert 3 * L + 2 == 12290 and n - 2 * L > 0
    assert len(dist.lag_dosage_plan(3 * n, (S + 31) // 32, 3 * L + 2)) > 0
    G = dosage_rows(n, S, 0.1)
    m = hip_ctx.matrix_from_host(pack(G))
    try:
        def form(call):
            def run(t):
                call(t.data_ptr(), int(t.stride(0)))
                hip_ctx.synchronize()
            return run
        got = {"dot": device_layout(form(lambda p, ld: m.pairw_lag_dosage_matrix_device(p, ld, L)), n, L, "pairw_lag_dosage_matrix_device"),
               "nobs": device_layout(form(lambda p, ld: m.pairw_lag_dosage_nobs_device(p, ld, L, S)), n, L, "pairw_lag_dosage_nobs_device")}
        for ms in ("r", "r2"):
            got[ms] = device_layout(form(lambda p, ld: m.pairw_lag_dosage_corr_complete_device(p, ld, L, S, ms)), n, L,
                                    f"pairw_lag_dosage_corr_complete_device {ms}")
    finally:
        m.close()
    stats = _sweep.Stats()
    for r0, r1 in chunks(n):
        sums = _ld_scale.dosage_lag_sums(G, L, r0, r1)
        inside = _ld_scale.inside(n, L, r0, r1)
        _sweep.equal(got["dot"][r0:r1], sums["P"].astype(np.uint32), f"dot rows {r0}..", inside)
        _sweep.equal(got["nobs"][r0:r1], sums["N"].astype(np.uint32), f"nobs rows {r0}..", inside)
        for ms in ("r", "r2"):
            ref = _ld_scale.corr_complete_lag(sums, ms, L, r0, r1)
            _sweep.close_floats(stats, got[ms][r0:r1], ref[0], ref[1], inside, f"corr_complete {ms} rows {r0}..")
    print(f"HipMatrix dosage {n} x {S}, lag {L}: worst ulp {stats.worst_ulp}")


def bit_container(kind, D, M):
    s = sb.StormContig(M) if kind == "contig" else sb.Storm()
    for row in D:
        s.add(np.flatnonzero(row).astype(np.uint32))
    assert s.n_rows == D.shape[0]
    return s


@pytest.mark.parametrize("kind,n,M,L", [("contig", 2300, 1000, 1100), ("storm", 2300, 1000, 1100), ("contig", 33000, 100, 40)])
def test_bit_lag_counts_and_measures_against_the_lag_layout_references(kind, n, M, L):
    plan = dist.lag_plan(n, (M + 63) // 64, L).astype(np.int64)
    if n > 32768:
        assert (n + 127) // 128 > 256 and int(plan[:, :2].max()) > 255             # tile indices past 255
    else:
        assert int((plan[:, 1] - plan[:, 0]).max()) == 9                           # nine tile columns behind the diagonal's
    D = _sweep.random_bits_dense(np.random.default_rng(n + M), n, M)
    s = bit_container(kind, D, M)
    try:
        got = {op: device_layout(lambda t: s.pairw_lag_matrix_device(t.data_ptr(), n + 2, int(t.stride(0)), L, op), n, L,
                                 f"pairw_lag_matrix_device {op}") for op in _sweep.OPS}
        for ms in ("jaccard", "ld_r2"):
            got[ms] = device_layout(lambda t: s.pairw_lag_similarity_device(t.data_ptr(), n + 2, int(t.stride(0)), L, ms, n_bits=M), n, L,
                                    f"pairw_lag_similarity_device {ms}")
    finally:
        s.free()
    stats = _sweep.Stats()
    for r0, r1 in chunks(n):
        c, a = _ld_scale.bit_lag_counts(D, L, r0, r1)
        inside = _ld_scale.inside(n, L, r0, r1)
        for op, ref in _ld_scale.bit_lag_ops(c, a, L, r0, r1).items():
            _sweep.equal(got[op][r0:r1], ref.astype(np.uint32), f"{kind} pairw_lag_matrix {op} rows {r0}..", inside)
        for ms in ("jaccard", "ld_r2"):
            v, nan = _ld_scale.similarity_lag(ms, c, a, M, L, r0, r1)
            _sweep.close_floats(stats, got[ms][r0:r1], v, nan, inside, f"{kind} pairw_lag_similarity {ms} rows {r0}..")
    print(f"{kind} {n} x {M} bits, lag {L}: worst ulp {stats.worst_ulp}")
