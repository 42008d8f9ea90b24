"""Every per-pair matrix call of the C-ABI comes as a pair: NAME_device writes a caller's device matrix, NAME writes host
memory through the context's band buffer. This file pins that the two forms of a pair write the SAME BITS, that the host
form writes `cols` entries per row and nothing behind them, and that neither leaves an error text — at the smallest shapes
at which the two forms can diverge. It is no test of the values (tests/test_gpu_similarity.py, test_gpu_dosage*.py,
test_gpu_lag_matrix.py, test_gpu_square.py and test_gpu_stage_edges.py check those against numpy); at 129 rows it only
asks that something other than zero was written, so that two forms that both did nothing do not pass.

One case = one pair at one shape:
  * the device form into a torch tensor of pitch ld = cols + 3 filled with zeros (what the form leaves alone — the entries
    i >= j of a triangle, the lower-right corner of the lag layout — is what the host form clears to zero), downloaded;
  * the host form into a numpy array of the same pitch filled with a sentinel;
  * entries [0, cols) of every row equal as uint32; entries [cols, ld) of the host rows still the sentinel;
  * storm_hip_last_error() empty. The text is per thread and is never cleared, and other files of the suite provoke errors
    on purpose, so every case makes its calls on a thread of its own.

Shapes: triangles of n = 0, 1, 2, 129 rows (129 crosses a 128-row tile; at n = 1 the device form returns at once and the
host form still writes its one zero); rectangles of 1 x 2 and 129 x 3; the lag layout for the same n and max_lag = 1, 5,
n - 1, n + 4 (those that are >= 1), cols = min(max_lag, n - 1). Bit rows of 3 words; dosage rows of 70 samples (3 words,
the last one ragged), a tenth of the genotypes missing for the nobs and pairwise-complete forms. The row-list forms start at
n = 1: a container without rows has no row lists. Every op, measure and statistic of a pair runs inside its case.

The calls go through ctypes, as in tests/test_gpu_streams_ld.py."""
import ctypes as C
import threading

import numpy as np
import pytest

import stormbitmaps_amd as sb
from tests.test_gpu_dosage import pack
from tests.test_gpu_stage_edges import Desc, NONE, _p

pytestmark = pytest.mark.gpu

WORDS, SAMPLES, PAD = 3, 70, 3
SENTINEL = 0xA5A5A5A5
ALL_ROWS = (1 << 64) - 1
TRIANGLES = (0, 1, 2, 129)
RECTANGLES = ((1, 2), (129, 3))
LAGS = tuple((n, L) for n in TRIANGLES for L in sorted({1, 5, n - 1, n + 4}) if L >= 1)
OPS, MEASURES, R_FORMS = (0, 1, 2), (0, 1, 2, 3), (0, 1)


def on_a_thread_of_its_own(fn):
    """fn() on a new thread; returns storm_hip_last_error() as that thread sees it afterwards"""
    box = {}

    def run():
        try:
            fn()
            box["error"] = sb._lib.last_error()
        except BaseException as e:   # noqa: BLE001 (handed to the test's thread)
            box["raised"] = e

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "raised" in box:
        raise box["raised"]
    return box["error"]


# ------------------------------------------------------------------------------------------ operands
def bit_rows(n, seed):
    return np.random.default_rng(seed).integers(0, 1 << 63, size=(n, WORDS), dtype=np.uint64)


def dosage_rows(n, seed, missing):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 3, size=(n, SAMPLES))
    if missing:
        g[rng.random((n, SAMPLES)) < 0.1] = 3
    return pack(g) if n else np.zeros((0, WORDS), dtype=np.uint64)   # (pack reshapes by n)


class Operands:
    """the matrices and row lists of one case, released at its end"""

    def __init__(self, ctx):
        self.ctx, self.mats, self.lists = ctx, [], []

    def matrix(self, rows):
        m = sb.HipMatrix(self.ctx, rows.shape[0], WORDS)
        self.mats.append(m)
        if rows.shape[0]:
            m.upload(rows)
        return m._h

    def rowlists(self, n, seed):
        """n rows of 1 .. 40 positions below 192, one list block each"""
        rng = np.random.default_rng(seed)
        d = Desc()
        for _ in range(n):
            d.block(0, 0, np.sort(rng.choice(64 * WORDS, size=int(rng.integers(1, 41)), replace=False)).astype(np.uint16), NONE)
            d.end_row()
        n_rows, n_blocks, off, ids, kinds, lens, ptrs, _ = d.arrays()
        h = C.c_void_p()
        sb._lib.check(self.ctx._lib.storm_hip_rowlists_create_blocks(self.ctx._h, n_rows, n_blocks, _p(off), _p(ids), _p(kinds),
                                                                     _p(lens), _p(ptrs), C.byref(h)), "storm_hip_rowlists_create_blocks")
        assert h.value, "a list-only container is eligible for the row lists"
        self.lists.append(h)
        return h

    def close(self):
        self.ctx.synchronize()
        for h in self.lists:
            self.ctx._lib.storm_hip_rowlists_destroy(self.ctx._h, h)
        for m in self.mats:
            m.close()


# ------------------------------------------------------------------------------------------ the pairs
# name -> (operands of a shape -> handles, [(label, device call, host call)]); a call: f(lib, ctx handle, handles, out, ld)
def _variants(args, device, host):
    return [(a, (lambda lib, c, h, out, ld, a=a: device(lib, c, h, a, out, ld)),
             (lambda lib, c, h, out, ld, a=a: host(lib, c, h, a, out, ld))) for a in args]


def _triangle_pairs():
    bits = lambda o, n: (o.matrix(bit_rows(n, 10 + n)),)                       # noqa: E731
    plain = lambda o, n: (o.matrix(dosage_rows(n, 20 + n, False)),)            # noqa: E731
    missing = lambda o, n: (o.matrix(dosage_rows(n, 30 + n, True)),)           # noqa: E731
    lists = lambda o, n: (o.rowlists(n, 40 + n),)                              # noqa: E731

    def band_host(lib, c, h, op, out, ld):
        return lib.storm_hip_pairw_matrix_band_begin(c, h[0], op, 0, lib.storm_hip_matrix_rows(h[0]), out, ld) or \
            lib.storm_hip_pairw_matrix_band_end(c)

    return {
        "pairw_matrix_band": (bits, _variants(
            OPS, lambda lib, c, h, op, out, ld: lib.storm_hip_pairw_matrix_band_device(c, h[0], op, 0, lib.storm_hip_matrix_rows(h[0]), out, ld),
            band_host)),
        "pairw_similarity": (bits, _variants(
            MEASURES, lambda lib, c, h, ms, out, ld: lib.storm_hip_pairw_similarity_device(c, h[0], ms, 64 * WORDS, out, ld),
            lambda lib, c, h, ms, out, ld: lib.storm_hip_pairw_similarity(c, h[0], ms, 64 * WORDS, out, ld))),
        "pairw_dosage_matrix": (plain, _variants(
            (None,), lambda lib, c, h, _, out, ld: lib.storm_hip_pairw_dosage_matrix_device(c, h[0], out, ld),
            lambda lib, c, h, _, out, ld: lib.storm_hip_pairw_dosage_matrix(c, h[0], out, ld))),
        "pairw_dosage_corr": (plain, _variants(
            R_FORMS, lambda lib, c, h, ms, out, ld: lib.storm_hip_pairw_dosage_corr_device(c, h[0], ms, SAMPLES, out, ld),
            lambda lib, c, h, ms, out, ld: lib.storm_hip_pairw_dosage_corr(c, h[0], ms, SAMPLES, out, ld))),
        "pairw_dosage_nobs": (missing, _variants(
            (None,), lambda lib, c, h, _, out, ld: lib.storm_hip_pairw_dosage_nobs_device(c, h[0], SAMPLES, out, ld),
            lambda lib, c, h, _, out, ld: lib.storm_hip_pairw_dosage_nobs(c, h[0], SAMPLES, out, ld))),
        "pairw_dosage_corr_complete": (missing, _variants(
            R_FORMS, lambda lib, c, h, ms, out, ld: lib.storm_hip_pairw_dosage_corr_complete_device(c, h[0], ms, SAMPLES, out, ld),
            lambda lib, c, h, ms, out, ld: lib.storm_hip_pairw_dosage_corr_complete(c, h[0], ms, SAMPLES, out, ld))),
        "rowlists_pairw_matrix": (lists, _variants(
            OPS, lambda lib, c, h, op, out, ld: lib.storm_hip_rowlists_pairw_matrix_device(c, h[0], op, out, ld),
            lambda lib, c, h, op, out, ld: lib.storm_hip_rowlists_pairw_matrix(c, h[0], op, out, ld))),
    }


def _rectangle_pairs():
    bits = lambda o, na, nb: (o.matrix(bit_rows(na, 50 + na)), o.matrix(bit_rows(nb, 60 + nb)))                        # noqa: E731
    plain = lambda o, na, nb: (o.matrix(dosage_rows(na, 70 + na, False)), o.matrix(dosage_rows(nb, 80 + nb, False)))   # noqa: E731
    lists = lambda o, na, nb: (o.rowlists(na, 90 + na), o.rowlists(nb, 100 + nb))                                      # noqa: E731
    return {
        "cross_dense_matrix": (bits, _variants(
            OPS, lambda lib, c, h, op, out, ld: lib.storm_hip_cross_dense_matrix_device(c, h[0], h[1], op, out, ld),
            lambda lib, c, h, op, out, ld: lib.storm_hip_cross_dense_matrix(c, h[0], h[1], op, out, ld))),
        "cross_dense_similarity": (bits, _variants(
            MEASURES, lambda lib, c, h, ms, out, ld: lib.storm_hip_cross_dense_similarity_device(c, h[0], h[1], ms, 64 * WORDS, out, ld),
            lambda lib, c, h, ms, out, ld: lib.storm_hip_cross_dense_similarity(c, h[0], h[1], ms, 64 * WORDS, out, ld))),
        "square_dosage_matrix": (plain, _variants(
            (None,), lambda lib, c, h, _, out, ld: lib.storm_hip_square_dosage_matrix_device(c, h[0], h[1], out, ld),
            lambda lib, c, h, _, out, ld: lib.storm_hip_square_dosage_matrix(c, h[0], h[1], out, ld))),
        "rowlists_square_matrix": (lists, _variants(
            OPS, lambda lib, c, h, op, out, ld: lib.storm_hip_rowlists_square_matrix_device(c, h[0], h[1], op, out, ld),
            lambda lib, c, h, op, out, ld: lib.storm_hip_rowlists_square_matrix(c, h[0], h[1], op, out, ld))),
    }


def _lag_pairs(L):
    bits = lambda o, n: (o.matrix(bit_rows(n, 110 + n)),)                      # noqa: E731
    plain = lambda o, n: (o.matrix(dosage_rows(n, 120 + n, False)),)           # noqa: E731
    missing = lambda o, n: (o.matrix(dosage_rows(n, 130 + n, True)),)          # noqa: E731
    return {
        "pairw_lag_matrix": (bits, _variants(
            OPS, lambda lib, c, h, op, out, ld: lib.storm_hip_pairw_lag_matrix_device(c, h[0], op, L, 0, ALL_ROWS, out, ld),
            lambda lib, c, h, op, out, ld: lib.storm_hip_pairw_lag_matrix(c, h[0], op, L, out, ld))),
        "pairw_lag_similarity": (bits, _variants(
            MEASURES, lambda lib, c, h, ms, out, ld: lib.storm_hip_pairw_lag_similarity_device(c, h[0], ms, 64 * WORDS, L, out, ld),
            lambda lib, c, h, ms, out, ld: lib.storm_hip_pairw_lag_similarity(c, h[0], ms, 64 * WORDS, L, out, ld))),
        "pairw_lag_dosage_matrix": (plain, _variants(
            (None,), lambda lib, c, h, _, out, ld: lib.storm_hip_pairw_lag_dosage_matrix_device(c, h[0], L, 0, ALL_ROWS, out, ld),
            lambda lib, c, h, _, out, ld: lib.storm_hip_pairw_lag_dosage_matrix(c, h[0], L, out, ld))),
        "pairw_lag_dosage_corr": (plain, _variants(
            R_FORMS, lambda lib, c, h, ms, out, ld: lib.storm_hip_pairw_lag_dosage_corr_device(c, h[0], ms, SAMPLES, L, out, ld),
            lambda lib, c, h, ms, out, ld: lib.storm_hip_pairw_lag_dosage_corr(c, h[0], ms, SAMPLES, L, out, ld))),
        "pairw_lag_dosage_nobs": (missing, _variants(
            (None,), lambda lib, c, h, _, out, ld: lib.storm_hip_pairw_lag_dosage_nobs_device(c, h[0], SAMPLES, L, out, ld),
            lambda lib, c, h, _, out, ld: lib.storm_hip_pairw_lag_dosage_nobs(c, h[0], SAMPLES, L, out, ld))),
        "pairw_lag_dosage_corr_complete": (missing, _variants(
            R_FORMS, lambda lib, c, h, ms, out, ld: lib.storm_hip_pairw_lag_dosage_corr_complete_device(c, h[0], ms, SAMPLES, L, out, ld),
            lambda lib, c, h, ms, out, ld: lib.storm_hip_pairw_lag_dosage_corr_complete(c, h[0], ms, SAMPLES, L, out, ld))),
    }


# ------------------------------------------------------------------------------------------ one case
def both_forms_agree(ctx, make, variants, shape, rows, cols, what):
    """the three assertions of this file for every variant of one pair at one shape (rows x cols entries)"""
    import torch
    lib, ld = ctx._lib, cols + PAD
    held = Operands(ctx)

    def calls():
        handles = make(held, *shape)
        for label, device, host in variants:
            d_out = torch.zeros((max(rows, 1), ld), dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()   # (the fill runs on torch's stream, the call on the context's)
            sb._lib.check(device(lib, ctx._h, handles, C.c_void_p(d_out.data_ptr()), ld), what + " (device form)")
            ctx.synchronize()
            dev = d_out.cpu().numpy().view(np.uint32)
            h_out = np.full((max(rows, 1), ld), SENTINEL, dtype=np.uint32)
            sb._lib.check(host(lib, ctx._h, handles, h_out.ctypes.data_as(C.c_void_p), ld), what + " (host form)")
            bad = np.argwhere(h_out[:rows, :cols] != dev[:rows, :cols])
            assert len(bad) == 0, (what, label, len(bad), [(int(i), int(j), hex(h_out[i, j]), hex(dev[i, j])) for i, j in bad[:5]])
            assert (h_out[:, cols:] == SENTINEL).all() and (h_out[rows:] == SENTINEL).all(), (what, label, "the host form wrote past its entries")
            assert not dev[:, cols:].any() and not dev[rows:].any(), (what, label, "the device form wrote past its entries")
            if rows >= 129:
                assert dev[:rows, :cols].any(), (what, label, "nothing was written")

    try:
        error = on_a_thread_of_its_own(calls)
    finally:
        held.close()
    assert error == "", (what, error)


@pytest.mark.parametrize("n", TRIANGLES)
@pytest.mark.parametrize("name", sorted(_triangle_pairs()))
def test_triangle_forms(hip_ctx, name, n):
    if name.startswith("rowlists") and n == 0:
        return   # (a container without rows has no row lists: storm_hip_rowlists_create_blocks hands back NULL)
    make, variants = _triangle_pairs()[name]
    both_forms_agree(hip_ctx, make, variants, (n,), n, n, "%s, %d rows" % (name, n))


def test_a_band_inside_the_triangle(hip_ctx):
    """storm_hip_pairw_matrix_band_device / _band_begin + _band_end on rows [1, 129) of 129: the band's rows from output row 0"""
    variants = _variants(OPS, lambda lib, c, h, op, out, ld: lib.storm_hip_pairw_matrix_band_device(c, h[0], op, 1, 128, out, ld),
                         lambda lib, c, h, op, out, ld: lib.storm_hip_pairw_matrix_band_begin(c, h[0], op, 1, 128, out, ld) or
                         lib.storm_hip_pairw_matrix_band_end(c))
    both_forms_agree(hip_ctx, lambda o, n: (o.matrix(bit_rows(n, 10 + n)),), variants, (129,), 128, 129, "pairw_matrix_band, rows 1 .. 128 of 129")


@pytest.mark.parametrize("shape", RECTANGLES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(_rectangle_pairs()))
def test_rectangle_forms(hip_ctx, name, shape):
    make, variants = _rectangle_pairs()[name]
    both_forms_agree(hip_ctx, make, variants, shape, shape[0], shape[1], "%s, %d x %d" % ((name,) + shape))


@pytest.mark.parametrize("n,L", LAGS)
@pytest.mark.parametrize("name", sorted(_lag_pairs(1)))
def test_lag_forms(hip_ctx, name, n, L):
    make, variants = _lag_pairs(L)[name]
    both_forms_agree(hip_ctx, make, variants, (n,), n, min(L, max(n - 1, 0)), "%s, %d rows, max_lag %d" % (name, n, L))
