"""Per-row top-k neighbours of dosage rows selected on the device (storm.h: STORM_dosage_pairw_topk, STORM_dosage_square_topk,
their _complete and _device forms; storm_hip.h: storm_hip_dosage_topk_rows_device and the forms above it): for each row the
k best rows by r^2, r or the dot product, value descending, then row index ascending; NaN entries are no candidates; short
rows are padded.

Expected values come from code that shares nothing with the selection: r / r^2 from the library's existing host forms
STORM_dosage_square_corr and _square_corr_complete (a against a for the pairw forms), the dot products from numpy on the
unpacked rows (3 an ordinary value). `rank` and `top` of tests/test_gpu_topk.py order them by the rule above; idx and val must
be EQUAL to that, bit for bit, no tolerance. Device outputs are pre-filled with a sentinel: columns [k, ld_k) and one row
beyond the output must still hold it (`into_device`)."""
import ctypes as C

import numpy as np
import pytest

import stormbitmaps_amd as sb
from tests.test_gpu_dosage import pack
from tests.test_gpu_lag_matrix import SENTINEL, device_buffer, read_back, report
from tests.test_gpu_similarity import NAN_BITS
from tests.test_gpu_topk import NO_INDEX, assert_topk, into_device, last_pass, rank, ties_across, top
# the streams, the context born on one of them and the backlog of tests/test_gpu_streams.py (one instance per importing module)
from tests.test_gpu_streams import held, st, sw, sw_module  # noqa: F401

pytestmark = pytest.mark.gpu

SCORES = ("r2", "r", "dot")                          # STORM_DOSAGE_R2, STORM_DOSAGE_R, STORM_DOSAGE_TOPK_DOT
RAN_TILES_OUT, RAN_TOPK = 128, 1024
ALL = (1 << 64) - 1


# ------------------------------------------------------------------------------------------ helpers
def kind(score):
    """how tests/test_gpu_topk.py's rank / top read the values: integers, or float bits with the NaN pattern"""
    return "count" if score == "dot" else score


def container(G):
    d = sb.StormDosage(G.shape[1])
    if G.shape[0]:
        d.add_packed(pack(np.ascontiguousarray(G, dtype=np.uint8)))
    return d


def values(a, b, Ga, Gb, score, complete=False):
    """[n_a, n_b] uint32 of every row of a against every row of b, from the calls the selection shares nothing with"""
    if score == "dot":
        assert not complete
        return (Ga.astype(np.int64) @ Gb.astype(np.int64).T).astype(np.uint32)
    if Ga.shape[0] == 0 or Gb.shape[0] == 0:
        return np.zeros((Ga.shape[0], Gb.shape[0]), dtype=np.uint32)
    return np.ascontiguousarray(a.square_corr(b, score, complete=complete)).view(np.uint32)


def call_device(a, b, score, k, complete=False, panel_rows=0):
    """the C call of the _device form, b None: the pairw form; for into_device with out_rows = n + 1"""
    lib = sb.load()
    name = ("STORM_dosage_pairw_topk" if b is None else "STORM_dosage_square_topk") + ("_complete" if complete else "") + "_device"
    handles = (a._h,) if b is None else (a._h, b._h)
    n = a.n_rows

    def call(di, dv, ld_k):
        rc = getattr(lib, name)(*handles, SCORES.index(score), k, panel_rows, C.c_void_p(di), C.c_void_p(dv), n + 1, ld_k)
        assert rc == 0, (name, rc, lib.STORM_hip_error())
    return call


def device_form(a, b, score, k, ld_k, **kw):
    call = call_device(a, b, score, k, **kw)
    return into_device(lambda di, dv: call(di, dv, ld_k), a.n_rows, k, ld_k)


def host_form(a, b, score, k, **kw):
    return a.pairw_topk(k, score, **kw) if b is None else a.square_topk(b, k, score, **kw)


# ------------------------------------------------------------------------------------------ 1. tile edges, ties, NaN
CONSTANT, DUPLICATES = (17, 140), ((250, 10), (251, 77), (252, 200))


@pytest.fixture(scope="module")
def edge300():
    """300 rows x 1000 samples of 0 .. 2 (two 128-row tiles and 44 rows; one sweep step): rows 17 and 140 constant — NaN
    against everyone — and three rows copies of three others: r^2 = 1 between them and equal values against everyone else.
    Per score the whole expected order, pairw (skip0 = 0) and square against itself, computed once."""
    rng = np.random.default_rng(3001)
    G = rng.integers(0, 3, size=(300, 1000), dtype=np.uint8)
    G[CONSTANT[0]], G[CONSTANT[1]] = 0, 2
    for dst, src in DUPLICATES:
        G[dst] = G[src]
    d = container(G)
    vals = {score: values(d, d, G, G, score) for score in SCORES}
    ranked = {(score, form): rank(vals[score], kind(score), skip0=0 if form == "pairw" else None)
              for score in SCORES for form in ("pairw", "square")}
    yield d, G, vals, ranked
    d.free()


@pytest.mark.parametrize("k", [1, 8, 128])
@pytest.mark.parametrize("score", SCORES)
@pytest.mark.parametrize("form", ["pairw", "square"])
def test_tile_edges_ties_and_nan(edge300, form, score, k):
    d, _, vals, ranked = edge300
    r = ranked[score, form]
    if form == "pairw":
        # with this generator 3 / 1 / 1 rows (r2), 2 / 2 / 1 rows (r) and 1 / 83 / 220 rows (dot) tie across position 1 / 8 / 128
        assert ties_across(r, k) >= 1, (score, k)
    want = top(r, k, kind(score))
    b = None if form == "pairw" else d
    for ld_k in (k, k + 3):
        assert_topk(device_form(d, b, score, k, ld_k), want, (form, score, k, ld_k))
    idx, val = host_form(d, b, score, k)
    assert val.dtype == (np.uint32 if score == "dot" else np.float32) and idx.shape == val.shape == (300, k)
    assert_topk((idx, val), want, (form, score, k, "host"))
    if form == "pairw":
        assert (idx != np.arange(300)[:, None]).all()                       # a row never lists itself
    if score != "dot":
        for c in CONSTANT:                                                    # all padding, and listed nowhere
            assert (idx[c] == NO_INDEX).all() and (val.view(np.uint32)[c] == NAN_BITS).all() and not (idx == c).any()
        if score == "r2" and form == "pairw":
            for x, y in DUPLICATES:                                           # a copy is the best neighbour: r^2 = 1
                assert idx[x, 0] == y and idx[y, 0] == x and val[x, 0] == 1.0


# ------------------------------------------------------------------------------------------ 2. fewer candidates than k
@pytest.mark.parametrize("complete", [False, True])
def test_fewer_candidates_than_k(complete):
    rng = np.random.default_rng(52)
    S, k = 333, 8
    G5, G3 = rng.integers(0, 3, size=(5, S), dtype=np.uint8), rng.integers(0, 3, size=(3, S), dtype=np.uint8)
    five, three, one, none = container(G5), container(G3), container(G5[:1]), container(G5[:0])
    try:
        for score in SCORES[:2] if complete else SCORES:
            pad = 0 if score == "dot" else NAN_BITS
            kw = dict(complete=complete)
            want = top(rank(values(five, five, G5, G5, score, complete), kind(score), skip0=0), k, kind(score))
            assert (want[0][:, :4] != NO_INDEX).all() and (want[0][:, 4:] == NO_INDEX).all() and (want[1][:, 4:] == pad).all()
            assert_topk(device_form(five, None, score, k, k + 2, **kw), want, (score, "pairw"))
            assert_topk(host_form(five, None, score, k, **kw), want, (score, "pairw", "host"))
            want = top(rank(values(five, three, G5, G3, score, complete), kind(score)), k, kind(score))
            assert (want[0][:, :3] != NO_INDEX).all() and (want[0][:, 3:] == NO_INDEX).all()
            assert_topk(device_form(five, three, score, k, k, **kw), want, (score, "square"))
            assert_topk(host_form(five, three, score, k, **kw), want, (score, "square", "host"))
            # one row among itself, and an empty b: k paddings per row
            for a, b in ((one, None), (five, none)):
                for idx, val in (device_form(a, b, score, k, k + 1, **kw), host_form(a, b, score, k, **kw)):
                    assert idx.shape == (a.n_rows, k) and (idx == NO_INDEX).all() and (val.view(np.uint32) == pad).all(), score
            # an empty a: 0, nothing written
            _, vi = device_buffer(2, k)
            call_device(none, five, score, k, **kw)(vi.data_ptr(), vi.data_ptr(), k)
            assert (read_back(vi, 2, k) == SENTINEL).all()
            assert host_form(none, five, score, k, **kw)[0].shape == (0, k)
    finally:
        for x in (five, three, one, none):
            x.free()


# ------------------------------------------------------------------------------------------ 3. sweep steps, tail, forced sorts
@pytest.fixture(scope="module")
def wide():
    """40 rows against 2501 at 96 samples: three sweep steps of 1024 columns, a tail that is no multiple of 4"""
    rng = np.random.default_rng(2501)
    Ga = rng.integers(0, 4, size=(40, 96), dtype=np.uint8)
    Gb = rng.integers(0, 4, size=(2501, 96), dtype=np.uint8)
    a, b = container(Ga), container(Gb)
    yield a, b, Ga, Gb
    a.free()
    b.free()


@pytest.mark.parametrize("complete", [False, True])
def test_several_sweep_steps_and_the_tail(wide, complete):
    a, b, Ga, Gb = wide
    for score in SCORES[:2] if complete else SCORES:
        ranked = rank(values(a, b, Ga, Gb, score, complete), kind(score))
        for k in (1, 128):
            want = top(ranked, k, kind(score))
            assert_topk(device_form(a, b, score, k, k + 1, complete=complete), want, (score, k, complete))
        assert_topk(host_form(a, b, score, 8, complete=complete), top(ranked, 8, kind(score)), (score, "host", complete))


@pytest.mark.parametrize("ld,off", [(2504, 0), (2501, 1)])
def test_primitive_on_a_panel_of_the_callers(hip_ctx, wide, ld, off):
    """the dot products with their sums at a base 16-byte aligned with ld % 4 == 0 (128-bit loads), and one word off a 16-byte
    boundary with an odd ld (entry by entry); the pitch columns are never read; alone the report is RAN_TOPK"""
    import torch
    a, b, Ga, Gb = wide
    na, nb, S, k = 40, 2501, 96, 16
    dots = (Ga.astype(np.int64) @ Gb.astype(np.int64).T).astype(np.uint32)
    pitched = np.full((na, ld), 0xABCDEF01, dtype=np.uint32)
    pitched[:, :nb] = dots
    flat, view = device_buffer(na, ld, off)
    view[:na * ld] = torch.from_numpy(pitched.reshape(-1).view(np.int32)).to("cuda:0")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to("cuda:0")
    sa, qa = dev(Ga.astype(np.int64).sum(1)), dev((Ga.astype(np.int64) ** 2).sum(1))
    sb_, qb = dev(Gb.astype(np.int64).sum(1)), dev((Gb.astype(np.int64) ** 2).sum(1))
    torch.cuda.synchronize()
    m = hip_ctx.matrix(0, 3)
    try:
        for score in SCORES:
            vals = values(a, b, Ga, Gb, score)
            for skip0 in (None, 5):
                want = top(rank(vals, kind(score), skip0=skip0), k, kind(score))
                got = into_device(lambda di, dv: (m.dosage_topk_rows_device(view.data_ptr(), ld, na, nb, sa.data_ptr(), qa.data_ptr(),
                                                                            sb_.data_ptr(), qb.data_ptr(), S, di, dv, k + 1, k, score,
                                                                            skip0=skip0), hip_ctx.synchronize()), na, k, k + 1)
                assert report(hip_ctx) == [RAN_TOPK, 0, 0, 0]
                assert_topk(got, want, (score, skip0, ld, off))
        assert np.array_equal(read_back(view, na, ld), pitched)               # the panel is unchanged
        if off:
            assert (flat[:off].cpu().numpy().view(np.uint32) == SENTINEL).all()
        # refusals: nothing launched, the report stays
        lib, h, p = sb.load(), hip_ctx._h, C.c_void_p(view.data_ptr())
        s = [C.c_void_p(t.data_ptr()) for t in (sa, qa, sb_, qb)]
        _, out = device_buffer(na, 4)
        o = C.c_void_p(out.data_ptr())
        good = [p, ld, na, nb, *s, S, ALL, 0, 4, o, o, 4]
        for at, bad in ((0, None), (4, None), (7, None), (12, None), (13, None), (10, 3), (10, -1), (8, 0), (8, (1 << 24) + 1),
                        (11, 0), (11, 129), (14, 3), (1, nb - 1)):
            args = list(good)
            args[at] = bad
            assert lib.storm_hip_dosage_topk_rows_device(h, *args) == -1 and sb._lib.last_error(), (at, bad)
        assert lib.storm_hip_dosage_topk_rows_device(None, *good) == -1
        hip_ctx.synchronize()
        assert (read_back(out, na, 4) == SENTINEL).all()
    finally:
        m.close()


def test_every_step_ends_in_a_sort():
    """column j is the query (values 0 and 2) with its last 2500 - j samples zeroed, at 2560 samples: the dot product, r and
    r^2 with the query never descend with the column (they stand still where the added sample is a 0: runs of equal values
    that the index decides), so that every step of the sweep brings entries that beat the threshold of the last sort and ends
    in a sort. Then the columns reversed: only the first step stages anything."""
    rng = np.random.default_rng(2560)
    S, nb = 2560, 2501
    q = (2 * rng.integers(0, 2, size=S)).astype(np.uint8)
    Gb = np.where(np.arange(S)[None, :] < (S - 2500 + np.arange(nb))[:, None], q[None, :], 0).astype(np.uint8)
    Ga = np.concatenate([q[None, :], rng.integers(0, 3, size=(7, S), dtype=np.uint8)])
    a = container(Ga)
    try:
        for order in ("ascending", "descending"):
            Gx = np.ascontiguousarray(Gb if order == "ascending" else Gb[::-1])
            b = container(Gx)
            try:
                for score in SCORES:
                    vals = values(a, b, Ga, Gx, score)
                    row = vals[0].astype(np.float64) if score == "dot" else vals[0].view(np.float32).astype(np.float64)
                    step = np.diff(row)
                    assert (step >= 0).all() if order == "ascending" else (step <= 0).all(), (order, score)
                    ranked = rank(vals, kind(score))
                    for k in (1, 128):
                        assert_topk(device_form(a, b, score, k, k), top(ranked, k, kind(score)), (order, score, k))
            finally:
                b.free()
    finally:
        a.free()


# ------------------------------------------------------------------------------------------ 4. panels
@pytest.mark.parametrize("complete", [False, True])
def test_panels(complete):
    """600 rows, panel_rows 256: panels of 256, 256 and 88 rows, each against all 600 columns, the later ones excluding the
    row itself at skip0 = 256 and 512; equal to panel_rows 0 bit for bit"""
    rng = np.random.default_rng(600)
    n, S, k = 600, 200, 16
    G = rng.integers(0, 3, size=(n, S), dtype=np.uint8)
    if complete:
        G[rng.random((n, S)) < 0.1] = 3
    d = container(G)
    try:
        for score in SCORES[:2] if complete else SCORES:
            want = top(rank(values(d, d, G, G, score, complete), kind(score), skip0=0), k, kind(score))
            paneled = device_form(d, None, score, k, k, complete=complete, panel_rows=256)
            whole = device_form(d, None, score, k, k, complete=complete, panel_rows=0)
            assert_topk(paneled, want, (score, 256))
            assert_topk(whole, want, (score, 0))
            assert_topk(host_form(d, None, score, k, complete=complete, panel_rows=512), want, (score, 512, "host"))
            assert (paneled[0] != np.arange(n)[:, None]).all()
        # the square form in panels: rows 300 .. 599 against rows 0 .. 299
        a, b = container(G[300:]), container(G[:300])
        try:
            want = top(rank(values(a, b, G[300:], G[:300], "r2", complete), "r2"), k, "r2")
            assert_topk(host_form(a, b, "r2", k, complete=complete, panel_rows=256), want, "square, 256")
        finally:
            a.free()
            b.free()
    finally:
        d.free()


# ------------------------------------------------------------------------------------------ 5. missing genotypes
def test_missing_genotypes():
    """300 rows x 200 samples, about a tenth coded 3; row 5 entirely missing; rows 6 and 7 share exactly one sample; row 8 is
    constant on the samples it shares with row 9"""
    rng = np.random.default_rng(3200)
    n, S, k = 300, 200, 12
    G = rng.integers(0, 3, size=(n, S), dtype=np.uint8)
    G[rng.random((n, S)) < 0.1] = 3
    G[5] = 3
    G[6, 1:], G[7, :100] = 3, 3
    G[6, 0], G[7, 0] = 1, 2                                                   # sample 0 alone is shared
    G[9, 100:] = 3
    G[8, :100] = np.where(G[9, :100] == 3, G[8, :100], 1)                     # constant where row 9 is present
    assert ((G[6] != 3) & (G[7] != 3)).sum() == 1 and len(set(G[8][(G[8] != 3) & (G[9] != 3)])) == 1
    d = container(G)
    clean = np.where(G == 3, 0, G).astype(np.uint8)
    c = container(clean)
    try:
        for score in ("r2", "r"):
            vals = values(d, d, G, G, score, complete=True)
            assert (vals[5] == NAN_BITS).all() and vals[6, 7] == NAN_BITS and vals[8, 9] == NAN_BITS
            for form, b, skip0 in (("pairw", None, 0), ("square", d, None)):
                want = top(rank(vals, score, skip0=skip0), k, score)
                got = device_form(d, b, score, k, k + 1, complete=True)
                assert_topk(got, want, (score, form))
                assert_topk(host_form(d, b, score, k, complete=True), want, (score, form, "host"))
                assert (got[0][5] == NO_INDEX).all() and not (got[0] == 5).any()
            # no 3 anywhere: the complete forms are the plain forms, bit for bit
            plain = device_form(c, None, score, k, k)
            assert_topk(device_form(c, None, score, k, k, complete=True), plain, (score, "complete == plain"))
            assert_topk(plain, top(rank(values(c, c, clean, clean, score), score, skip0=0), k, score), (score, "plain"))
    finally:
        d.free()
        c.free()


# ------------------------------------------------------------------------------------------ 6. reports and streams
def test_last_pass_report(hip_ctx):
    rng = np.random.default_rng(61)
    S, na, nb, k = 100, 300, 70, 4
    Ga, Gb = rng.integers(0, 4, size=(na, S), dtype=np.uint8), rng.integers(0, 4, size=(nb, S), dtype=np.uint8)
    a, b = hip_ctx.matrix_from_host(pack(Ga)), hip_ctx.matrix_from_host(pack(Gb))
    d = container(Ga)
    try:
        w = a.n_words
        a.pairw_dosage_topk(S, k, "dot")
        assert report(hip_ctx) == [RAN_TILES_OUT | RAN_TOPK, na * na * w, 0, 0]
        a.pairw_dosage_topk(S, k, "r2", complete=True, panel_rows=256)
        assert report(hip_ctx) == [RAN_TILES_OUT | RAN_TOPK, 6 * na * na * w, 0, 0]
        idx, val = b.cross_dosage_topk(a, S, k, "r")
        assert report(hip_ctx) == [RAN_TILES_OUT | RAN_TOPK, nb * na * w, 0, 0]
        assert_topk((idx, val), top(rank(np.ascontiguousarray(container_corr(Gb, Ga, "r")), "r"), k, "r"), "cross r")
        a.cross_dosage_topk(b, S, k, "r2", complete=True)
        assert report(hip_ctx) == [RAN_TILES_OUT | RAN_TOPK, 6 * na * nb * w, 0, 0]
        # refusals of the shim: the codes of check_square, check_samples and check_topk
        lib = sb.load()
        host = np.full((na, k), SENTINEL, dtype=np.uint32)
        p = host.ctypes.data_as(C.c_void_p)
        for panel_rows in (100, 255, 257):
            assert lib.storm_hip_pairw_dosage_topk(hip_ctx._h, a._h, 0, S, k, panel_rows, p, p, k) == -1 and sb._lib.last_error()
        assert lib.storm_hip_pairw_dosage_topk(hip_ctx._h, a._h, 3, S, k, 0, p, p, k) == -1
        assert lib.storm_hip_pairw_dosage_topk_complete(hip_ctx._h, a._h, 2, S, k, 0, p, p, k) == -1
        assert lib.storm_hip_pairw_dosage_topk(hip_ctx._h, a._h, 0, S + 32, k, 0, p, p, k) == -1
        assert lib.storm_hip_pairw_dosage_topk(hip_ctx._h, a._h, 0, S, 129, 0, p, p, 129) == -1
        assert lib.storm_hip_pairw_dosage_topk(hip_ctx._h, a._h, 0, S, k, 0, p, p, k - 1) == -1
        assert (host == SENTINEL).all()
        # through storm.h
        d.pairw_topk(3, "r2")
        assert last_pass() == RAN_TILES_OUT | RAN_TOPK
    finally:
        a.close()
        b.close()
        d.free()


def container_corr(Ga, Gb, measure):
    a, b = container(Ga), container(Gb)
    try:
        return a.square_corr(b, measure).view(np.uint32)
    finally:
        a.free()
        b.free()


def test_device_forms_are_complete_on_return(sw, held, st):
    """the context born on a caller's stream, behind a backlog on it: the outputs are read under another stream at once"""
    rng = np.random.default_rng(62)
    S, n, k = 96, 300, 8
    G = rng.integers(0, 3, size=(n, S), dtype=np.uint8)
    G[rng.random((n, S)) < 0.1] = 3
    m = held.matrix(sw.ctx, pack(G))
    d = container(G)
    try:
        want = {c: top(rank(values(d, d, G, G, "r2", c), "r2", skip0=0), k, "r2") for c in (False, True)}
    finally:
        d.free()
    lib = sb.load()
    for complete in (False, True):
        name = "storm_hip_pairw_dosage_topk" + ("_complete" if complete else "") + "_device"
        warm = st.full(st.s1, (2, n, k))
        assert getattr(lib, name)(sw.ctx._h, m._h, 0, S, k, 0, C.c_void_p(warm[0].data_ptr()), C.c_void_p(warm[1].data_ptr()), k) == 0
        st.drain()
        idx, val = st.full(st.s1, (n, k)), st.full(st.s1, (n, k))
        sw.backlog()
        assert getattr(lib, name)(sw.ctx._h, m._h, 0, S, k, 0, C.c_void_p(idx.data_ptr()), C.c_void_p(val.data_ptr()), k) == 0
        got = st.read(idx).view(np.uint32), st.read(val).view(np.uint32)
        assert_topk(got, want[complete], name)
        st.drain()


def test_primitive_is_ordered_behind_a_write_on_the_callers_stream(sw, held, st):
    """the panel holds a decoy; behind a backlog on the caller's stream the real dot products are copied over it ON that stream
    and the primitive is queued at once: it must select over what the copy wrote"""
    torch = st.torch
    rng = np.random.default_rng(63)
    S, na, nb, k = 96, 64, 700, 8
    Ga, Gb = rng.integers(0, 3, size=(na, S), dtype=np.uint8), rng.integers(0, 3, size=(nb, S), dtype=np.uint8)
    dots = (Ga.astype(np.int64) @ Gb.astype(np.int64).T).astype(np.uint32)
    want = top(rank(container_corr(Ga, Gb, "r2"), "r2"), k, "r2")
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to("cuda:0")
    real, panel = dev(dots), dev(rng.permutation(dots.reshape(-1)).reshape(na, nb))
    sums = [dev(x) for x in (Ga.astype(np.int64).sum(1), (Ga.astype(np.int64) ** 2).sum(1), Gb.astype(np.int64).sum(1),
                             (Gb.astype(np.int64) ** 2).sum(1))]
    m = held(sw.ctx.matrix(0, 3))
    idx, val = st.full(st.s1, (na, k)), st.full(st.s1, (na, k))
    st.drain()
    sw.backlog()
    with torch.cuda.stream(st.s1):
        panel.copy_(real)
    m.dosage_topk_rows_device(panel.data_ptr(), nb, na, nb, *(t.data_ptr() for t in sums), S, idx.data_ptr(), val.data_ptr(), k, k, "r2")
    st.drain()
    assert_topk((idx.cpu().numpy().view(np.uint32), val.cpu().numpy().view(np.uint32)), want, "behind the copy")


# ------------------------------------------------------------------------------------------ 7. the Python surface
def test_python_surface():
    import torch
    rng = np.random.default_rng(71)
    S, k = 150, 5
    Ga, Gb = rng.integers(0, 4, size=(140, S), dtype=np.uint8), rng.integers(0, 4, size=(75, S), dtype=np.uint8)
    a, b = container(Ga), container(Gb)
    try:
        for score in SCORES:
            for complete in (False, True) if score != "dot" else (False,):
                for other, Gx, skip0 in ((None, Ga, 0), (b, Gb, None)):
                    want = top(rank(values(a, a if other is None else other, Ga, Gx, score, complete), kind(score), skip0=skip0), k,
                               kind(score))
                    args = (k, score) if other is None else (other, k, score)
                    f = a.pairw_topk if other is None else a.square_topk
                    idx, val = f(*args, complete=complete)
                    assert isinstance(idx, np.ndarray) and idx.dtype == np.uint32
                    assert val.dtype == (np.uint32 if score == "dot" else np.float32)
                    assert_topk((idx, val), want, (score, complete, "host"))
                    ti, tv = f(*args, complete=complete, panel_rows=256, device="cuda:0")
                    assert ti.is_cuda and tv.is_cuda and tuple(ti.shape) == tuple(tv.shape) == (140, k)
                    assert ti.dtype == torch.int32 and tv.dtype == (torch.int32 if score == "dot" else torch.float32)
                    assert_topk((ti.cpu().numpy().view(np.uint32), tv.cpu().numpy().view(np.uint32)), want, (score, complete, "device"))
        with pytest.raises(RuntimeError):
            a.pairw_topk(k, "r2", panel_rows=100)
        with pytest.raises(KeyError):
            a.pairw_topk(k, "jaccard")
    finally:
        a.free()
        b.free()
