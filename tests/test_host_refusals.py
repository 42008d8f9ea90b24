"""Every public entry point of the per-pair container calls (storm_square.c, storm_lag.c, storm_topk.c and the storm_dosage*.c
units) with each argument fault it refuses before a device is asked for, and the degenerate shapes that return 0 and write
nothing, through ctypes and without a GPU: the return code, the text of STORM_hip_error() where the call reports one (-3, -5)
and the bytes the call wrote are compared, word for word, with tests/golden/host_refusals.json. The fixture was recorded from
the build before the entry points were moved onto one call frame (`python -m tests.test_host_refusals --record` writes it
from whatever library is loaded); a change of a message, a code or the order of two checks shows here as a differing case."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "host_refusals.json")
SENTINEL = 0xA5
NAN, INF = float("nan"), float("inf")
TOPK_MAX, MAX_ANNOT = 128, 1024          # storm.h: STORM_TOPK_MAX, STORM_LDSCORE_MAX_ANNOT
BIG = (1 << 32) + 1                      # an n_bits beyond 2^32
DEV = ("", "_device")


class Session:
    """The containers the cases run on and the two output buffers every call is pointed at."""

    def __init__(self, lib):
        self.lib = lib
        self.results = {}
        self.bufs = [np.full(8192, SENTINEL, dtype=np.uint8) for _ in range(2)]
        self.o, self.o2 = (b.ctypes.data for b in self.bufs)
        self.keep = []
        # bit containers: 3 rows, 1 row, none
        self.c, self.c1, self.c0 = (self.contig(n) for n in (3, 1, 0))
        self.s, self.s1, self.s0 = (self.storm(n) for n in (3, 1, 0))
        # dosage containers: 5 rows, 1 row, none (40 samples); 2 rows of 41 samples; 1 row of 2 samples
        self.d, self.d1, self.d0 = (self.dosage(40, n) for n in (5, 1, 0))
        self.e = self.dosage(41, 2)
        self.few = self.dosage(2, 1)

    def contig(self, n):
        h = self.lib.STORM_contig_new(128)
        for r in range(n):
            pos = np.array([r, r + 7, 100], dtype=np.uint32)
            assert self.lib.STORM_contig_add(h, pos.ctypes.data, 3) >= 0
        return h

    def storm(self, n):
        h = self.lib.STORM_new()
        for r in range(n):
            pos = np.array([r, r + 7, 100], dtype=np.uint32)
            assert self.lib.STORM_add(h, pos.ctypes.data, 3) >= 0
        return h

    def dosage(self, n_samples, n):
        h = self.lib.STORM_dosage_new(n_samples)
        row = (np.arange(n_samples) % 3).astype(np.uint8)
        for _ in range(n):
            assert self.lib.STORM_dosage_add(h, row.ctypes.data, n_samples) == 0
        return h

    def arr(self, values, dtype):
        a = np.array(values, dtype=dtype)
        self.keep.append(a)
        return a.ctypes.data

    def case(self, fn, what, *args):
        key = f"{fn}: {what}"
        assert key not in self.results, key
        for b in self.bufs:
            b[:] = SENTINEL
        rc = getattr(self.lib, fn)(*args)
        rc = rc - (1 << 64) if rc >= (1 << 63) else rc      # (uint64_t)-1 as -1
        text = self.lib.STORM_hip_error().decode() if rc in (-3, -5) or (rc == -1 and "cardinality" in fn) else ""
        wrote = {f"out{i}[{j}]": int(b[j]) for i, b in enumerate(self.bufs) for j in np.flatnonzero(b != SENTINEL)}
        self.results[key] = {"rc": rc, "error": text, "wrote": wrote}

    def close(self):
        for h in (self.c, self.c1, self.c0):
            self.lib.STORM_contig_free(h)
        for h in (self.s, self.s1, self.s0):
            self.lib.STORM_free(h)
        for h in (self.d, self.d1, self.d0, self.e, self.few):
            self.lib.STORM_dosage_free(h)


def similarity_cases(t):
    o = t.o
    for kind, h, h0 in (("contig_pairw", t.c, t.c0), ("pairw", t.s, t.s0), ("square", t.s, t.s0)):
        two = kind == "square"
        for dev in DEV:
            fn = f"STORM_{kind}_similarity{dev}"
            H = lambda a, b=None: (a, a if b is None else b) if two else (a,)
            t.case(fn, "NULL handle", *H(None, h), 0, 0, o, 3, 3)
            if two:
                t.case(fn, "NULL second handle", h, None, 0, 0, o, 3, 3)
            t.case(fn, "NULL output", *H(h), 0, 0, None, 3, 3)
            t.case(fn, "out_rows too small", *H(h), 0, 0, o, 2, 3)
            t.case(fn, "out_ld too small", *H(h), 0, 0, o, 3, 2)
            t.case(fn, "measure -1", *H(h), -1, 0, o, 3, 3)
            t.case(fn, "measure 4", *H(h), 4, 0, o, 3, 3)
            t.case(fn, "too small and measure 4", *H(h), 4, 0, o, 2, 3)
            if kind != "contig_pairw":
                t.case(fn, "n_bits 0 with LD D", *H(h), 2, 0, o, 3, 3)
                t.case(fn, "n_bits 0 with LD r2", *H(h), 3, 0, o, 3, 3)
            t.case(fn, "n_bits beyond 2^32", *H(h), 3, BIG, o, 3, 3)
            t.case(fn, "empty", *H(h0), 0, 0, o, 0, 0)
            t.case(fn, "empty, LD measure refused all the same", *H(h0), 2, BIG, o, 0, 0)
            if two:
                t.case(fn, "b empty", h, h0, 0, 0, o, 3, 0)
                t.case(fn, "a empty", h0, h, 0, 0, o, 0, 3)


def square_matrix_cases(t):
    o = t.o
    for dev in DEV:
        fn = f"STORM_square_matrix{dev}"
        t.case(fn, "NULL handle", None, t.s, 0, o, 3, 3)
        t.case(fn, "NULL second handle", t.s, None, 0, o, 3, 3)
        t.case(fn, "NULL output", t.s, t.s, 0, None, 3, 3)
        t.case(fn, "out_rows too small", t.s, t.s, 0, o, 2, 3)
        t.case(fn, "out_ld too small", t.s, t.s1, 0, o, 3, 0)
        t.case(fn, "op -1", t.s, t.s, -1, o, 3, 3)
        t.case(fn, "op 3", t.s, t.s, 3, o, 3, 3)
        t.case(fn, "too small and op 3", t.s, t.s, 3, o, 2, 3)
        t.case(fn, "a empty", t.s0, t.s, 0, o, 0, 3)
        t.case(fn, "b empty", t.s, t.s0, 0, o, 3, 0)
        t.case(fn, "b empty and op 3", t.s, t.s0, 3, o, 3, 0)
    fn = "STORM_intersect_cardinality_square"
    t.case(fn, "NULL handle", None, t.s)
    t.case(fn, "NULL second handle", t.s, None)
    t.case(fn, "a empty", t.s0, t.s)
    t.case(fn, "b empty", t.s, t.s0)


def lag_cases(t):
    o = t.o
    for kind, h, h1, h0 in (("contig_pairw", t.c, t.c1, t.c0), ("pairw", t.s, t.s1, t.s0)):
        for dev in DEV:
            fn = f"STORM_{kind}_lag_matrix{dev}"
            t.case(fn, "NULL handle", None, 0, 1, o, 3, 2)
            t.case(fn, "NULL output", h, 0, 1, None, 3, 2)
            t.case(fn, "max_lag 0", h, 0, 0, o, 3, 2)
            t.case(fn, "out_rows too small", h, 0, 2, o, 2, 2)
            t.case(fn, "out_ld too small", h, 0, 2, o, 3, 1)
            t.case(fn, "out_ld too small for n - 1", h, 0, 9, o, 3, 1)
            t.case(fn, "op -1", h, -1, 1, o, 3, 2)
            t.case(fn, "op 3", h, 3, 1, o, 3, 2)
            t.case(fn, "too small and max_lag 0", h, 0, 0, o, 0, 0)
            t.case(fn, "too small and op 3", h, 3, 2, o, 2, 2)
            t.case(fn, "max_lag 0 and op 3", h, 3, 0, o, 3, 2)
            t.case(fn, "empty", h0, 0, 1, o, 0, 0)
            t.case(fn, "empty and max_lag 0", h0, 0, 0, o, 0, 0)
            t.case(fn, "one row", h1, 0, 4, o, 1, 0)
            t.case(fn, "one row and op 3", h1, 3, 4, o, 1, 0)
            fn = f"STORM_{kind}_lag_similarity{dev}"
            t.case(fn, "NULL handle", None, 0, 0, 1, o, 3, 2)
            t.case(fn, "NULL output", h, 0, 0, 1, None, 3, 2)
            t.case(fn, "max_lag 0", h, 0, 0, 0, o, 3, 2)
            t.case(fn, "out_rows too small", h, 0, 0, 2, o, 2, 2)
            t.case(fn, "out_ld too small", h, 0, 0, 2, o, 3, 1)
            t.case(fn, "measure -1", h, -1, 0, 1, o, 3, 2)
            t.case(fn, "measure 4", h, 4, 0, 1, o, 3, 2)
            t.case(fn, "too small and max_lag 0", h, 0, 0, 0, o, 0, 0)
            t.case(fn, "too small and measure 4", h, 4, 0, 2, o, 2, 2)
            t.case(fn, "max_lag 0 and measure 4", h, 4, 0, 0, o, 3, 2)
            if kind == "pairw":
                t.case(fn, "n_bits 0 with LD D", h, 2, 0, 1, o, 3, 2)
                t.case(fn, "n_bits 0 with LD r2", h, 3, 0, 1, o, 3, 2)
            t.case(fn, "n_bits beyond 2^32", h, 3, BIG, 1, o, 3, 2)
            t.case(fn, "empty", h0, 0, 0, 1, o, 0, 0)
            t.case(fn, "one row", h1, 1, 0, 4, o, 1, 0)
            t.case(fn, "one row, n_bits beyond 2^32", h1, 2, BIG, 4, o, 1, 0)


def topk_cases(t):
    o, o2 = t.o, t.o2
    for kind, h, h0 in (("contig_pairw", t.c, t.c0), ("pairw", t.s, t.s0), ("square", t.s, t.s0)):
        two = kind == "square"
        for dev in DEV:
            fn = f"STORM_{kind}_topk{dev}"
            H = lambda a, b=None: (a, a if b is None else b) if two else (a,)
            t.case(fn, "NULL handle", *H(None, h), 0, 0, 2, 0, o, o2, 3, 2)
            if two:
                t.case(fn, "NULL second handle", h, None, 0, 0, 2, 0, o, o2, 3, 2)
            t.case(fn, "NULL idx", *H(h), 0, 0, 2, 0, None, o2, 3, 2)
            t.case(fn, "NULL val", *H(h), 0, 0, 2, 0, o, None, 3, 2)
            t.case(fn, "out_rows too small", *H(h), 0, 0, 2, 0, o, o2, 2, 2)
            t.case(fn, "out_ld below k", *H(h), 0, 0, 2, 0, o, o2, 3, 1)
            t.case(fn, "score -1", *H(h), -1, 0, 2, 0, o, o2, 3, 2)
            t.case(fn, "score 5", *H(h), 5, 0, 2, 0, o, o2, 3, 2)
            t.case(fn, "k 0", *H(h), 0, 0, 0, 0, o, o2, 3, 2)
            t.case(fn, "k beyond STORM_TOPK_MAX", *H(h), 0, 0, TOPK_MAX + 1, 0, o, o2, 3, TOPK_MAX + 1)
            t.case(fn, "panel_rows 100", *H(h), 0, 0, 2, 100, o, o2, 3, 2)
            t.case(fn, "score 5 and k 0", *H(h), 5, 0, 0, 0, o, o2, 3, 2)
            t.case(fn, "k 0 and panel_rows 100", *H(h), 0, 0, 0, 100, o, o2, 3, 2)
            t.case(fn, "too small and score 5", *H(h), 5, 0, 2, 0, o, o2, 2, 2)
            t.case(fn, "panel_rows 100 and n_bits beyond 2^32", *H(h), 3, BIG, 2, 100, o, o2, 3, 2)
            if kind != "contig_pairw":
                t.case(fn, "n_bits 0 with LD D", *H(h), 2, 0, 2, 0, o, o2, 3, 2)
                t.case(fn, "n_bits 0 with LD r2", *H(h), 3, 0, 2, 0, o, o2, 3, 2)
            t.case(fn, "n_bits beyond 2^32", *H(h), 3, BIG, 2, 0, o, o2, 3, 2)
            t.case(fn, "empty", *H(h0), 4, 0, 2, 0, o, o2, 0, 2)
            t.case(fn, "empty and k 0", *H(h0), 4, 0, 0, 0, o, o2, 0, 2)
            if two:
                t.case(fn, "a empty", h0, h, 0, 0, 2, 0, o, o2, 0, 2)


def dosage_matrix_cases(t):
    o = t.o
    for stat in ("dot", "corr", "nobs", "corr_complete"):
        M = (0,) if "corr" in stat else ()
        bad = lambda m: (m,) if M else ()
        for dev in DEV:
            fn = f"STORM_dosage_pairw_{stat}{dev}"
            t.case(fn, "NULL handle", None, *M, o, 5, 5)
            t.case(fn, "NULL output", t.d, *M, None, 5, 5)
            t.case(fn, "out_rows too small", t.d, *M, o, 4, 5)
            t.case(fn, "out_ld too small", t.d, *M, o, 5, 4)
            if M:
                t.case(fn, "measure -1", t.d, -1, o, 5, 5)
                t.case(fn, "measure 2", t.d, 2, o, 5, 5)
                t.case(fn, "too small and measure 2", t.d, 2, o, 4, 5)
                t.case(fn, "one row and measure 2", t.d1, 2, o, 1, 1)
            t.case(fn, "empty", t.d0, *M, o, 0, 0)
            t.case(fn, "one row", t.d1, *M, o, 1, 1)
            fn = f"STORM_dosage_square_{stat}{dev}"
            t.case(fn, "NULL handle", None, t.d, *M, o, 5, 5)
            t.case(fn, "NULL second handle", t.d, None, *M, o, 5, 5)
            t.case(fn, "NULL output", t.d, t.d, *M, None, 5, 5)
            t.case(fn, "out_rows too small", t.d, t.d1, *M, o, 4, 1)
            t.case(fn, "out_ld too small", t.d, t.d1, *M, o, 5, 0)
            t.case(fn, "different n_samples", t.d, t.e, *M, o, 5, 2)
            t.case(fn, "too small and different n_samples", t.d, t.e, *M, o, 5, 1)
            if M:
                t.case(fn, "measure -1", t.d, t.d, -1, o, 5, 5)
                t.case(fn, "measure 2", t.d, t.d, 2, o, 5, 5)
                t.case(fn, "too small and measure 2", t.d, t.d, 2, o, 4, 5)
                t.case(fn, "different n_samples and measure 2", t.d, t.e, 2, o, 5, 2)
                t.case(fn, "b empty and measure 2", t.d, t.d0, 2, o, 5, 0)
            t.case(fn, "a empty", t.d0, t.d, *bad(0), o, 0, 5)
            t.case(fn, "b empty", t.d, t.d0, *bad(0), o, 5, 0)
            t.case(fn, "both empty, the same handle", t.d0, t.d0, *bad(0), o, 0, 0)
    t.case("STORM_dosage_row_sums", "NULL handle", None, t.o, t.o2)
    t.case("STORM_dosage_row_sums", "NULL sum", t.d, None, t.o2)
    t.case("STORM_dosage_row_sums", "NULL sum_sq", t.d, t.o, None)
    t.case("STORM_dosage_row_sums", "empty", t.d0, t.o, t.o2)
    t.case("STORM_dosage_row_missing", "NULL handle", None, t.o)
    t.case("STORM_dosage_row_missing", "NULL output", t.d, None)
    t.case("STORM_dosage_row_missing", "empty", t.d0, t.o)


def dosage_lag_cases(t):
    o = t.o
    for stat in ("dot", "corr", "nobs", "corr_complete"):
        M = (0,) if "corr" in stat else ()
        for dev in DEV:
            fn = f"STORM_dosage_pairw_lag_{stat}{dev}"
            t.case(fn, "NULL handle", None, *M, 2, o, 5, 2)
            t.case(fn, "NULL output", t.d, *M, 2, None, 5, 2)
            t.case(fn, "max_lag 0", t.d, *M, 0, o, 5, 2)
            t.case(fn, "out_rows too small", t.d, *M, 2, o, 4, 2)
            t.case(fn, "out_ld too small", t.d, *M, 2, o, 5, 1)
            t.case(fn, "out_ld too small for n - 1", t.d, *M, 9, o, 5, 3)
            t.case(fn, "too small and max_lag 0", t.d, *M, 0, o, 0, 0)
            if M:
                t.case(fn, "measure -1", t.d, -1, 2, o, 5, 2)
                t.case(fn, "measure 2", t.d, 2, 2, o, 5, 2)
                t.case(fn, "too small and measure 2", t.d, 2, 2, o, 4, 2)
                t.case(fn, "max_lag 0 and measure 2", t.d, 2, 0, o, 5, 2)
            t.case(fn, "empty", t.d0, *M, 2, o, 0, 0)
            t.case(fn, "empty and max_lag 0", t.d0, *M, 0, o, 0, 0)
            t.case(fn, "one row", t.d1, *M, 2, o, 1, 0)


def ldscore_cases(t):
    o, o2 = t.o, t.o2
    for complete in ("", "_complete"):
        for dev in DEV:
            fn = f"STORM_dosage_lag_ldscore{complete}{dev}"
            t.case(fn, "NULL handle", None, 0, 2, o, o2, 5)
            t.case(fn, "NULL score", t.d, 0, 2, None, o2, 5)
            t.case(fn, "max_lag 0", t.d, 0, 0, o, o2, 5)
            t.case(fn, "out_len too small", t.d, 0, 2, o, o2, 4)
            t.case(fn, "stat -1", t.d, -1, 2, o, o2, 5)
            t.case(fn, "stat 2", t.d, 2, 2, o, o2, 5)
            t.case(fn, "too small and max_lag 0", t.d, 0, 0, o, o2, 4)
            t.case(fn, "too small and stat 2", t.d, 2, 2, o, o2, 4)
            t.case(fn, "max_lag 0 and stat 2", t.d, 2, 0, o, o2, 5)
            t.case(fn, "adjusted statistic with 2 samples", t.few, 1, 2, o, o2, 1)
            t.case(fn, "empty", t.d0, 0, 2, o, None, 0)
            t.case(fn, "one row", t.d1, 1, 2, o, o2, 1)


def window_faults(t):
    """(what, max_lag, pos, max_dist) the window planner refuses on five rows"""
    return (("max_dist negative", 3, t.arr([0, 1, 2, 3, 4], np.float64), -1.0),
            ("max_dist NaN", 3, t.arr([0, 1, 2, 3, 4], np.float64), NAN),
            ("pos not finite", 3, t.arr([0, 1, NAN, 3, 4], np.float64), 1.0),
            ("pos infinite", 3, t.arr([0, 1, 2, 3, INF], np.float64), 1.0),
            ("pos decreasing", 3, t.arr([0, 1, 2, 1.5, 4], np.float64), 1.0),
            ("windows wider than max_lag", 2, t.arr([0, 1, 2, 3, 4], np.float64), 3.0))


def annot_cases(t):
    o, o2 = t.o, t.o2
    pos = t.arr([0, 1, 2, 3, 4], np.float64)
    bad_pos = t.arr([0, 1, 2, 1.5, 4], np.float64)
    an = t.arr(np.ones((5, 2)), np.float32)
    bad_an = np.ones((5, 2), dtype=np.float32)
    bad_an[3, 1] = np.inf
    bad_an[4, 0] = np.nan
    bad_an = t.arr(bad_an, np.float32)
    for complete in ("", "_complete"):
        for dev in DEV:
            fn = f"STORM_dosage_lag_ldscore_annot{complete}{dev}"
            t.case(fn, "NULL handle", None, 0, 2, None, 0.0, an, 2, 2, o, 2, o2, 5)
            t.case(fn, "NULL score", t.d, 0, 2, None, 0.0, an, 2, 2, None, 2, o2, 5)
            t.case(fn, "NULL annot", t.d, 0, 2, None, 0.0, None, 2, 2, o, 2, o2, 5)
            t.case(fn, "max_lag 0 without positions", t.d, 0, 0, None, 0.0, an, 2, 2, o, 2, o2, 5)
            t.case(fn, "out_rows too small", t.d, 0, 2, None, 0.0, an, 2, 2, o, 2, o2, 4)
            t.case(fn, "out_rows too small, max_lag 0 with positions", t.d, 0, 0, pos, 1.0, an, 2, 2, o, 2, o2, 4)
            t.case(fn, "too small and max_lag 0 without positions", t.d, 0, 0, None, 0.0, an, 2, 2, o, 2, o2, 4)
            t.case(fn, "stat -1", t.d, -1, 2, None, 0.0, an, 2, 2, o, 2, o2, 5)
            t.case(fn, "stat 2", t.d, 2, 2, None, 0.0, an, 2, 2, o, 2, o2, 5)
            t.case(fn, "too small and stat 2", t.d, 2, 2, None, 0.0, an, 2, 2, o, 2, o2, 4)
            t.case(fn, "adjusted statistic with 2 samples", t.few, 1, 2, None, 0.0, an, 2, 2, o, 2, o2, 1)
            t.case(fn, "n_annot 0", t.d, 0, 2, None, 0.0, an, 0, 2, o, 2, o2, 5)
            t.case(fn, "n_annot beyond STORM_LDSCORE_MAX_ANNOT", t.d, 0, 2, None, 0.0, an, MAX_ANNOT + 1, MAX_ANNOT + 1, o,
                   MAX_ANNOT + 1, o2, 5)
            t.case(fn, "stat 2 and n_annot 0", t.d, 2, 2, None, 0.0, an, 0, 2, o, 2, o2, 5)
            t.case(fn, "annot_ld too small", t.d, 0, 2, None, 0.0, an, 2, 1, o, 2, o2, 5)
            t.case(fn, "score_ld too small", t.d, 0, 2, None, 0.0, an, 2, 2, o, 1, o2, 5)
            t.case(fn, "n_annot 0 and score_ld too small", t.d, 0, 2, None, 0.0, an, 0, 2, o, 0, o2, 5)
            t.case(fn, "score_ld too small and pos decreasing", t.d, 0, 3, bad_pos, 1.0, an, 2, 2, o, 1, o2, 5)
            for what, max_lag, p, dist in window_faults(t):
                t.case(fn, what, t.d, 0, max_lag, p, dist, an, 2, 2, o, 2, o2, 5)
            if not dev:          # (a _device form's annot is device memory: it is not read here)
                t.case(fn, "annot not finite", t.d, 0, 2, None, 0.0, bad_an, 2, 2, o, 2, o2, 5)
                t.case(fn, "pos decreasing and annot not finite", t.d, 0, 3, bad_pos, 1.0, bad_an, 2, 2, o, 2, o2, 5)
                t.case(fn, "one row and annot not finite", t.d1, 0, 2, None, 0.0, t.arr([[1, NAN]], np.float32), 2, 2, o, 2, o2, 1)
            t.case(fn, "empty", t.d0, 0, 2, None, 0.0, an, 2, 2, o, 2, None, 0)
            t.case(fn, "empty, max_lag 0 with positions", t.d0, 0, 0, pos, 1.0, an, 2, 2, o, 2, o2, 0)
            t.case(fn, "one row", t.d1, 1, 2, None, 0.0, an, 2, 2, o, 2, o2, 1)
            t.case(fn, "one row with a position", t.d1, 0, 0, pos, 1.0, an, 2, 2, o, 2, o2, 1)


def prune_cases(t):
    o, o2 = t.o, t.o2
    pos = t.arr([0, 1, 2, 3, 4], np.float64)
    bad_pos = t.arr([0, 1, 2, 1.5, 4], np.float64)
    prio = t.arr([4, 3, 2, 1, 0], np.float32)
    nan_prio = t.arr([4, NAN, 2, 1, NAN], np.float32)
    for complete in ("", "_complete"):
        for dev in DEV:
            fn = f"STORM_dosage_lag_prune{complete}{dev}"
            t.case(fn, "NULL handle", None, 0.2, 2, None, 0.0, None, o, o2, 5)
            t.case(fn, "NULL keep", t.d, 0.2, 2, None, 0.0, None, None, o2, 5)
            t.case(fn, "max_lag 0 without positions", t.d, 0.2, 0, None, 0.0, None, o, o2, 5)
            t.case(fn, "out_len too small", t.d, 0.2, 2, None, 0.0, None, o, o2, 4)
            t.case(fn, "too small and max_lag 0 without positions", t.d, 0.2, 0, None, 0.0, None, o, o2, 4)
            t.case(fn, "too small ahead of everything behind it", t.d, NAN, 0, pos, -1.0, nan_prio, o, o2, 4)
            t.case(fn, "min_r2 NaN", t.d, NAN, 2, None, 0.0, None, o, o2, 5)
            t.case(fn, "min_r2 NaN and max_dist negative", t.d, NAN, 3, pos, -1.0, nan_prio, o, o2, 5)
            for what, max_lag, p, dist in window_faults(t):
                t.case(fn, what, t.d, 0.2, max_lag, p, dist, nan_prio, o, o2, 5)
            t.case(fn, "priority NaN", t.d, 0.2, 2, None, 0.0, nan_prio, o, None, 5)
            t.case(fn, "priority NaN with positions", t.d, 0.2, 0, pos, 3.0, nan_prio, o, o2, 5)
            t.case(fn, "pos decreasing and priority NaN", t.d, 0.2, 3, bad_pos, 1.0, nan_prio, o, o2, 5)
            t.case(fn, "empty", t.d0, 0.2, 2, None, 0.0, None, o, None, 0)
            t.case(fn, "empty with positions and priorities", t.d0, 0.2, 0, pos, 2.0, prio, o, o2, 0)
            t.case(fn, "empty, max_lag 0 without positions", t.d0, 0.2, 0, None, 0.0, None, o, o2, 5)
            if not dev:          # (one row, host form: kept, owns itself, no device is asked)
                t.case(fn, "one row", t.d1, 0.2, 2, None, 0.0, None, o, o2, 1)
                t.case(fn, "one row, no owner", t.d1, 0.2, 0, pos, 1.0, prio, o, None, 3)
                t.case(fn, "one row and priority NaN", t.d1, 0.2, 2, None, 0.0, t.arr([NAN], np.float32), o, o2, 1)


def dosage_topk_cases(t):
    o, o2 = t.o, t.o2
    for kind in ("pairw", "square"):
        two = kind == "square"
        for complete in ("", "_complete"):
            for dev in DEV:
                fn = f"STORM_dosage_{kind}_topk{complete}{dev}"
                H = lambda a, b=None: (a, a if b is None else b) if two else (a,)
                t.case(fn, "NULL handle", *H(None, t.d), 0, 2, 0, o, o2, 5, 2)
                if two:
                    t.case(fn, "NULL second handle", t.d, None, 0, 2, 0, o, o2, 5, 2)
                t.case(fn, "NULL idx", *H(t.d), 0, 2, 0, None, o2, 5, 2)
                t.case(fn, "NULL val", *H(t.d), 0, 2, 0, o, None, 5, 2)
                t.case(fn, "out_rows too small", *H(t.d), 0, 2, 0, o, o2, 4, 2)
                t.case(fn, "out_ld below k", *H(t.d), 0, 2, 0, o, o2, 5, 1)
                t.case(fn, "score -1", *H(t.d), -1, 2, 0, o, o2, 5, 2)
                t.case(fn, "score 3", *H(t.d), 3, 2, 0, o, o2, 5, 2)
                if complete:
                    t.case(fn, "score 2: no complete dot product", *H(t.d), 2, 2, 0, o, o2, 5, 2)
                t.case(fn, "k 0", *H(t.d), 0, 0, 0, o, o2, 5, 2)
                t.case(fn, "k beyond STORM_TOPK_MAX", *H(t.d), 0, TOPK_MAX + 1, 0, o, o2, 5, TOPK_MAX + 1)
                t.case(fn, "panel_rows 100", *H(t.d), 0, 2, 100, o, o2, 5, 2)
                t.case(fn, "score 3 and k 0", *H(t.d), 3, 0, 0, o, o2, 5, 2)
                t.case(fn, "k 0 and panel_rows 100", *H(t.d), 0, 0, 100, o, o2, 5, 2)
                t.case(fn, "too small and score 3", *H(t.d), 3, 2, 0, o, o2, 4, 2)
                if two:
                    t.case(fn, "different n_samples", t.d, t.e, 0, 2, 0, o, o2, 5, 2)
                    t.case(fn, "score 3 and different n_samples", t.d, t.e, 3, 2, 0, o, o2, 5, 2)
                    t.case(fn, "too small and different n_samples", t.d, t.e, 0, 2, 0, o, o2, 4, 2)
                    t.case(fn, "a empty", t.d0, t.d, 0, 2, 0, o, o2, 0, 2)
                    t.case(fn, "a empty and different n_samples", t.d0, t.e, 0, 2, 0, o, o2, 0, 2)
                t.case(fn, "empty", *H(t.d0), 0, 2, 0, o, o2, 0, 2)
                t.case(fn, "empty and k 0", *H(t.d0), 0, 0, 0, o, o2, 0, 2)


def container_cases(t):
    h = t.dosage(40, 1)
    good = t.arr(np.arange(40) % 4, np.uint8)
    four = t.arr([0] * 17 + [4] + [0] * 22, np.uint8)
    t.case("STORM_dosage_add", "NULL handle", None, good, 40)
    t.case("STORM_dosage_add", "NULL values", h, None, 40)
    t.case("STORM_dosage_add", "39 values for 40 samples", h, good, 39)
    t.case("STORM_dosage_add", "41 values for 40 samples", h, good, 41)
    t.case("STORM_dosage_add", "a value of 4", h, four, 40)
    words = t.arr([0x5555555555555555, 0x5555], np.uint64)
    beyond = t.arr([0, 0, 0x5555555555555555, 1 << 16], np.uint64)
    t.case("STORM_dosage_add_packed", "NULL handle", None, words, 1)
    t.case("STORM_dosage_add_packed", "NULL words", h, None, 1)
    t.case("STORM_dosage_add_packed", "no rows", h, words, 0)
    t.case("STORM_dosage_add_packed", "bits beyond the last sample", h, beyond, 2)
    assert t.lib.STORM_dosage_n_rows(h) == 1          # a refusal appends nothing
    t.case("STORM_dosage_clear", "NULL handle", None)
    t.case("STORM_dosage_n_rows", "NULL handle", None)
    t.lib.STORM_dosage_free(h)
    lag = C.cast(t.o, C.POINTER(C.c_uint64))
    fn = "STORM_ldscore_window_lag"
    pos = t.arr([0, 1, 2, 3, 4], np.float64)
    t.case(fn, "NULL lag", pos, 5, 1.0, None)
    t.case(fn, "NULL pos with rows", None, 5, 1.0, lag)
    t.case(fn, "no rows", None, 0, 1.0, lag)
    t.case(fn, "a lag of 2", pos, 5, 2.0, lag)
    for what, _, p, dist in window_faults(t)[:5]:
        t.case(fn, what, p, 5, dist, lag)


def several_slots_cases(t):
    """-5 ahead of every other check: three slots in view (the same device three times: nothing is asked of the hardware)"""
    o, o2 = t.o, t.o2
    pos = t.arr([0, 1, 2, 3, 4], np.float64)
    an = t.arr(np.ones((5, 2)), np.float32)
    calls = []
    for dev in DEV:
        calls += [(f"STORM_contig_pairw_similarity{dev}", (t.c, 9, 0, o, 0, 0)), (f"STORM_pairw_similarity{dev}", (t.s, 9, 0, o, 0, 0)),
                  (f"STORM_square_similarity{dev}", (t.s, t.s, 9, 0, o, 0, 0)),
                  (f"STORM_contig_pairw_lag_matrix{dev}", (t.c, 9, 0, o, 0, 0)), (f"STORM_pairw_lag_matrix{dev}", (t.s, 9, 0, o, 0, 0)),
                  (f"STORM_contig_pairw_lag_similarity{dev}", (t.c, 9, 0, 0, o, 0, 0)),
                  (f"STORM_pairw_lag_similarity{dev}", (t.s, 9, 0, 0, o, 0, 0)),
                  (f"STORM_contig_pairw_topk{dev}", (t.c, 9, 0, 0, 0, o, o2, 0, 0)), (f"STORM_pairw_topk{dev}", (t.s, 9, 0, 0, 0, o, o2, 0, 0)),
                  (f"STORM_square_topk{dev}", (t.s, t.s, 9, 0, 0, 0, o, o2, 0, 0))]
        for stat in ("dot", "corr", "nobs", "corr_complete"):
            M = (9,) if "corr" in stat else ()
            calls += [(f"STORM_dosage_pairw_{stat}{dev}", (t.d, *M, o, 0, 0)), (f"STORM_dosage_square_{stat}{dev}", (t.d, t.e, *M, o, 0, 0)),
                      (f"STORM_dosage_pairw_lag_{stat}{dev}", (t.d, *M, 0, o, 0, 0))]
        for complete in ("", "_complete"):
            calls += [(f"STORM_dosage_lag_ldscore{complete}{dev}", (t.d, 9, 0, o, o2, 0)),
                      (f"STORM_dosage_lag_ldscore_annot{complete}{dev}", (t.d, 9, 0, pos, -1.0, an, 0, 0, o, 0, o2, 0)),
                      (f"STORM_dosage_lag_prune{complete}{dev}", (t.d, NAN, 0, pos, -1.0, None, o, o2, 0)),
                      (f"STORM_dosage_pairw_topk{complete}{dev}", (t.d, 9, 0, 100, o, o2, 0, 0)),
                      (f"STORM_dosage_square_topk{complete}{dev}", (t.d, t.e, 9, 0, 100, o, o2, 0, 0))]
    calls += [("STORM_square_matrix_device", (t.s, t.s, 9, o, 0, 0)), ("STORM_dosage_row_sums", (t.d0, o, o2)),
              ("STORM_dosage_row_missing", (t.d0, o))]
    assert t.lib.STORM_hip_set_devices(3, (C.c_int * 3)(0, 0, 0)) == 0
    try:
        for fn, args in calls:
            t.case(fn, "three device slots in view, every argument wrong", *args)
    finally:
        assert t.lib.STORM_hip_set_devices(1, (C.c_int * 1)(0)) == 0


def run_cases(lib):
    t = Session(lib)
    for group in (similarity_cases, square_matrix_cases, lag_cases, topk_cases, dosage_matrix_cases, dosage_lag_cases, ldscore_cases,
                  annot_cases, prune_cases, dosage_topk_cases, container_cases, several_slots_cases):
        group(t)
    t.close()
    return t.results


def test_every_refusal_and_degenerate_shape_is_the_recorded_one(lib):
    with open(FIXTURE) as f:
        want = json.load(f)
    got = run_cases(lib)
    assert sorted(got) == sorted(want)
    differing = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not differing, differing
    # what the cases are: a refusal says who refuses, and only the one-row prune and the window's lag write anything
    for key, r in want.items():
        fn = key.split(":")[0]
        if r["rc"] in (-3, -5):
            assert r["error"].startswith(fn + ":"), key
        if r["wrote"]:
            assert r["rc"] == 0 and ("prune" in fn or fn == "STORM_ldscore_window_lag"), key
    assert {r["rc"] for r in want.values()} == {0, -1, -2, -3, -4, -5}


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, ROOT)
    import stormbitmaps_amd as sb
    recorded = run_cases(sb.load())
    with open(FIXTURE, "w") as f:
        json.dump(recorded, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(recorded)} cases -> {FIXTURE}")
