#!/usr/bin/env python3
"""The dosage container against the route the library offered before it, for the same numbers: us per call into device
memory, S = 65536 samples of genotype-like dosages 0 / 1 / 2, per row count n:
  dot_us      STORM_dosage_pairw_dot_device: n rows of 2-bit values, K2h in its dosage form (one launch, n^2 / 2 pairs)
  planes_us   STORM_contig_pairw_matrix_device (op AND) on the 2 n-row container of the SAME data as bit planes (rows
              [0, n): the values' low bits, rows [n, 2 n): their high bits): about 2 n^2 pairs. The host combine
              P = ll + 2 lh + 2 hl + 4 hh that this route still needs is NOT timed, which favours it.
  corr_us     STORM_dosage_pairw_corr_device (r^2): the dot products, the rows' sums and the finishing pass
  finish_us   corr_us - dot_us: what the finishing pass (and the row sums) cost
Each figure: --calls back-to-back calls between two device events and a synchronise, divided by the calls; the routes
alternate within a round, --reps rounds after a warm-up; median and minimum. The two routes are checked against each other
on the device before anything is timed. `fp4_share`: pairs x S x 2 FLOP per dot_us against 10 PFLOP/s (the convention of
DESIGN.md §4; a call's time, not the kernel's: that comes from a kernel trace of `--only dosage`). One JSON line per n.
    python tools/bench_dosage.py [--rows 1024,4096] [--reps 9] [--calls 5] [--only dosage] > out.jsonl

--complete: rows with missing genotypes (5 % of the samples of every row carry the code 3) under the same protocol, in one
process:
  complete_us STORM_dosage_pairw_corr_complete_device (r^2): the split, two triangles and the rectangle [G ; H] x M on K2h
              (3 n^2 row-pair products), the finishing pass
  corr_us     STORM_dosage_pairw_corr_device on the same rows (3 read as a value: n^2 / 2 products) — what the missing
              genotypes cost over the complete-case call; the MFMA count predicts 6 x
  stacked_us  the route to the same sums without the rectangle: STORM_dosage_pairw_dot_device on the 3 n-row container
              [G ; H ; M] split on the host (4.5 n^2 products; the finishing pass this route still needs is NOT timed,
              which favours it); the MFMA count predicts complete_us = 0.67 x stacked_us
The r^2 of the complete call is checked against the stacked route's sums (float64 on the device) before anything is timed.
    python tools/bench_dosage.py --complete [--rows 1024,4096] > profiles/dosage_complete.jsonl"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stormbitmaps_amd as sb  # noqa: E402

S = 65536
PEAK_FP4 = 10e15


def pack2(G):
    out = np.empty((G.shape[0], G.shape[1] // 32), dtype=np.uint64)
    shifts = np.arange(32, dtype=np.uint64) * np.uint64(2)
    for r0 in range(0, G.shape[0], 256):
        v = G[r0:r0 + 256].reshape(-1, G.shape[1] // 32, 32).astype(np.uint64)
        out[r0:r0 + 256] = (v << shifts).sum(axis=2, dtype=np.uint64)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1024,4096")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--only", default="", help="'dosage': the dosage calls alone (a kernel trace of this form)")
    ap.add_argument("--complete", action="store_true", help="rows with missing genotypes: the pairwise-complete call")
    a = ap.parse_args()
    import torch
    lib = sb.load()

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} -> {rc}: {lib.STORM_hip_error().decode()}")

    if a.complete:
        return complete(a, lib, ok, torch)

    for n in [int(x) for x in a.rows.split(",")]:
        rng = np.random.default_rng(n)
        freq = rng.uniform(0.05, 0.5, size=(n, 1))
        G = np.empty((n, S), dtype=np.uint8)
        for r0 in range(0, n, 256):        # (in row blocks: the uniform draws are 8 bytes a sample)
            f = freq[r0:r0 + 256]
            G[r0:r0 + 256] = (rng.random((len(f), S)) < f).astype(np.uint8) + (rng.random((len(f), S)) < f).astype(np.uint8)
        d = lib.STORM_dosage_new(S)
        words = pack2(G)
        ok(lib.STORM_dosage_add_packed(d, words.ctypes.data, n), "STORM_dosage_add_packed")
        out = torch.zeros((n, n), dtype=torch.int32, device="cuda:0")
        fout = torch.zeros((n, n), dtype=torch.float32, device="cuda:0")
        calls = {"dot": lambda: ok(lib.STORM_dosage_pairw_dot_device(d, C.c_void_p(out.data_ptr()), n, n), "dot"),
                 "corr": lambda: ok(lib.STORM_dosage_pairw_corr_device(d, 0, C.c_void_p(fout.data_ptr()), n, n), "corr")}
        c = None
        if a.only != "dosage":
            c = lib.STORM_contig_new(S)
            for plane in (1, 2):
                for i in range(n):
                    pos = np.flatnonzero(G[i] & plane).astype(np.uint32)
                    if pos.size == 0:      # (an empty add appends no row: keep the row numbering)
                        raise RuntimeError("an empty bit-plane row: choose another seed")
                    assert lib.STORM_contig_add(c, pos.ctypes.data, pos.size) == pos.size
            planes = torch.zeros((2 * n, 2 * n), dtype=torch.int32, device="cuda:0")
            calls["planes"] = lambda: ok(lib.STORM_contig_pairw_matrix_device(c, 0, C.c_void_p(planes.data_ptr()), 2 * n, 2 * n),
                                         "planes")
        del G
        for fn in calls.values():          # warm-up: uploads, work lists, windows, code objects
            fn()
            fn()
        if c is not None:                  # the same numbers by both routes, compared on the device
            i, j = torch.triu_indices(n, n, 1, device="cuda:0")
            ll, hh = planes[i, j], planes[n + i, n + j]
            lh, hl = planes[i, n + j], planes[j, n + i]
            assert torch.equal(out[i, j], ll + 2 * lh + 2 * hl + 4 * hh)
            del i, j, ll, hh, lh, hl
        ts = {k: [] for k in calls}
        for _ in range(a.reps):            # alternating: a clock or a neighbour that drifts hits every route alike
            for k, fn in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                ts[k].append(e0.elapsed_time(e1) * 1e3 / a.calls)
        med = {k: statistics.median(v) for k, v in ts.items()}
        row = {"rows": n, "samples": S, "reps": a.reps, "calls": a.calls,
               "dot_us": round(med["dot"], 1), "corr_us": round(med["corr"], 1),
               "finish_us": round(med["corr"] - med["dot"], 1), "min_us": {k: round(min(v), 1) for k, v in ts.items()},
               "fp4_share": round(n * (n - 1) / 2 * S * 2 / (med["dot"] * 1e-6) / PEAK_FP4, 4)}
        if c is not None:
            row.update({"planes_us": round(med["planes"], 1), "planes_over_dot": round(med["planes"] / med["dot"], 3),
                        "not_slower": bool(med["dot"] <= med["planes"])})
            lib.STORM_contig_free(c)
        print(json.dumps(row), flush=True)
        lib.STORM_dosage_free(d)
        del out, fout


def timed(calls, reps, n_calls, torch):
    """median and minimum us per call of every route, the routes alternating within a round"""
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n_calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1) * 1e3 / n_calls)
    return {k: statistics.median(v) for k, v in ts.items()}, {k: round(min(v), 1) for k, v in ts.items()}


def complete(a, lib, ok, torch):
    for n in [int(x) for x in a.rows.split(",")]:
        rng = np.random.default_rng(n)
        freq = rng.uniform(0.05, 0.5, size=(n, 1))
        d, stacked = lib.STORM_dosage_new(S), lib.STORM_dosage_new(S)
        parts = {"g": [], "h": [], "m": []}
        for r0 in range(0, n, 256):        # (in row blocks: the uniform draws are 8 bytes a sample)
            f = freq[r0:r0 + 256]
            X = (rng.random((len(f), S)) < f).astype(np.uint8) + (rng.random((len(f), S)) < f).astype(np.uint8)
            X[rng.random((len(f), S)) < 0.05] = 3
            words = pack2(X)               # (held in a name: the call reads the array's memory)
            ok(lib.STORM_dosage_add_packed(d, words.ctypes.data, len(f)), "STORM_dosage_add_packed")
            parts["g"].append(pack2(np.where(X == 3, 0, X).astype(np.uint8)))
            parts["h"].append(pack2((X == 2).astype(np.uint8)))
            parts["m"].append(pack2((X != 3).astype(np.uint8)))
        del X
        for k in ("g", "h", "m"):
            words = np.concatenate(parts[k])
            ok(lib.STORM_dosage_add_packed(stacked, words.ctypes.data, n), "STORM_dosage_add_packed")
        del parts, words
        fout = torch.zeros((n, n), dtype=torch.float32, device="cuda:0")
        cout = torch.zeros((n, n), dtype=torch.float32, device="cuda:0")
        sout = torch.zeros((3 * n, 3 * n), dtype=torch.int32, device="cuda:0")
        calls = {"complete": lambda: ok(lib.STORM_dosage_pairw_corr_complete_device(d, 0, C.c_void_p(cout.data_ptr()), n, n),
                                        "complete"),
                 "corr": lambda: ok(lib.STORM_dosage_pairw_corr_device(d, 0, C.c_void_p(fout.data_ptr()), n, n), "corr"),
                 "stacked": lambda: ok(lib.STORM_dosage_pairw_dot_device(stacked, C.c_void_p(sout.data_ptr()), 3 * n, 3 * n),
                                       "stacked")}
        for fn in calls.values():          # warm-up: uploads, work lists, windows, code objects
            fn()
            fn()
        # the same r^2 from the stacked route's sums, in float64 on the device
        i, j = torch.triu_indices(n, n, 1, device="cuda:0")
        f64 = torch.float64
        P, N = sout[i, j].to(f64), sout[2 * n + i, 2 * n + j].to(f64)
        sx, sy = sout[i, 2 * n + j].to(f64), sout[j, 2 * n + i].to(f64)
        qx, qy = sx + 2 * sout[n + i, 2 * n + j].to(f64), sy + 2 * sout[n + j, 2 * n + i].to(f64)
        num, dx, dy = N * P - sx * sy, N * qx - sx * sx, N * qy - sy * sy
        want = (num * num / (dx * dy)).to(torch.float32)
        got = cout[i, j]
        defined = (dx != 0) & (dy != 0)
        assert bool(torch.isnan(got[~defined]).all()) and bool(defined.float().mean() > 0.99)
        assert bool(((got[defined] - want[defined]).abs() <= 2.4e-7 * want[defined].abs() + 1e-45).all())
        del i, j, P, N, sx, sy, qx, qy, num, dx, dy, want, got, defined
        med, low = timed(calls, a.reps, a.calls, torch)
        print(json.dumps({"rows": n, "samples": S, "missing": 0.05, "reps": a.reps, "calls": a.calls,
                          "complete_us": round(med["complete"], 1), "corr_us": round(med["corr"], 1),
                          "stacked_us": round(med["stacked"], 1), "min_us": low,
                          "complete_over_corr": round(med["complete"] / med["corr"], 3),
                          "complete_over_stacked": round(med["complete"] / med["stacked"], 3),
                          "not_slower_than_stacked": bool(med["complete"] <= med["stacked"])}), flush=True)
        lib.STORM_dosage_free(d)
        lib.STORM_dosage_free(stacked)
        del fout, cout, sout


if __name__ == "__main__":
    main()
