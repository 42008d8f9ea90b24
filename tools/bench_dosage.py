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
    python tools/bench_dosage.py [--rows 1024,4096] [--reps 9] [--calls 5] [--only dosage] > out.jsonl"""
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
    a = ap.parse_args()
    import torch
    lib = sb.load()

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} -> {rc}: {lib.STORM_hip_error().decode()}")

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


if __name__ == "__main__":
    main()
