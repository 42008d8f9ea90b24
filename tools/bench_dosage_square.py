#!/usr/bin/env python3
"""r^2 between two dosage containers against the route the library offered before it, for the same numbers: us per call
into device memory, S = 65536 samples, 6.25 % of the samples of every row carrying the code 3, per shape n_a x n_b:
  square_us            STORM_dosage_square_corr_device (r^2): K2h over the rectangle (n_a n_b row-pair products), both
                       containers' row sums, the finishing pass
  square_complete_us   STORM_dosage_square_corr_complete_device (r^2): both splits, six n_a x n_b products on K2h in three
                       launches, the finishing pass
  stacked_us           STORM_dosage_pairw_corr_device on the container [a ; b] of n_a + n_b rows: (n_a + n_b)^2 / 2 products,
                       and an (n_a + n_b)^2 output of which the n_a x n_b block is wanted
  stacked_complete_us  STORM_dosage_pairw_corr_complete_device on the same container: 3 (n_a + n_b)^2 products
`products_ratio`: what the product counts alone predict for square_complete_us / stacked_complete_us,
6 n_a n_b / (3 (n_a + n_b)^2) (the plain form: n_a n_b against (n_a + n_b)^2 / 2, the same ratio). Each figure: --calls
back-to-back calls between two device events and a synchronise, divided by the calls; the routes alternate within a round,
--reps rounds after a warm-up; median and minimum. Before anything is timed the rectangle's floats are compared, bit for bit
on the device, with the block [0, n_a) x [n_a, n_a + n_b) of the stacked route's. The rows are drawn as packed words (values
0 / 1 / 2 / 3 with probabilities 7/16, 7/16, 1/16, 1/16 at every sample): what the calls cost does not depend on the values.
One JSON line per shape.
    python tools/bench_dosage_square.py [--shapes 256x8192,256x32768,4096x4096] [--reps 9] [--calls 5] > profiles/dosage_square.jsonl"""
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
LOW = np.uint64(0x5555555555555555)


def packed_rows(rng, n):
    """[n, S / 32] uint64: the low bit of a value with probability 1/2, the high bit with 1/8, independently"""
    out = np.empty((n, S // 32), dtype=np.uint64)
    for r0 in range(0, n, 1024):
        shape = (min(1024, n - r0), S // 32)
        r = [rng.integers(0, 1 << 64, size=shape, dtype=np.uint64) for _ in range(4)]
        out[r0:r0 + 1024] = (r[0] & LOW) | ((r[1] & r[2] & r[3] & LOW) << np.uint64(1))
    return out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x8192,256x32768,4096x4096")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    import torch
    lib = sb.load()
    if lib.storm_hip_device_count() < 1:
        raise RuntimeError("bench_dosage_square: no HIP device visible")

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} -> {rc}: {lib.STORM_hip_error().decode()}")

    for shape in a.shapes.split(","):
        na, nb = (int(x) for x in shape.split("x"))
        n = na + nb
        rng = np.random.default_rng([na, nb])
        da, db, stacked = lib.STORM_dosage_new(S), lib.STORM_dosage_new(S), lib.STORM_dosage_new(S)
        for d, rows in ((da, na), (db, nb)):
            words = packed_rows(rng, rows)     # (held in a name: the call reads the array's memory)
            ok(lib.STORM_dosage_add_packed(d, words.ctypes.data, rows), "STORM_dosage_add_packed")
            ok(lib.STORM_dosage_add_packed(stacked, words.ctypes.data, rows), "STORM_dosage_add_packed")
        del words
        sq = torch.zeros((na, nb), dtype=torch.float32, device="cuda:0")
        sqc = torch.zeros((na, nb), dtype=torch.float32, device="cuda:0")
        st = torch.zeros((n, n), dtype=torch.float32, device="cuda:0")
        stc = torch.zeros((n, n), dtype=torch.float32, device="cuda:0")
        calls = {
            "square": lambda: ok(lib.STORM_dosage_square_corr_device(da, db, 0, C.c_void_p(sq.data_ptr()), na, nb), "square"),
            "square_complete": lambda: ok(lib.STORM_dosage_square_corr_complete_device(da, db, 0, C.c_void_p(sqc.data_ptr()), na, nb),
                                          "square_complete"),
            "stacked": lambda: ok(lib.STORM_dosage_pairw_corr_device(stacked, 0, C.c_void_p(st.data_ptr()), n, n), "stacked"),
            "stacked_complete": lambda: ok(lib.STORM_dosage_pairw_corr_complete_device(stacked, 0, C.c_void_p(stc.data_ptr()), n, n),
                                           "stacked_complete")}
        for fn in calls.values():              # warm-up: uploads, work lists, scratch, code objects
            fn()
            fn()
        # the same floats by both routes, bit for bit, compared on the device
        assert torch.equal(sq.view(torch.int32), st[:na, na:].view(torch.int32)), "square_corr differs from the stacked route"
        assert torch.equal(sqc.view(torch.int32), stc[:na, na:].view(torch.int32)), "square_corr_complete differs from the stacked route"
        assert bool(torch.isfinite(sqc).float().mean() > 0.99)
        med, low = timed(calls, a.reps, a.calls, torch)
        print(json.dumps({"rows_a": na, "rows_b": nb, "samples": S, "missing": 0.0625, "reps": a.reps, "calls": a.calls,
                          "square_us": round(med["square"], 1), "square_complete_us": round(med["square_complete"], 1),
                          "stacked_us": round(med["stacked"], 1), "stacked_complete_us": round(med["stacked_complete"], 1),
                          "min_us": low, "products_ratio": round(6 * na * nb / (3 * n * n), 4),
                          "square_over_stacked": round(med["square"] / med["stacked"], 4),
                          "square_complete_over_stacked_complete": round(med["square_complete"] / med["stacked_complete"], 4)}),
              flush=True)
        for d in (da, db, stacked):
            lib.STORM_dosage_free(d)
        del sq, sqc, st, stc


if __name__ == "__main__":
    main()
