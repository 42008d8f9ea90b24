#!/usr/bin/env python3
"""The lag layout against the full triangle: us per synchronous call into device memory (launch + completion included),
M = 65536 dense, per row count and max_lag:
  lag_us        storm_hip_pairw_lag_matrix_device, op AND (tile128_kernel, lag form)
  lag_sim_us    storm_hip_pairw_lag_similarity_device (LD r^2): counts + row counts + finish_lag_tiles_kernel<SimilarityStat>
  finish_us     lag_sim_us - lag_us: the finish pass (and the row counts) alone
  triangle_us   storm_hip_pairw_matrix_device for the whole triangle of the same matrix, same process, alternating with the
                lag calls (the automatic kernel choice; `triangle_kernel` says which ran)
  tile_ratio    lag tiles / triangle tiles of 128 x 128 from the planners (about 2 (L + 128) / n): what lag_us / triangle_us
                is to be held against. Wherever it is <= 0.5 the lag call must be the faster one (`faster`).
Medians of --reps alternating rounds after a warm-up; the minimum beside them. One JSON line per (rows, max_lag).
The context keeps ONE work list: in a round `lag` follows `triangle` and so plans and uploads its list again inside its timed
window, `lag_sim` follows `lag` and finds it — lag_us is the dearer of the two by that much, finish_us too small by it.
    python tools/bench_lag_matrix.py [--rows 8192,32768] [--lags 128,512,1024,4096] [--reps 15] > out.jsonl"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stormbitmaps_amd as sb  # noqa: E402
from stormbitmaps_amd import dist  # noqa: E402

M = 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="8192,32768")
    ap.add_argument("--lags", default="128,512,1024,4096")
    ap.add_argument("--reps", type=int, default=15)
    a = ap.parse_args()
    import torch
    ctx = sb.HipContext(0)
    n_cus = ctx.get_option("n_cus")
    for n in [int(x) for x in a.rows.split(",")]:
        m = ctx.matrix(n, M // 64)
        m.fill_synthetic(M, M // 2, seed=42)
        tri = torch.zeros((n, n), dtype=torch.int32, device="cuda:0")
        tri_tiles = len({(int(i), int(j)) for i, j in dist.matrix_plan(n, M // 64, n_cus=n_cus)[:, :2]})
        for max_lag in [int(x) for x in a.lags.split(",")]:
            L = min(max_lag, n - 1)
            out = torch.zeros((n, L), dtype=torch.int32, device="cuda:0")
            calls = {"lag": lambda: m.pairw_lag_matrix_device(out.data_ptr(), L, max_lag, "and"),
                     "lag_sim": lambda: m.pairw_lag_similarity_device(out.data_ptr(), L, max_lag, "ld_r2", M),
                     "triangle": lambda: m.pairw_matrix_device(tri.data_ptr(), n, "and")}
            for fn in calls.values():      # warm-up: work lists, windows, code objects
                fn()
                fn()
            tri_kernel = None
            ts = {k: [] for k in calls}
            for _ in range(a.reps):        # alternating: a clock or a neighbour that drifts hits every call alike
                for k, fn in calls.items():
                    t0 = time.perf_counter()
                    fn()
                    ts[k].append((time.perf_counter() - t0) * 1e6)
                    if k == "triangle":
                        tri_kernel = ctx.get_option("k2_tile_shape_used")
            # the same numbers: the lag matrix against the triangle just written, on the device
            m.pairw_lag_matrix_device(out.data_ptr(), L, max_lag, "and")
            i = torch.arange(n, device="cuda:0")[:, None]
            j = i + 1 + torch.arange(L, device="cuda:0")[None, :]
            ok = j < n
            assert torch.equal(out[ok], tri[i.expand_as(j)[ok], j[ok]])
            med = {k: statistics.median(v) for k, v in ts.items()}
            lag_tiles = len({(int(x), int(y)) for x, y in dist.lag_plan(n, M // 64, max_lag, n_cus=n_cus)[:, :2]})
            ratio = lag_tiles / tri_tiles
            print(json.dumps({"rows": n, "bits": M, "max_lag": max_lag, "reps": a.reps,
                              "lag_us": round(med["lag"], 1), "lag_sim_us": round(med["lag_sim"], 1),
                              "finish_us": round(med["lag_sim"] - med["lag"], 1), "triangle_us": round(med["triangle"], 1),
                              "triangle_kernel": tri_kernel, "min_us": {k: round(min(v), 1) for k, v in ts.items()},
                              "lag_tiles": lag_tiles, "triangle_tiles": tri_tiles, "tile_ratio": round(ratio, 4),
                              "time_ratio": round(med["lag"] / med["triangle"], 4),
                              "faster": bool(med["lag"] < med["triangle"]), "must_be_faster": ratio <= 0.5}), flush=True)
            del out
        del tri
        m.close()
    ctx.close()


if __name__ == "__main__":
    main()
