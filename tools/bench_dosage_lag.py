#!/usr/bin/env python3
"""The dosage form in the lag layout against the n x n dosage calls: us per synchronous call into device memory (launch +
completion included), S = 65536 samples of random codes 0 .. 3 (a quarter of them 3: missing, for the calls that read it
so), per row count and max_lag:
  lag_dot_us        storm_hip_pairw_lag_dosage_matrix_device (tile128_kernel<true, 2>)
  lag_corr_us       storm_hip_pairw_lag_dosage_corr_device: dot products + row sums + finish_lag_tiles_kernel<DosageStat>
  lag_complete_us   storm_hip_pairw_lag_dosage_corr_complete_device: interleaved split, ONE launch over 3 n rows at lag
                    3 L + 2, dosage_complete_finish_lag_kernel
  complete_over_corr  lag_complete_us / lag_corr_us: the cost of the interleaved layout (the MFMA count predicts about 9)
  full_dot_us, full_complete_us   storm_hip_pairw_dosage_matrix_device / _corr_complete_device on the same matrix, same
                    process, alternating with the lag calls; only up to --full-max-rows rows (the n x n output and about 3 n^2
                    words of scratch: 4 + 12 GiB at 32768 rows), null beyond
  tile_ratio        lag tiles / triangle tiles of 128 x 128 from the planners: wherever it is <= 0.5 the lag call must be the
                    faster one of its pair (`dot_faster`, `complete_faster`)
Medians of --reps alternating rounds after a warm-up; the minimum beside them. One JSON line per (rows, max_lag). The context
keeps ONE work list, so every call of a round plans and uploads its list again inside its timed window (the forms alternate).
    python tools/bench_dosage_lag.py [--rows 8192,32768] [--lags 128,1024,4096] [--reps 9] > profiles/dosage_lag.jsonl"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stormbitmaps_amd as sb  # noqa: E402
from stormbitmaps_amd import dist  # noqa: E402
from stormbitmaps_amd._lib import check  # noqa: E402

S = 65536


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="8192,32768")
    ap.add_argument("--lags", default="128,1024,4096")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--full-max-rows", type=int, default=8192)
    a = ap.parse_args()
    import torch
    lib = sb.load()
    ctx = sb.HipContext(0)
    n_cus = ctx.get_option("n_cus")
    n_words = S // 32
    for n in [int(x) for x in a.rows.split(",")]:
        words = torch.randint(-(1 << 62), 1 << 62, (n, n_words), dtype=torch.int64, device="cuda:0")
        words = words * 2 + torch.randint(0, 2, (n, n_words), dtype=torch.int64, device="cuda:0")   # all 64 bits random
        m = ctx.matrix(n, n_words)
        m.import_device(words.data_ptr(), n, n_words)
        ctx.synchronize()
        del words
        full = n <= a.full_max_rows
        tri = torch.zeros((n, n), dtype=torch.int32, device="cuda:0") if full else None
        tri_tiles = len({(int(i), int(j)) for i, j in dist.dosage_plan(n, n_words, n_cus=n_cus)[:, :2]})
        for max_lag in [int(x) for x in a.lags.split(",")]:
            L = min(max_lag, n - 1)
            out = torch.zeros((n, L), dtype=torch.int32, device="cuda:0")
            calls = {"lag_dot": lambda: m.pairw_lag_dosage_matrix_device(out.data_ptr(), L, max_lag),
                     "lag_corr": lambda: m.pairw_lag_dosage_corr_device(out.data_ptr(), L, max_lag, S, "r2"),
                     "lag_complete": lambda: m.pairw_lag_dosage_corr_complete_device(out.data_ptr(), L, max_lag, S, "r2")}
            if full:
                calls["full_complete"] = lambda: check(lib.storm_hip_pairw_dosage_corr_complete_device(
                    ctx._h, m._h, 0, S, C.c_void_p(tri.data_ptr()), n), "storm_hip_pairw_dosage_corr_complete_device")
                calls["full_dot"] = lambda: check(lib.storm_hip_pairw_dosage_matrix_device(
                    ctx._h, m._h, C.c_void_p(tri.data_ptr()), n), "storm_hip_pairw_dosage_matrix_device")
            for fn in calls.values():      # warm-up: work lists, windows, scratch, code objects
                fn()
                fn()
            ts = {k: [] for k in calls}
            for _ in range(a.reps):        # alternating: a clock or a neighbour that drifts hits every call alike
                for k, fn in calls.items():
                    t0 = time.perf_counter()
                    fn()
                    ts[k].append((time.perf_counter() - t0) * 1e6)
            if full:                       # the same numbers: the lag matrix against the triangle just written (full_dot ran last)
                calls["lag_dot"]()
                i = torch.arange(n, device="cuda:0")[:, None]
                j = i + 1 + torch.arange(L, device="cuda:0")[None, :]
                ok = j < n
                assert torch.equal(out[ok], tri[i.expand_as(j)[ok], j[ok]])
            med = {k: statistics.median(v) for k, v in ts.items()}
            lag_tiles = len({(int(x), int(y)) for x, y in dist.lag_dosage_plan(n, n_words, max_lag, n_cus=n_cus)[:, :2]})
            lag3_tiles = len({(int(x), int(y)) for x, y in dist.lag_dosage_plan(3 * n, n_words, 3 * L + 2, n_cus=n_cus)[:, :2]})
            ratio = lag_tiles / tri_tiles
            rec = {"rows": n, "samples": S, "max_lag": max_lag, "reps": a.reps,
                   "lag_dot_us": round(med["lag_dot"], 1), "lag_corr_us": round(med["lag_corr"], 1),
                   "lag_complete_us": round(med["lag_complete"], 1),
                   "complete_over_corr": round(med["lag_complete"] / med["lag_corr"], 2),
                   "full_dot_us": round(med["full_dot"], 1) if full else None,
                   "full_complete_us": round(med["full_complete"], 1) if full else None,
                   "min_us": {k: round(min(v), 1) for k, v in ts.items()},
                   "lag_tiles": lag_tiles, "interleaved_tiles": lag3_tiles, "triangle_tiles": tri_tiles,
                   "tile_ratio": round(ratio, 4), "must_be_faster": ratio <= 0.5,
                   "scratch_mib": round((3 * n * ((3 * L + 2 + 3) // 4 * 4) * 4 + (3 * n + 130) * n_words * 8) / 2**20, 1)}
            if full:
                rec.update({"dot_time_ratio": round(med["lag_dot"] / med["full_dot"], 4),
                            "complete_time_ratio": round(med["lag_complete"] / med["full_complete"], 4),
                            "dot_faster": bool(med["lag_dot"] < med["full_dot"]),
                            "complete_faster": bool(med["lag_complete"] < med["full_complete"])})
            else:
                rec["full"] = f"not run: above --full-max-rows {a.full_max_rows} (n x n output and about 3 n^2 words of scratch)"
            print(json.dumps(rec), flush=True)
            del out
        del tri
        m.close()
    ctx.close()


if __name__ == "__main__":
    main()
