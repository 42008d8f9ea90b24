#!/usr/bin/env python3
"""LD scores reduced on the device against today's route through the host: us per synchronous call (launch + completion
included), S = 65536 samples of random codes 0 .. 3 (a quarter of them 3: missing, for the calls that read it so), per row
count and max_lag, for r2 and r2_adj, complete-case ("cc") and pairwise-complete ("pc"):
  ldscore_us        (a) storm_hip_lag_dosage_ldscore[_complete]_device + a stream synchronize: the band of r^2 into the context's
                    scratch, lag_band_sums_kernel over it, n floats and n counts in device memory
  corr_us           (b) storm_hip_pairw_lag_dosage_corr[_complete]_device alone, on the same build: (a) - (b) is what the
                    reduction adds
  reduce_us         lag_band_sums_kernel alone over a band already in device memory (storm_hip_lag_band_sums_device + a
                    synchronize); reduce_gbs = 8 n L bytes (every entry is read twice) over it
  host_route_us     (c) today's route: the HOST form of pairw_lag_dosage_corr[_complete] (n x L floats over the bus), then numpy:
                    the sum of every row for the pairs ahead, the anti-diagonals for the pairs behind, NaN skipped (r2 only;
                    --host-reps rounds)
  d2d_us            (d) a device-to-device copy of n x L floats: the bandwidth yardstick of the reduction (4 n L bytes read and
                    as many written); d2d_gbs = 8 n L bytes over it
Medians of --reps rounds after a warm-up, every round in a freshly shuffled order of the calls (a call that always ran
behind the same neighbour inherited that neighbour's caches); the minimum beside them. One JSON line per (rows, max_lag).
    python tools/bench_ldscore.py [--rows 8192,32768] [--lags 128,1024,4096] [--reps 9] > profiles/ldscore.jsonl"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stormbitmaps_amd as sb  # noqa: E402

S = 65536


def host_route(band, n, L):
    """what a caller does today with the n x L host matrix: rows for the pairs ahead, anti-diagonals for the pairs behind"""
    score = np.nansum(band, axis=1, dtype=np.float64)
    for d in range(L):
        score[d + 1:] += np.nan_to_num(band[:n - 1 - d, d]).astype(np.float64)
    return score.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="8192,32768")
    ap.add_argument("--lags", default="128,1024,4096")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    random.seed(1)
    import torch
    ctx = sb.HipContext(0)
    n_words = S // 32
    for n in [int(x) for x in a.rows.split(",")]:
        words = torch.randint(-(1 << 62), 1 << 62, (n, n_words), dtype=torch.int64, device="cuda:0")
        words = words * 2 + torch.randint(0, 2, (n, n_words), dtype=torch.int64, device="cuda:0")   # all 64 bits random
        m = ctx.matrix(n, n_words)
        m.import_device(words.data_ptr(), n, n_words)
        ctx.synchronize()
        del words
        score = torch.zeros(n, dtype=torch.float32, device="cuda:0")
        pairs = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        for max_lag in [int(x) for x in a.lags.split(",")]:
            L = min(max_lag, n - 1)
            band = torch.zeros((n, L), dtype=torch.float32, device="cuda:0")
            copy = torch.empty_like(band)

            def ldscore(stat, complete):
                m.lag_dosage_ldscore_device(score.data_ptr(), pairs.data_ptr(), max_lag, S, stat, complete)
                ctx.synchronize()

            def reduce(stat):
                ctx.lag_band_sums_device(band.data_ptr(), L, n, max_lag, score.data_ptr(), pairs.data_ptr(), stat, S)
                ctx.synchronize()

            def d2d():
                copy.copy_(band)
                torch.cuda.synchronize()

            calls = {"ldscore_cc_r2": lambda: ldscore("r2", False), "ldscore_cc_r2_adj": lambda: ldscore("r2_adj", False),
                     "ldscore_pc_r2": lambda: ldscore("r2", True), "ldscore_pc_r2_adj": lambda: ldscore("r2_adj", True),
                     "corr_cc": lambda: m.pairw_lag_dosage_corr_device(band.data_ptr(), L, max_lag, S, "r2"),
                     "corr_pc": lambda: m.pairw_lag_dosage_corr_complete_device(band.data_ptr(), L, max_lag, S, "r2"),
                     "reduce_r2": lambda: reduce("r2"), "reduce_r2_adj": lambda: reduce("r2_adj"), "d2d": d2d}
            for fn in calls.values():      # warm-up: work lists, scratch, code objects
                fn()
                fn()
            ts = {k: [] for k in calls}
            order = list(calls)
            for _ in range(a.reps):        # alternating: a clock or a neighbour that drifts hits every call alike ...
                random.shuffle(order)      # ... in a new order every round: no call always runs behind the same one
                for k in order:
                    t0 = time.perf_counter()
                    calls[k]()
                    ts[k].append((time.perf_counter() - t0) * 1e6)
            # the same numbers: the device's scores against the host route's (float64 sums of the same floats)
            host = {}
            for key, complete in (("host_route_cc", False), ("host_route_pc", True)):
                f = m.pairw_lag_dosage_corr_complete if complete else m.pairw_lag_dosage_corr
                ts[key] = []
                for _ in range(a.host_reps):
                    t0 = time.perf_counter()
                    host[key] = host_route(f(max_lag, S, "r2"), n, L)
                    ts[key].append((time.perf_counter() - t0) * 1e6)
                ldscore("r2", complete)
                dev = score.cpu().numpy()
                assert np.allclose(dev, host[key], rtol=1e-6, atol=1e-6), (key, float(np.abs(dev - host[key]).max()))
            med = {k: statistics.median(v) for k, v in ts.items()}
            nbytes = 8.0 * n * L
            rec = {"rows": n, "samples": S, "max_lag": max_lag, "reps": a.reps, "host_reps": a.host_reps,
                   "ldscore_us": {k[8:]: round(med[k], 1) for k in calls if k.startswith("ldscore_")},
                   "corr_us": {"cc": round(med["corr_cc"], 1), "pc": round(med["corr_pc"], 1)},
                   "ldscore_minus_corr_us": {k[8:]: round(med[k] - med["corr_" + k[8:10]], 1) for k in calls if k.startswith("ldscore_")},
                   "reduce_us": {"r2": round(med["reduce_r2"], 1), "r2_adj": round(med["reduce_r2_adj"], 1)},
                   "reduce_gbs": {"r2": round(nbytes / med["reduce_r2"] / 1e3, 1), "r2_adj": round(nbytes / med["reduce_r2_adj"] / 1e3, 1)},
                   "host_route_us": {"cc": round(med["host_route_cc"], 1), "pc": round(med["host_route_pc"], 1)},
                   "host_over_device": {"cc": round(med["host_route_cc"] / med["ldscore_cc_r2"], 1),
                                        "pc": round(med["host_route_pc"] / med["ldscore_pc_r2"], 1)},
                   "d2d_us": round(med["d2d"], 1), "d2d_gbs": round(nbytes / med["d2d"] / 1e3, 1),
                   "band_mib": round(4.0 * n * L / 2**20, 1),
                   "min_us": {k: round(min(v), 1) for k, v in ts.items()}}
            print(json.dumps(rec), flush=True)
            del band, copy
        m.close()
    ctx.close()


if __name__ == "__main__":
    main()
