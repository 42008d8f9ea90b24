#!/usr/bin/env python3
"""The sparse LD report compacted on the device against the route through the host it replaces: us per synchronous call (launch
+ completion included), S = 65536 samples, rows with real LD (tools/bench_prune.py's generator: the law of tests/_prune.py's
ld_rows, drawn on the device), per row count, max_lag and min_r2:
  sparse_us         (a) storm_hip_lag_dosage_corr_sparse_device + a stream synchronize: the band of r^2 into the context's
                    scratch, lag_band_sparse_count_kernel, the three launches of the scan, lag_band_sparse_fill_kernel; the
                    offsets and exactly `pairs` (col, val) entries in device memory (the capacity is the total, counted
                    outside the timed region)
  corr_us           (b) storm_hip_pairw_lag_dosage_corr_device alone, on the same build
  band_us           (c) the five launches alone over a band already in device memory (storm_hip_lag_band_sparse_device + a
                    synchronize); band_count_us: the count-only call (no fill)
  kernel_us         the device time of each kernel alone, from the profiler's kernel records over calls of (c) in a run of
                    their own (torch.profiler; null where no record came back: not measured); "threshold" is
                    lag_band_threshold_kernel of the pruning call over the same band and threshold, the nearest existing
                    kernel: it also reads the band once, and writes both sides' masks
  d2d_us            (d) a device-to-device copy of n x L floats: the yardstick of the count kernel, which reads the band ONCE
                    (4 n L bytes) and writes n x ceil(L / 64) 64-bit words of masks (1/32 of that)
  host_route_us     (e) the route it replaces: the HOST form of pairw_lag_dosage_corr (n x L floats over the bus), then numpy's
                    nonzero over band > min_r2 (--host-reps rounds); its list is compared with the device's: row_start, col and
                    the bits of val equal, or the run fails
  pairs             entries listed; share = pairs / (the band's entries that are pairs)
Medians of --reps rounds after a warm-up, every round in a freshly shuffled order of the calls; the minimum beside them. One
JSON line per (rows, max_lag, min_r2).
    python tools/bench_lag_sparse.py [--rows 8192,32768] [--lags 128,1024,4096] [--reps 9] > profiles/lag_sparse.jsonl"""
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
from bench_prune import S, ld_words  # noqa: E402  (tools/ is the script's own directory)

KERNELS = {"count": "lag_band_sparse_count_kernel", "block_sums": "lag_sparse_block_sums_kernel",
           "scan_sums": "lag_sparse_scan_sums_kernel", "offsets": "lag_sparse_offsets_kernel",
           "fill": "lag_band_sparse_fill_kernel", "threshold": "lag_band_threshold_kernel"}


def host_list(band, n, L, min_r2):
    """what a caller does today with the n x L host matrix (the corner is 0 there, and a NaN fails the comparison)"""
    with np.errstate(invalid="ignore"):
        listed = band > np.float32(min_r2)
    listed &= (np.arange(n)[:, None] + 1 + np.arange(L)[None, :]) < n              # (a negative threshold would list the corner)
    i, d = np.nonzero(listed)
    row_start = np.concatenate([[0], np.cumsum(listed.sum(axis=1))]).astype(np.uint64)
    return row_start, (i + 1 + d).astype(np.uint32), band[i, d]


def kernel_times(fns, reps):
    """median device us of each kernel over `reps` calls of every fn, or None"""
    try:
        import torch
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                for fn in fns:
                    fn()
            torch.cuda.synchronize()
        found = {k: [] for k in KERNELS}
        for ev in prof.events():
            for k, name in KERNELS.items():
                if name in ev.name:
                    t = getattr(ev, "device_time", None)
                    found[k].append(float(t if t is not None else ev.cuda_time))
        return {k: (round(statistics.median(v), 1) if v else None) for k, v in found.items()}
    except Exception as e:  # the profiler is an optional yardstick: say so, never guess
        print(f"kernel records not available: {e!r}", file=sys.stderr)
        return {k: None for k in KERNELS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="8192,32768")
    ap.add_argument("--lags", default="128,1024,4096")
    ap.add_argument("--min-r2", default="0.2,0.5,0.8")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    a = ap.parse_args()
    random.seed(1)
    import torch
    ctx = sb.HipContext(0)
    n_words = S // 32
    for n in [int(x) for x in a.rows.split(",")]:
        words = ld_words(n, n)
        m = ctx.matrix(n, n_words)
        m.import_device(words.data_ptr(), n, n_words)
        ctx.synchronize()
        del words
        rows = torch.zeros(n + 1, dtype=torch.int64, device="cuda:0")
        keep = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        for max_lag in [int(x) for x in a.lags.split(",")]:
            L = min(max_lag, n - 1)
            band = torch.zeros((n, L), dtype=torch.float32, device="cuda:0")
            copy = torch.empty_like(band)
            m.pairw_lag_dosage_corr_device(band.data_ptr(), L, max_lag, S, "r2")
            ctx.synchronize()
            live = n * L - L * (L + 1) // 2                                        # the band's entries that are pairs
            for min_r2 in [float(x) for x in a.min_r2.split(",")]:
                m.lag_dosage_corr_sparse_device(rows.data_ptr(), None, None, 0, min_r2, max_lag, S)   # the total, untimed
                total = int(rows[n].item())
                col = torch.zeros(max(total, 1), dtype=torch.int32, device="cuda:0")
                val = torch.zeros(max(total, 1), dtype=torch.float32, device="cuda:0")

                def d2d():
                    copy.copy_(band)
                    torch.cuda.synchronize()

                def corr():
                    m.pairw_lag_dosage_corr_device(band.data_ptr(), L, max_lag, S, "r2")
                    ctx.synchronize()

                calls = {"sparse": lambda: m.lag_dosage_corr_sparse_device(rows.data_ptr(), col.data_ptr(), val.data_ptr(), total,
                                                                           min_r2, max_lag, S),
                         "corr": corr,
                         "band": lambda: ctx.lag_band_sparse_device(band.data_ptr(), L, n, max_lag, min_r2, rows.data_ptr(),
                                                                    col.data_ptr(), val.data_ptr(), total),
                         "band_count": lambda: ctx.lag_band_sparse_device(band.data_ptr(), L, n, max_lag, min_r2, rows.data_ptr()),
                         "d2d": d2d}
                prune = lambda: ctx.lag_band_prune_device(band.data_ptr(), L, n, max_lag, min_r2, keep.data_ptr())   # noqa: E731
                for fn in calls.values():      # warm-up: work lists, scratch, code objects
                    fn()
                    fn()
                ts = {k: [] for k in calls}
                names = list(calls)
                for _ in range(a.reps):
                    random.shuffle(names)      # no call always runs behind the same one
                    for k in names:
                        t0 = time.perf_counter()
                        calls[k]()
                        ts[k].append((time.perf_counter() - t0) * 1e6)
                kern = kernel_times([calls["band"], prune], a.reps)
                calls["sparse"]()
                dev = (rows.cpu().numpy().view(np.uint64), col.cpu().numpy().view(np.uint32)[:total],
                       val.cpu().numpy().view(np.uint32)[:total])
                ts["host_route"] = []
                for _ in range(a.host_reps):
                    t0 = time.perf_counter()
                    host_band = m.pairw_lag_dosage_corr(max_lag, S, "r2")
                    host = host_list(host_band, n, L, min_r2)
                    ts["host_route"].append((time.perf_counter() - t0) * 1e6)
                assert np.array_equal(dev[0], host[0]) and np.array_equal(dev[1], host[1]), "the host route lists other pairs"
                assert np.array_equal(dev[2], host[2].view(np.uint32)), "the host route lists other values"
                med = {k: statistics.median(v) for k, v in ts.items()}
                new = [kern[k] for k in ("count", "block_sums", "scan_sums", "offsets", "fill")]
                rec = {"rows": n, "samples": S, "max_lag": max_lag, "min_r2": min_r2, "reps": a.reps, "host_reps": a.host_reps,
                       "pairs": total, "share": round(total / live, 4),
                       "sparse_us": round(med["sparse"], 1), "corr_us": round(med["corr"], 1),
                       "sparse_over_corr": round(med["sparse"] / med["corr"], 3),
                       "band_us": round(med["band"], 1), "band_count_us": round(med["band_count"], 1), "kernel_us": kern,
                       "kernels_sum_us": None if None in new else round(sum(new), 1),
                       "d2d_us": round(med["d2d"], 1),
                       "count_over_d2d": None if kern["count"] is None else round(kern["count"] / med["d2d"], 2),
                       "count_over_threshold": None if None in (kern["count"], kern["threshold"]) else
                       round(kern["count"] / kern["threshold"], 2),
                       "host_route_us": round(med["host_route"], 1), "host_over_sparse": round(med["host_route"] / med["sparse"], 1),
                       "band_mib": round(4.0 * n * L / 2**20, 1), "list_mib": round(8.0 * total / 2**20, 2),
                       "min_us": {k: round(min(v), 1) for k, v in ts.items()}}
                print(json.dumps(rec), flush=True)
                del col, val
            del band, copy
        m.close()
    ctx.close()


if __name__ == "__main__":
    main()
