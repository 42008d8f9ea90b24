#!/usr/bin/env python3
"""Greedy LD pruning / clumping resolved on the device against today's route through the host: us per synchronous call (launch
+ completion included), S = 65536 samples, rows with real LD — the law of tests/_prune.py's generator, drawn on the device:
blocks of 1 to 24 rows, within a block every row is the previous one with each sample redrawn with a probability of
U(0.10, 0.35), so r^2 decays along a block and chains form (independent random codes would give an empty graph) — per row
count, max_lag, min_r2 and order ("row": priority NULL; "random": random priorities, sorted by the host planner outside the
timed region as storm.h's call does inside it):
  prune_us          (a) storm_hip_lag_dosage_prune_device with owners + a stream synchronize: the band of r^2 into the context's
                    scratch, lag_band_threshold_kernel, band_mis_resolve_kernel, band_mis_owner_kernel; n bytes and n words in
                    device memory
  corr_us           (b) storm_hip_pairw_lag_dosage_corr_device alone, on the same build
  band_us           (c) the three kernels alone over a band already in device memory (storm_hip_lag_band_prune_device + a
                    synchronize), with owners; band_keep_us: without (no owner kernel)
  kernel_us         the device time of each kernel alone, from the profiler's kernel records over the calls of (c)
                    (torch.profiler; null where no record came back: not measured)
  d2d_us            (d) a device-to-device copy of n x L floats: the yardstick of the threshold kernel, which reads the band
                    ONCE (4 n L bytes) and writes n x pitch words of masks (1/16 of that)
  host_route_us     (e) today's route: the HOST form of pairw_lag_dosage_corr (n x L floats over the bus), then a numpy greedy
                    over the band (--host-reps rounds); its keep flags are compared with the device's: equal, or the run fails
  kept              rows kept; resolve_ns_per_kept = the resolver's kernel time over it
Medians of --reps rounds after a warm-up, every round in a freshly shuffled order of the calls; the minimum beside them. One
JSON line per (rows, max_lag, min_r2, order).
    python tools/bench_prune.py [--rows 8192,32768] [--lags 128,1024,4096] [--reps 9] > profiles/prune.jsonl"""
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
KERNELS = {"threshold": "lag_band_threshold_kernel", "resolve": "band_mis_resolve_kernel", "owner": "band_mis_owner_kernel"}


def ld_words(n, seed):
    """[n, S / 32] int64 on the device: packed 2-bit dosages 0 .. 2 of rows in blocks of decaying LD (tests/_prune.py: ld_rows),
    all blocks drawn side by side, one step per position within the block"""
    import torch
    g = torch.Generator(device="cuda:0").manual_seed(seed)
    sizes = []
    rng = np.random.default_rng(seed)
    while sum(sizes) < n:
        sizes.append(int(rng.integers(1, 25)))
    sizes[-1] -= sum(sizes) - n
    starts = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    size_t, start_t = torch.tensor(sizes, device="cuda:0"), torch.tensor(starts, device="cuda:0")
    words = torch.zeros((n, S // 32), dtype=torch.int64, device="cuda:0")
    shifts = (2 * torch.arange(32, device="cuda:0", dtype=torch.int64)).view(1, 1, 32)
    chunk = 512                                                                    # blocks at a time: 512 x S values per step
    for b0 in range(0, len(sizes), chunk):
        sz, st = size_t[b0:b0 + chunk], start_t[b0:b0 + chunk]
        k = sz.shape[0]
        freq = (0.15 + 0.35 * torch.rand((k, 1), generator=g, device="cuda:0")).expand(k, S)
        draw = lambda: (torch.rand((k, S), generator=g, device="cuda:0") < freq).to(torch.int64) + \
            (torch.rand((k, S), generator=g, device="cuda:0") < freq).to(torch.int64)   # binomial(2, freq)
        cur = draw()
        for t in range(int(sz.max())):
            live = sz > t
            packed = (cur.view(k, S // 32, 32) << shifts).sum(dim=2)
            words[(st + t)[live]] = packed[live]
            p = 0.10 + 0.25 * torch.rand((k, 1), generator=g, device="cuda:0")
            cur = torch.where(torch.rand((k, S), generator=g, device="cuda:0") < p, draw(), cur)
    return words


def host_greedy(band, n, L, min_r2, order):
    """what a caller does today with the n x L host matrix: walk the order, mark the kept row's neighbours on both sides"""
    keep, marked = np.zeros(n, np.uint8), np.zeros(n, bool)
    with np.errstate(invalid="ignore"):
        edge = band > np.float32(min_r2)
    lags = np.arange(L)
    for v in (range(n) if order is None else order.tolist()):
        if marked[v]:
            continue
        keep[v] = 1
        k = min(L, n - 1 - v)
        marked[v + 1:v + 1 + k] |= edge[v, :k]
        k = min(L, v)
        marked[v - 1 - lags[:k]] |= edge[v - 1 - lags[:k], lags[:k]]
    return keep


def kernel_times(fn, reps):
    """median device us of each of the three kernels over `reps` calls of fn, or None"""
    try:
        import torch
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
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
    ap.add_argument("--min-r2", default="0.2,0.5")
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
        keep = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        owner = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        priority = np.random.default_rng(n).random(n, dtype=np.float32)
        orders = {"row": None, "random": np.lexsort((np.arange(n), -priority)).astype(np.uint32)}
        for max_lag in [int(x) for x in a.lags.split(",")]:
            L = min(max_lag, n - 1)
            band = torch.zeros((n, L), dtype=torch.float32, device="cuda:0")
            copy = torch.empty_like(band)
            m.pairw_lag_dosage_corr_device(band.data_ptr(), L, max_lag, S, "r2")
            ctx.synchronize()
            host_band = None
            for min_r2 in [float(x) for x in a.min_r2.split(",")]:
                for order_name, order in orders.items():
                    def d2d():
                        copy.copy_(band)
                        torch.cuda.synchronize()

                    def corr():
                        m.pairw_lag_dosage_corr_device(band.data_ptr(), L, max_lag, S, "r2")
                        ctx.synchronize()

                    calls = {"prune": lambda: m.lag_dosage_prune_device(keep.data_ptr(), owner.data_ptr(), min_r2, max_lag, S, order=order),
                             "corr": corr,
                             "band": lambda: ctx.lag_band_prune_device(band.data_ptr(), L, n, max_lag, min_r2, keep.data_ptr(),
                                                                       owner.data_ptr(), order=order),
                             "band_keep": lambda: ctx.lag_band_prune_device(band.data_ptr(), L, n, max_lag, min_r2, keep.data_ptr(),
                                                                            order=order),
                             "d2d": d2d}
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
                    kern = kernel_times(calls["band"], a.reps)
                    calls["prune"]()
                    dev_keep = keep.cpu().numpy().copy()
                    ts["host_route"] = []
                    for _ in range(a.host_reps):
                        t0 = time.perf_counter()
                        host_band = m.pairw_lag_dosage_corr(max_lag, S, "r2")
                        host_keep = host_greedy(host_band, n, L, min_r2, order)
                        ts["host_route"].append((time.perf_counter() - t0) * 1e6)
                    assert np.array_equal(dev_keep, host_keep), int((dev_keep != host_keep).sum())
                    med = {k: statistics.median(v) for k, v in ts.items()}
                    kept = int(dev_keep.sum())
                    rec = {"rows": n, "samples": S, "max_lag": max_lag, "min_r2": min_r2, "order": order_name, "reps": a.reps,
                           "host_reps": a.host_reps, "kept": kept, "kept_share": round(kept / n, 3),
                           "prune_us": round(med["prune"], 1), "corr_us": round(med["corr"], 1),
                           "prune_over_corr": round(med["prune"] / med["corr"], 3),
                           "band_us": round(med["band"], 1), "band_keep_us": round(med["band_keep"], 1), "kernel_us": kern,
                           "d2d_us": round(med["d2d"], 1),
                           "threshold_over_d2d": None if kern["threshold"] is None else round(kern["threshold"] / med["d2d"], 2),
                           "resolve_ns_per_kept": None if kern["resolve"] is None else round(1e3 * kern["resolve"] / max(kept, 1), 1),
                           "resolve_over_corr": None if kern["resolve"] is None else round(kern["resolve"] / med["corr"], 3),
                           "host_route_us": round(med["host_route"], 1), "host_over_prune": round(med["host_route"] / med["prune"], 1),
                           "band_mib": round(4.0 * n * L / 2**20, 1),
                           "min_us": {k: round(min(v), 1) for k, v in ts.items()}}
                    print(json.dumps(rec), flush=True)
            del band, copy, host_band
        m.close()
    ctx.close()


if __name__ == "__main__":
    main()
