#!/usr/bin/env python3
"""Stratified LD scores in a distance window, reduced on the device: us per synchronous call (launch + completion included),
S = 65536 samples of random codes 0 .. 3, complete-case r2, per (rows, max_lag), window kind and column count C:
  call_us        storm_hip_lag_dosage_ldscore_annot_device + a stream synchronize: the band of r^2 into the context's scratch,
                 the window bounds uploaded, lag_band_annot_sums_kernel over it, n x C floats and n counts in device memory
  reduce_us      lag_band_annot_sums_kernel alone over a band already in device memory
                 (storm_hip_lag_band_annot_sums_device + a synchronize), once per inner product: "fma" (v_fma_f64 from LDS
                 operands) and "mfma" (v_mfma_f64_16x16x4_f64), chosen per launch by STORM_HIP_LDSCORE_ANNOT_INNER; the
                 whole call runs what ships (the variable unset). The two agree to double rounding (checked here).
  corr_us        storm_hip_pairw_lag_dosage_corr_device alone at the same shape: call_us - corr_us is what the reduction adds
  plain_us       at C = 1: lag_band_sums_kernel alone (storm_hip_lag_band_sums_device) at the same shape, in the same run
  d2d_us         a device-to-device copy of the n x L floats: 4 n L bytes read and as many written, the band read twice at
                 the bandwidth of a device copy; d2d_gbs = 8 n L bytes over it
windows: "count" — max_lag rows on each side (no bounds); "pos" — positions whose windows reach between L/4 and L rows
(steps that grow from 1 to 4 and back along the rows, max_dist = L), the band computed at max_lag = L.
Medians of --reps rounds after a warm-up, every round in a freshly shuffled order of the calls; the minimum beside them. One
JSON line per (rows, max_lag, window, C).
    python tools/bench_ldscore_annot.py [--shapes 8192:128,32768:4096] [--cols 1,64,96] [--reps 9] > profiles/ldscore_annot.jsonl"""
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


def positions(n, L):
    """steps between 1 and 4 in a slow wave: under max_dist = L a row reaches between L / 4 and L rows on either side"""
    step = 2.5 + 1.5 * np.sin(np.arange(n) * (2 * np.pi / max(8 * L, 1024)))
    return np.cumsum(np.clip(step, 1.0, 4.0))


def windows(pos, dist):
    lo = np.searchsorted(pos, pos - dist, "left").astype(np.uint32)
    hi = (np.searchsorted(pos, pos + dist, "right") - 1).astype(np.uint32)
    return lo, hi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8192:128,32768:4096")
    ap.add_argument("--cols", default="1,64,96")
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    random.seed(1)
    import torch
    ctx = sb.HipContext(0)
    n_words = S // 32
    for shape in a.shapes.split(","):
        n, max_lag = (int(x) for x in shape.split(":"))
        words = torch.randint(-(1 << 62), 1 << 62, (n, n_words), dtype=torch.int64, device="cuda:0")
        words = words * 2 + torch.randint(0, 2, (n, n_words), dtype=torch.int64, device="cuda:0")   # all 64 bits random
        m = ctx.matrix(n, n_words)
        m.import_device(words.data_ptr(), n, n_words)
        ctx.synchronize()
        del words
        L = min(max_lag, n - 1)
        band = torch.zeros((n, L), dtype=torch.float32, device="cuda:0")
        copy = torch.empty_like(band)
        pairs = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        plain = torch.zeros(n, dtype=torch.float32, device="cuda:0")
        pos = positions(n, L)
        lo, hi = windows(pos, float(L))
        i = np.arange(n)
        reach = np.maximum(i - lo, hi - i)
        assert reach.max() <= L and reach[L:n - L].min() >= L // 4, (int(reach.max()), int(reach[L:n - L].min()))
        d_lo, d_hi = torch.from_numpy(lo.view(np.int32).copy()).cuda(), torch.from_numpy(hi.view(np.int32).copy()).cuda()
        m.pairw_lag_dosage_corr_device(band.data_ptr(), L, max_lag, S, "r2")       # the band the reduce-alone calls read
        ctx.synchronize()
        for window in ("count", "pos"):
            for C in [int(x) for x in a.cols.split(",")]:
                annot = torch.randn((n, C), dtype=torch.float32, device="cuda:0")
                score = torch.zeros((n, C), dtype=torch.float32, device="cuda:0")
                w_lo, w_hi = (lo, hi) if window == "pos" else (None, None)
                p_lo, p_hi = (d_lo.data_ptr(), d_hi.data_ptr()) if window == "pos" else (None, None)

                def call():
                    m.lag_dosage_ldscore_annot_device(annot.data_ptr(), C, C, score.data_ptr(), C, pairs.data_ptr(), max_lag, S, "r2",
                                                      False, w_lo, w_hi)   # (waits itself)

                def reduce(inner=None):
                    if inner:
                        os.environ["STORM_HIP_LDSCORE_ANNOT_INNER"] = inner
                    ctx.lag_band_annot_sums_device(band.data_ptr(), L, n, max_lag, annot.data_ptr(), C, C, score.data_ptr(), C,
                                                   pairs.data_ptr(), "r2", S, None, 0, 1, p_lo, p_hi)
                    ctx.synchronize()
                    os.environ.pop("STORM_HIP_LDSCORE_ANNOT_INNER", None)

                def corr():
                    m.pairw_lag_dosage_corr_device(copy.data_ptr(), L, max_lag, S, "r2")

                def d2d():
                    copy.copy_(band)
                    torch.cuda.synchronize()

                def plain_reduce():
                    ctx.lag_band_sums_device(band.data_ptr(), L, n, max_lag, plain.data_ptr(), pairs.data_ptr(), "r2", S)
                    ctx.synchronize()

                calls = {"call": call, "reduce_fma": lambda: reduce("fma"), "reduce_mfma": lambda: reduce("mfma"), "corr": corr,
                         "d2d": d2d}
                if C == 1:
                    calls["plain"] = plain_reduce
                for fn in calls.values():      # warm-up: work lists, scratch, code objects
                    fn()
                    fn()
                ts = {k: [] for k in calls}
                order = list(calls)
                for _ in range(a.reps):
                    random.shuffle(order)
                    for k in order:
                        t0 = time.perf_counter()
                        calls[k]()
                        ts[k].append((time.perf_counter() - t0) * 1e6)
                if C == 1 and window == "count":   # the same numbers: a column of ones is the plain reduction
                    annot.fill_(1.0)
                    reduce()
                    plain_reduce()
                    assert torch.allclose(score[:, 0], plain, rtol=1e-6, atol=1e-6)
                reduce("fma")                      # the two inner products: the same sums to double rounding
                by_fma = score.clone()
                reduce("mfma")
                assert torch.allclose(score, by_fma, rtol=1e-6, atol=1e-6), float((score - by_fma).abs().max())
                med = {k: statistics.median(v) for k, v in ts.items()}
                nbytes = 8.0 * n * L
                rec = {"rows": n, "samples": S, "max_lag": max_lag, "window": window, "cols": C, "reps": a.reps,
                       "window_rows": {"min": int(reach.min()), "median": int(np.median(reach)), "max": int(reach.max())} if window == "pos" else None,
                       "call_us": round(med["call"], 1),
                       "reduce_us": {"fma": round(med["reduce_fma"], 1), "mfma": round(med["reduce_mfma"], 1)},
                       "corr_us": round(med["corr"], 1),
                       "call_minus_corr_us": round(med["call"] - med["corr"], 1),
                       "plain_us": round(med["plain"], 1) if "plain" in med else None,
                       "d2d_us": round(med["d2d"], 1), "d2d_gbs": round(nbytes / med["d2d"] / 1e3, 1),
                       "reduce_over_d2d": {"fma": round(med["reduce_fma"] / med["d2d"], 2), "mfma": round(med["reduce_mfma"] / med["d2d"], 2)},
                       "band_mib": round(4.0 * n * L / 2**20, 1), "min_us": {k: round(min(v), 1) for k, v in ts.items()}}
                print(json.dumps(rec), flush=True)
                del annot, score
        del band, copy
        m.close()
    ctx.close()


if __name__ == "__main__":
    main()
