#!/usr/bin/env python3
"""tilering_kernel in both of its forms: us per synchronous call of storm_hip_pairw_matrix_device (op AND) under k2_tile_shape 5
with k2_ring_sync 0 / 1 (tilering_kernel<false> / <true>), M = 65536 dense: median and minimum of 40 calls after 5, per row
count. One JSON line per (rows, ring_sync). STORM_HIP_LIB selects another build of the library.
    python tools/bench_ring_sync.py > out.jsonl"""
import json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import stormbitmaps_amd as sb

ctx = sb.HipContext(0)
M = 65536
for N in (2048, 4096, 8192, 10000):
    m = ctx.matrix(N, M // 64)
    m.fill_synthetic(M, M // 2, seed=42)
    out = torch.zeros((N, N), dtype=torch.int32, device="cuda:0")
    for sync in (0, 1):
        ctx.set_option("k2_tile_shape", 5)
        ctx.set_option("k2_ring_sync", sync)
        for _ in range(5):
            m.pairw_matrix_device(out.data_ptr(), N, "and")
        ts = []
        for _ in range(40):
            t0 = time.perf_counter()
            m.pairw_matrix_device(out.data_ptr(), N, "and")
            ts.append(time.perf_counter() - t0)
        print(json.dumps({"rows": N, "ring_sync": sync, "median_us": round(statistics.median(ts) * 1e6, 1), "min_us": round(min(ts) * 1e6, 1)}), flush=True)
    del out
    m.close()
