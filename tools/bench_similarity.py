"""What finishing the per-pair matrix on the device costs (finish_tiles_kernel<SimilarityStat> behind the count kernels). Per
shape, alternating in one process after a warm-up, every call synchronous (the wait is inside the timed window):
  (a) the existing *_pairw_matrix_device with op AND (the counts alone);
  (b) *_pairw_similarity_device for each measure (counts + row counts + finish);
  (c) a device-to-device copy of 4 x (entries converted) bytes: the same bytes in and out as the finishing pass moves —
      the yardstick, not the code under test.
Shapes: STORM_contiguous_t of 1024 / 2048 / 4096 / 10000 rows x 65536 bits (the LD-window sizes of DESIGN.md §4 and
BASELINE c2, 32768 draws per row) and the K5 shape (STORM_t, 10000 rows x 524288 bits, 524 draws per row). One JSON line
per shape: medians in ms, (b) - (a) per measure, and the copy's ms.
    python tools/bench_similarity.py [--reps 20] [--shapes 1024,2048,4096,10000,k5] > out.jsonl
The finishing kernel's own time: `rocprofv3 --kernel-trace --stats -- python tools/bench_similarity.py ...` in a run of
its own; its FETCH_SIZE / WRITE_SIZE: `rocprofv3 --pmc FETCH_SIZE WRITE_SIZE -- python tools/bench_similarity.py --reps 2
--shapes 10000` (counters only)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stormbitmaps_amd as sb  # noqa: E402

MEASURES = ("jaccard", "cosine", "ld_d", "ld_r2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="1024,2048,4096,10000,k5")
    a = ap.parse_args()
    import torch
    for shape in a.shapes.split(","):
        if shape == "k5":
            n, bits, draws = 10000, 524288, 524
            h = sb.Storm()
            h.add_synthetic(bits, n, draws, seed=42)
        else:
            n, bits, draws = int(shape), 65536, 32768
            h = sb.StormContig(bits)
            h.add_synthetic(n, draws, seed=42)
        out = torch.zeros((n, n), dtype=torch.float32, device="cuda:0")
        converted = n * (n - 1) // 2
        src = torch.zeros(converted, dtype=torch.float32, device="cuda:0")
        dst = torch.empty_like(src)

        def copy():
            dst.copy_(src)
            torch.cuda.synchronize()

        calls = {"counts": lambda: h.pairw_matrix_device(out.data_ptr(), n, n), "copy": copy}
        for m in MEASURES:
            calls[m] = lambda m=m: h.pairw_similarity_device(out.data_ptr(), n, n, m, n_bits=bits)
        for fn in calls.values():    # warm-up: device copies, work lists, code objects
            fn()
            fn()
        ts = {k: [] for k in calls}
        for _ in range(a.reps):      # alternating: a clock or a neighbour that drifts hits every call alike
            for k, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                ts[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: statistics.median(v) for k, v in ts.items()}
        rec = {"shape": shape, "rows": n, "bits": bits, "draws": draws, "reps": a.reps, "entries_converted": converted,
               "counts_ms": round(med["counts"], 4), "copy_ms": round(med["copy"], 4),
               "copy_GBps": round(8 * converted / med["copy"] / 1e6, 1),
               "similarity_ms": {m: round(med[m], 4) for m in MEASURES},
               "similarity_minus_counts_ms": {m: round(med[m] - med["counts"], 4) for m in MEASURES},
               "min_ms": {k: round(min(v), 4) for k, v in ts.items()}}
        print(json.dumps(rec), flush=True)
        h.free()
        del out, src, dst


if __name__ == "__main__":
    main()
