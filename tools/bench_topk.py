"""What selecting each row's k best neighbours on the device costs (topk_rows_kernel behind the panels' count kernel). Per
shape, alternating in one process after a warm-up, every call synchronous (the wait is inside the timed window):
  (a) storm_hip_pairw_topk_device for each score and k (count rectangles + row counts + selection, panel by panel);
  (b) the same panels' count rectangles alone: storm_hip_cross_dense_matrix_device of each panel's rows (copies of the
      rows, made once outside the timed window) against the whole matrix, into one panel-sized buffer;
  (c) a device-to-device copy of the panels' bytes (4 x rows x rows): the selection reads exactly these bytes once and
      writes next to nothing, the copy reads and writes them — the yardstick, not the code under test.
Shapes: rows x 65536 bits, 32768 draws per row (BASELINE c2's rows), 10000 and 32768 rows. One JSON line per shape: medians
in ms, (a) - (b) per score and k, and the copy's ms.
    python tools/bench_topk.py [--reps 10] [--shapes 10000,32768] [--ks 16,128] [--panel-rows 0] > out.jsonl
The selection kernel's own time: `rocprofv3 --kernel-trace --stats -- python tools/bench_topk.py ...` in a run of its own;
its FETCH_SIZE and VALU share: `rocprofv3 --pmc FETCH_SIZE VALUBusy -- python tools/bench_topk.py --reps 2 --shapes 10000`
(counters only)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stormbitmaps_amd as sb  # noqa: E402

SCORES = ("count", "jaccard", "ld_r2")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--shapes", default="10000,32768")
    ap.add_argument("--ks", default="16,128")
    ap.add_argument("--panel-rows", type=int, default=0)
    a = ap.parse_args()
    import torch
    lib = sb.load()
    ctx = sb.HipContext(0)
    ks = [int(k) for k in a.ks.split(",")]
    for shape in a.shapes.split(","):
        n, bits, draws = int(shape), 65536, 32768
        m = ctx.matrix(n, bits // 64)
        m.fill_synthetic(bits, draws, seed=42)
        ld = (n + 3) // 4 * 4
        panel = a.panel_rows or max(256, (256 << 20) // (4 * ld) // 256 * 256)
        panel = min(panel, (n + 255) // 256 * 256)
        starts = list(range(0, n, panel))
        parts = []
        for p0 in starts:        # the panels' rows as matrices of their own (the library's panels are views)
            rows = min(panel, n - p0)
            part = ctx.matrix(rows, bits // 64)
            part.import_device(m.device_ptr + 8 * p0 * m.stride_words, rows, m.stride_words)
            parts.append(part)
        rect = torch.zeros((panel, ld), dtype=torch.int32, device="cuda:0")
        dst = torch.empty_like(rect)
        idx = torch.zeros((n, max(ks)), dtype=torch.int32, device="cuda:0")
        val = torch.zeros((n, max(ks)), dtype=torch.int32, device="cuda:0")

        def counts():
            for part in parts:
                sb._lib.check(lib.storm_hip_cross_dense_matrix_device(ctx._h, part._h, m._h, 0, C.c_void_p(rect.data_ptr()), ld),
                              "storm_hip_cross_dense_matrix_device")

        def copy():
            for p0 in starts:
                rows = min(panel, n - p0)
                dst[:rows].copy_(rect[:rows])
            torch.cuda.synchronize()

        calls = {"counts": counts, "copy": copy}
        for score in SCORES:
            for k in ks:
                calls[f"{score}/{k}"] = lambda score=score, k=k: m.pairw_topk_device(idx.data_ptr(), val.data_ptr(), max(ks), k, score,
                                                                                    n_bits=bits, panel_rows=a.panel_rows)
        for fn in calls.values():    # warm-up: work lists, code objects, the context's buffers
            fn()
            fn()
        ts = {key: [] for key in calls}
        for _ in range(a.reps):      # alternating: a clock or a neighbour that drifts hits every call alike
            for key, fn in calls.items():
                t0 = time.perf_counter()
                fn()
                ts[key].append((time.perf_counter() - t0) * 1e3)
        med = {key: statistics.median(v) for key, v in ts.items()}
        topk = [key for key in calls if "/" in key]
        rec = {"shape": shape, "rows": n, "bits": bits, "draws": draws, "reps": a.reps, "panel_rows": panel, "panels": len(starts),
               "entries": n * n, "counts_ms": round(med["counts"], 4), "copy_ms": round(med["copy"], 4),
               "copy_GBps": round(8 * n * n / med["copy"] / 1e6, 1),
               "topk_ms": {key: round(med[key], 4) for key in topk},
               "topk_minus_counts_ms": {key: round(med[key] - med["counts"], 4) for key in topk},
               "selection_read_GBps": {key: round(4 * n * n / max(med[key] - med["counts"], 1e-6) / 1e6, 1) for key in topk},
               "min_ms": {key: round(min(v), 4) for key, v in ts.items()}}
        print(json.dumps(rec), flush=True)
        for part in parts:
            part.close()
        m.close()
        del rect, dst, idx, val
    ctx.close()


if __name__ == "__main__":
    main()
