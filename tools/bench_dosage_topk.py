"""What selecting each dosage row's k best r^2 neighbours on the device costs, against the route there was before the call
existed. Per shape and form (plain / pairwise-complete), alternating in one process after a warm-up, every call synchronous
(the wait is inside the timed window):
  (a) STORM_dosage_pairw_topk[_complete]_device: row sums or splits once, then per panel the sums' rectangles and the
      selection, which forms every entry's value itself;
  (b) the same panels' rectangles alone — plain: STORM_dosage_square_dot_device of each panel's rows (containers of their
      own, filled outside the timed window) against the whole container into one panel-sized buffer; complete:
      STORM_dosage_square_corr_complete_device of the same panels, i.e. the six products WITH their finish pass (no public
      call runs the six products alone), so (a) - (b) understates the selection there;
  (c) the former route: STORM_dosage_square_corr[_complete]_device of the container against itself into an n x n float
      matrix, the diagonal and the NaN entries set to -inf, then torch.topk on the device;
  (d) a device-to-device copy of the panels' bytes (4 x rows x rows, complete: the six planes' share of them): the
      selection reads these bytes once and writes next to nothing, the copy reads and writes them — the yardstick.
One JSON line per shape and form: medians in ms, (a) - (b), the copy's ms, and the device scratch of both routes in bytes
(computed from the shapes: the panel's planes plus the splits against the float matrix plus the former call's sums).
    python tools/bench_dosage_topk.py [--reps 7] [--shapes 8192,16384] [--samples 2048] [--k 16] [--panel-rows 0] > out.jsonl
The kernels' own times: `rocprofv3 --kernel-trace --stats -- python tools/bench_dosage_topk.py ...` in a run of its own."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stormbitmaps_amd as sb  # noqa: E402


def pack(G):
    n, S = G.shape
    v = np.zeros((n, (S + 31) // 32 * 32), dtype=np.uint64)
    v[:, :S] = G
    return (v.reshape(n, -1, 32) << (np.arange(32, dtype=np.uint64) * np.uint64(2))).sum(axis=2, dtype=np.uint64)


def container(words, S):
    d = sb.StormDosage(S)
    d.add_packed(words)
    return d


def up(x, m):
    return (x + m - 1) // m * m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="8192,16384")
    ap.add_argument("--samples", type=int, default=2048)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--panel-rows", type=int, default=0)
    a = ap.parse_args()
    import torch
    lib = sb.load()
    S, k = a.samples, a.k

    def ok(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} -> {rc}: {lib.STORM_hip_error().decode()}")

    for shape in a.shapes.split(","):
        n = int(shape)
        rng = np.random.default_rng(n)
        p = rng.uniform(0.05, 0.95, size=(n, 1))
        G = (rng.random((n, S)) < p).astype(np.uint8) + (rng.random((n, S)) < p).astype(np.uint8)
        for complete in (False, True):
            if complete:
                G[rng.random((n, S)) < 0.05] = 3
            words = pack(G)
            whole = container(words, S)
            ld, rows128 = up(n, 4), up(n, 128)
            plane_words = ld + 2 * ld + 2 * rows128 + ld if complete else ld
            panel = a.panel_rows or max(256, (256 << 20) // (4 * plane_words) // 256 * 256)
            panel = min(panel, up(n, 256))
            starts = list(range(0, n, panel))
            parts = [container(words[p0:p0 + panel], S) for p0 in starts]
            rect = torch.zeros((panel, ld), dtype=torch.int32, device="cuda:0")
            planes = torch.zeros((panel, plane_words), dtype=torch.int32, device="cuda:0")
            dst = torch.empty_like(planes)
            full = torch.zeros((n, n), dtype=torch.float32, device="cuda:0")
            idx = torch.zeros((n, k), dtype=torch.int32, device="cuda:0")
            val = torch.zeros((n, k), dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            tail = "_complete" if complete else ""

            def topk():
                ok(getattr(lib, f"STORM_dosage_pairw_topk{tail}_device")(whole._h, 0, k, a.panel_rows, C.c_void_p(idx.data_ptr()),
                                                                         C.c_void_p(val.data_ptr()), n, k), "topk")

            def rectangles():
                for part in parts:
                    if complete:
                        ok(lib.STORM_dosage_square_corr_complete_device(part._h, whole._h, 0, C.c_void_p(rect.data_ptr()), panel, ld), "rect")
                    else:
                        ok(lib.STORM_dosage_square_dot_device(part._h, whole._h, C.c_void_p(rect.data_ptr()), panel, ld), "rect")

            def former():
                ok(getattr(lib, f"STORM_dosage_square_corr{tail}_device")(whole._h, whole._h, 0, C.c_void_p(full.data_ptr()), n, n), "corr")
                full.fill_diagonal_(float("-inf"))
                torch.nan_to_num_(full, nan=float("-inf"))
                v, i = torch.topk(full, k, dim=1)
                torch.cuda.synchronize()
                return v, i

            def copy():
                for p0 in starts:
                    rows = min(panel, n - p0)
                    dst[:rows].copy_(planes[:rows])
                torch.cuda.synchronize()

            calls = {"topk": topk, "rectangles": rectangles, "former": former, "copy": copy}
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
            # the two routes agree on the values (the order within ties is torch's own)
            topk()
            v, _ = former()
            mine = val.clone()
            mine[torch.isnan(mine)] = float("-inf")
            same = bool(torch.equal(mine, v))
            stride_words = up(words.shape[1], 64)
            split_bytes = 3 * rows128 * stride_words * 8 if complete else 0
            rec = {"shape": shape, "rows": n, "samples": S, "k": k, "complete": complete, "reps": a.reps, "panel_rows": panel,
                   "panels": len(starts), "values_equal_former_route": same,
                   "topk_ms": round(med["topk"], 4), "rectangles_ms": round(med["rectangles"], 4),
                   "topk_minus_rectangles_ms": round(med["topk"] - med["rectangles"], 4),
                   "former_route_ms": round(med["former"], 4), "copy_ms": round(med["copy"], 4),
                   "copy_GBps": round(8 * n * plane_words / med["copy"] / 1e6, 1),
                   "scratch_bytes_topk": 4 * panel * plane_words + split_bytes + 8 * n,
                   "scratch_bytes_former": 4 * n * n + (4 * ((rows128 + n) * ld + n * (2 * rows128 + ld)) + split_bytes if complete else 0)
                   + 12 * n * k,
                   "min_ms": {key: round(min(v), 4) for key, v in ts.items()}}
            print(json.dumps(rec), flush=True)
            for part in parts:
                part.free()
            whole.free()
            del rect, planes, dst, full, idx, val
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
