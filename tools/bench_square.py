"""The rectangle of two STORM_t (STORM_intersect_cardinality_square, STORM_square_matrix_device) at BASELINE c4's shape:
A = rows 0-4999 and B = rows 5000-9999 of the 10000-row synthetic container. Per case (positions per row): first call
and steady ms of the total and of the device matrix, on the list join (K5x, option matrix_lists 1) and on the dense
replicas (matrix_lists 0), what the automatic rule picks, and the 10000-row union's STORM_pairw_matrix_device (K5 / dense
triangle) as the yardstick. One JSON line per case.
    python tools/bench_square.py [--half 5000] [--bits 524288] [--draws 104,524,2096,20971,262144] > out.jsonl
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_square.py ...` on its own."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import stormbitmaps_amd as sb  # noqa: E402

RAN_NAMES = {1: "popcount", 4: "fp4_strips", 64: "lists_matrix(K5)", 128: "tiles_out", 256: "lists_square(K5x)"}


def _ran(lib):
    rep = (C.c_uint64 * 4)()
    lib.STORM_hip_last_pass(rep)
    return [name for bit, name in RAN_NAMES.items() if rep[0] & bit]


def _ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(min(ts) * 1e3, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--half", type=int, default=5000)
    ap.add_argument("--bits", type=int, default=524288)
    ap.add_argument("--draws", default="104,524,2096,20971,262144")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    lib = sb.load()
    n = a.half
    for d in [int(x) for x in a.draws.split(",")]:
        rec = {"half_rows": n, "bits": a.bits, "draws": d}
        rect = torch.zeros((n, n), dtype=torch.int32, device="cuda:0")
        for name, lists in (("k5x", 1), ("dense", 0), ("auto", -1)):
            lib.STORM_hip_set_option(b"matrix_lists", lists)
            A, B = sb.Storm(), sb.Storm()     # fresh containers: the first call builds the device copies
            A.add_synthetic(a.bits, n, d, seed=42, row0=0)
            B.add_synthetic(a.bits, n, d, seed=42, row0=n)
            t0 = time.perf_counter()
            total = A.intersect_cardinality_square(B)
            first_total = round((time.perf_counter() - t0) * 1e3, 3)
            ran_total = _ran(lib)
            steady_total = _ms(lambda: A.intersect_cardinality_square(B), a.reps)
            t0 = time.perf_counter()
            A.square_matrix_device(B, rect.data_ptr(), n, n)
            first_dev = round((time.perf_counter() - t0) * 1e3, 3)
            ran_dev = _ran(lib)
            steady_dev = _ms(lambda: A.square_matrix_device(B, rect.data_ptr(), n, n), a.reps)
            rec[name] = {"total": total, "first_total_ms": first_total, "steady_total_ms": steady_total,
                         "ran_total": ran_total, "first_device_ms": first_dev, "steady_device_ms": steady_dev,
                         "ran_device": ran_dev, "sum_equals_total": int(rect.to(torch.int64).sum().item()) == total}
            A.free()
            B.free()
        del rect
        lib.STORM_hip_set_option(b"matrix_lists", -1)
        U = sb.Storm()
        U.add_synthetic(a.bits, 2 * n, d, seed=42, row0=0)
        tri = torch.zeros((2 * n, 2 * n), dtype=torch.int32, device="cuda:0")
        U.pairw_matrix_device(tri.data_ptr(), 2 * n, 2 * n)
        rec["union_pairw_matrix_device"] = {"steady_ms": _ms(lambda: U.pairw_matrix_device(tri.data_ptr(), 2 * n, 2 * n), a.reps),
                                            "ran": _ran(lib)}
        rec["totals_agree"] = rec["k5x"]["total"] == rec["dense"]["total"] == rec["auto"]["total"]
        del tri
        U.free()
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
