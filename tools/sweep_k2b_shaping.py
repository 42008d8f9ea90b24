#!/usr/bin/env python3
"""Work-list shaping of K2b (k2_max_run, k2_tail_run, k2_tail_slices, k2_lpt_rounds) swept for one of its forms at one shape:
whole pass by HIP events, same process, one option away from the defaults at a time, the defaults first and last.
sweep_k2b_shaping.py [rows] [bits] [--opt=key=value ...]   (e.g. --opt=k2_strip_rows=128)"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import stormbitmaps_amd as sb

def bench(ctx, m, t, passes=150, warm_ms=30.0):
    stream = torch.cuda.current_stream()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_ms * 1e-3:
        for _ in range(20):
            m.pairw_launch(t.data_ptr(), 0, 1)
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    for _ in range(passes):
        m.pairw_launch(t.data_ptr(), 0, 1)
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / passes

def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rows = int(args[0]) if args else 10000
    bits = int(args[1]) if len(args) > 1 else 65536
    ctx = sb.HipContext(0, torch.cuda.current_stream().cuda_stream)
    fixed = {}
    for o in sys.argv[1:]:
        if o.startswith("--opt="):
            k, v = o[6:].split("="); ctx.set_option(k, int(v)); fixed[k] = int(v)
    t = torch.zeros(1, dtype=torch.int64, device="cuda:0")
    m = ctx.matrix(rows, bits // 64)
    m.fill_synthetic(bits, bits // 2, seed=42)
    want = m.column_identity()
    base = {"k2_max_run": 0, "k2_tail_run": 32, "k2_tail_slices": 3, "k2_lpt_rounds": 6}
    trials = [dict(base)]
    for k, vals in (("k2_max_run", (48, 64, 96, 128, 192)), ("k2_tail_run", (8, 16, 24, 48, 64)),
                    ("k2_tail_slices", (1, 2, 6, 12)), ("k2_lpt_rounds", (0, 12))):
        for v in vals:
            d = dict(base); d[k] = v; trials.append(d)
    trials.append(dict(base))
    for d in trials:
        for k, v in d.items():
            ctx.set_option(k, v)
        us = bench(ctx, m, t)
        ok = int(t.item()) == want
        print(json.dumps({"rows": rows, "bits": bits, **fixed, **d, "us": round(us, 2), "ok": ok,
                          "rows_used": ctx.get_option("k2_strip_rows_used"), "items": ctx.last_launch_info()["items"]}), flush=True)
    m.close(); ctx.close()

if __name__ == "__main__":
    main()
