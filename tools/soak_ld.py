#!/usr/bin/env python3
"""Randomised parity soak of the lag, dosage, LD and top-k calls on the GPU: the families of tests/_sweep.py — bit
containers, top-k, dosage n x n and rectangle, dosage in the lag layout, LD scores, pruning, and the sessions of interleaved
calls and mutations on live containers — drawn from seeds the suite does not use, each case compared with plain numpy on the unpacked rows, for a bounded time. For whoever changes these
kernels; the suite does not run it. Prints one JSON line; exit code 1 on the first mismatch (the line names the case and
its replay command).   soak_ld.py [--seconds 240] [--seed 1] [--family F]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import _sweep  # noqa: E402  (numpy only at module level)

BATCH = 8          # cases of one family drawn from one seed before the next family's turn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--family", choices=_sweep.FAMILIES + (_sweep.SESSION,), default=None)
    args = ap.parse_args()
    import stormbitmaps_amd as sb
    families = _sweep.FAMILIES + (_sweep.SESSION,) if args.family is None else (args.family,)
    ctx = sb.HipContext(0)
    t0 = time.time()
    totals = {f: _sweep.Stats() for f in families}
    seconds = {f: 0.0 for f in families}
    failure = None
    round_ = 0
    while failure is None and time.time() - t0 < args.seconds:
        for family in families:
            # seeds from 1000 on: the suite's own are 1, 2, 3
            seed = 1000 * args.seed + round_
            t1 = time.time()
            for rec in _sweep.cases(family, seed, BATCH):
                try:
                    totals[family].merge(_sweep.run_case(family, rec, ctx))
                except AssertionError as e:
                    failure = {"family": family, "seed": seed, "index": rec["index"], "message": str(e)}
                    break
                if time.time() - t0 >= args.seconds:
                    break
            seconds[family] += time.time() - t1
            if failure is not None or time.time() - t0 >= args.seconds:
                break
        round_ += 1
    ctx.close()
    print(json.dumps({"tool": "soak_ld", "seed": args.seed, "seconds": round(time.time() - t0, 1), "ok": failure is None,
                      "families": {f: dict(totals[f].as_dict(), seconds=round(seconds[f], 1)) for f in families},
                      "failure": failure}))
    return 0 if failure is None else 1


if __name__ == "__main__":
    sys.exit(main())
