"""The seeded parity sweep of the dosage containers' top-k calls (STORM_dosage_pairw_topk, STORM_dosage_square_topk and their
_complete forms): every case is drawn from (SEED, index) — the rows of both sides (1 .. 700), the samples (1 .. 3000, never a
multiple of 32), k (1 .. 128), panel_rows (0, 256, 512), the form (pairw, square, or square with a == b, each plain or
pairwise-complete), the score, the missing share, the pitch of the device output — and checked by the rule of
tests/test_gpu_dosage_topk.py: the values of STORM_dosage_square_corr[_complete] (numpy dot products for the dot score)
ranked by tests/test_gpu_topk.py's `rank` and `top`; idx and val of the host and the _device form EQUAL to that bit for bit.

COUNT cases. A failure names (seed, index) and prints the record; one case replays with
    python -m tests.test_gpu_sweep_dosage_topk --case I"""
import argparse
import json
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 20
COUNT = 24
FORMS = ("pairw", "square", "self")          # self: square with a == b (a row lists itself)
MISSING = (0.0, 0.02, 0.1, 0.5)


def cases(count=COUNT):
    rng = np.random.default_rng([2000, SEED])
    for index in range(count):
        samples = int(rng.integers(1, 3001))
        samples += samples % 32 == 0
        complete = bool(rng.integers(0, 2))
        yield {"seed": SEED, "index": index, "na": int(rng.integers(1, 701)), "nb": int(rng.integers(1, 701)), "S": samples,
               "k": int(rng.integers(1, 129)), "panel_rows": int(rng.choice((0, 256, 512))), "form": str(rng.choice(FORMS)),
               "complete": complete, "score": str(rng.choice(("r2", "r") if complete else ("r2", "r", "dot"))),
               "missing": float(rng.choice(MISSING)), "pad": int(rng.integers(0, 4)), "input_seed": int(rng.integers(1 << 31))}


def _rows(rng, n, S, missing):
    """0 / 1 / 2 with an allele frequency per row, 3 at `missing` of the samples; now and then a constant row and a copy"""
    p = rng.uniform(0.05, 0.95, size=(n, 1))
    G = (rng.random((n, S)) < p).astype(np.uint8) + (rng.random((n, S)) < p).astype(np.uint8)
    G[rng.random((n, S)) < missing] = 3
    if n > 2:
        G[rng.integers(n)] = rng.integers(0, 3)
        G[rng.integers(n)] = G[rng.integers(n)]
    return G


def run_case(rec):
    from tests.test_gpu_dosage_topk import container, device_form, host_form, kind, values
    from tests.test_gpu_topk import assert_topk, rank, top
    rng = np.random.default_rng(rec["input_seed"])
    Ga = _rows(rng, rec["na"], rec["S"], rec["missing"])
    Gb = Ga if rec["form"] != "square" else _rows(rng, rec["nb"], rec["S"], rec["missing"])
    a = container(Ga)
    b = a if rec["form"] != "square" else container(Gb)
    try:
        score, k, kw = rec["score"], rec["k"], dict(complete=rec["complete"], panel_rows=rec["panel_rows"])
        ranked = rank(values(a, b, Ga, Gb, score, rec["complete"]), kind(score), skip0=0 if rec["form"] == "pairw" else None)
        want = top(ranked, k, kind(score))
        other = None if rec["form"] == "pairw" else b
        assert_topk(device_form(a, other, score, k, k + rec["pad"], **kw), want, "device form")
        assert_topk(host_form(a, other, score, k, **kw), want, "host form")
    finally:
        a.free()
        if b is not a:
            b.free()


def run(count=COUNT, only=None):
    done = 0
    for rec in cases(count):
        if only is not None and rec["index"] != only:
            continue
        try:
            run_case(rec)
        except AssertionError as e:
            raise AssertionError(f"dosage_topk sweep, seed {rec['seed']} case {rec['index']}: {e}\nrecord: {json.dumps(rec)}\n"
                                 f"replay: python -m tests.test_gpu_sweep_dosage_topk --case {rec['index']}") from e
        done += 1
    return done


def test_dosage_topk_sweep():
    drawn = list(cases())
    assert {r["form"] for r in drawn} == set(FORMS) and {r["complete"] for r in drawn} == {False, True}
    assert {r["score"] for r in drawn} == {"r2", "r", "dot"} and {r["panel_rows"] for r in drawn} == {0, 256, 512}
    assert all(r["S"] % 32 for r in drawn)
    assert run() == COUNT


def main(argv=None):
    ap = argparse.ArgumentParser(description="replays one case of the dosage_topk sweep")
    ap.add_argument("--case", type=int, required=True)
    args = ap.parse_args(argv)
    print(json.dumps(next(r for r in cases(args.case + 1) if r["index"] == args.case)))
    run(args.case + 1, only=args.case)
    return 0


if __name__ == "__main__":
    sys.exit(main())
