"""The seeded parity sweep of r / r^2 and N between two dosage containers (STORM_dosage_square_corr, _square_nobs,
_square_corr_complete), in the style of tests/test_gpu_sweep_ld.py: every case is drawn from (seed, index) — both row counts,
the samples, the missing share, the special rows of either side, the pitches of the host and the device output and the
device base's offset from a 16-byte boundary — with the draw and reference helpers of tests/_sweep.py, which stays as it
is. Each case is checked by the rule of tests/test_gpu_dosage_square.py: N equal, r and r^2 (plain and pairwise-complete) the
one NaN pattern exactly on the integer mask and at most 1 ulp from the float64 value elsewhere, host and _device forms bit
for bit alike, nothing written outside the n_a x n_b window.

COUNT cases per seed. A failure names (seed, index) and prints the record; one case replays with
    python -m tests.test_gpu_sweep_dosage_square --seed S --case I"""
import argparse
import json
import sys
import time

import numpy as np
import pytest

from tests import _sweep

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3)
COUNT = 40
FAMILY_ID = 1000            # (tests/_sweep.py's families count from 0)


def _side(rng, n, samples, missing):
    rec = {"n": n, "S": samples, "missing": missing, "input_seed": int(rng.integers(1 << 31))}
    _sweep._special_rows(rng, rec, n, samples)
    return rec


def cases(seed, count=COUNT):
    """`count` records: "a" and "b" are records tests/_sweep.dosage_matrix builds a side from (rows, samples, missing share,
    special rows, input seed); pad_host / pad_dev: the outputs' pitch columns; off: the device base's offset in words"""
    rng = np.random.default_rng([FAMILY_ID, int(seed)])
    for index in range(count):
        samples, missing = _sweep._draw_samples(rng), float(_sweep._pick(rng, _sweep.MISSING_SET))
        na = 1 if rng.random() < 0.1 else _sweep._draw_n(rng)
        nb = 1 if rng.random() < 0.1 else _sweep._draw_n(rng)
        yield {"seed": int(seed), "index": index, "a": _side(rng, na, samples, missing), "b": _side(rng, nb, samples, missing),
               "pad_host": int(rng.integers(0, 8)), "pad_dev": int(rng.integers(0, 8)), "off": int(_sweep._pick(rng, (0, 0, 1, 2, 3)))}


def run_case(rec, lib, stats):
    from tests.test_gpu_dosage_square import check_against_numpy, containers, close_all
    Ga, Gb = _sweep.dosage_matrix(rec["a"]), _sweep.dosage_matrix(rec["b"])
    a, b = containers(lib, Ga, Gb)
    try:
        check_against_numpy(a, b, Ga, Gb, stats, ld_host=b.n + rec["pad_host"], ld_dev=b.n + rec["pad_dev"], off=rec["off"])
    finally:
        close_all(a, b)
    stats.cases += 1


def run_seed(seed, lib, count=COUNT, only=None):
    stats = _sweep.Stats()
    for rec in cases(seed, count):
        if only is not None and rec["index"] != only:
            continue
        try:
            run_case(rec, lib, stats)
        except AssertionError as e:
            raise AssertionError(f"dosage_square sweep, seed {rec['seed']} case {rec['index']}: {e}\nrecord: {json.dumps(rec)}\n"
                                 f"replay: python -m tests.test_gpu_sweep_dosage_square --seed {rec['seed']} --case {rec['index']}"
                                 ) from e
    return stats


@pytest.mark.parametrize("seed", SEEDS)
def test_dosage_square_sweep(lib, seed):
    t0 = time.perf_counter()
    stats = run_seed(seed, lib)
    assert stats.cases == COUNT
    print(f"\nsweep dosage_square seed {seed}: {stats.cases} cases in {time.perf_counter() - t0:.2f} s, worst {stats.worst_ulp} ulp")


def main(argv=None):
    ap = argparse.ArgumentParser(description="replays one case of the dosage_square sweep")
    ap.add_argument("--seed", type=int, required=True)
    ap.add_argument("--case", type=int, required=True)
    args = ap.parse_args(argv)
    import stormbitmaps_amd as sb
    rec = next(r for r in cases(args.seed, args.case + 1) if r["index"] == args.case)
    print(json.dumps(rec))
    stats = run_seed(args.seed, sb.load(), args.case + 1, only=args.case)
    print(json.dumps(stats.as_dict()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
