"""The seeded session sweep: what survives from one call to the next. tests/_sweep.py draws, from (family "session", seed), lists
of steps over a few LIVE containers — mutations (add, clear, free and create again, upload, resize, set_rows_from_positions,
import_device, hip_invalidate), changes of result-preserving options, and queries of every kind, interleaved —
keeps a numpy model of every container (bits 0 / 1; dosages 0 .. 3), applies each mutation to the model and to the library
alike, and answers every query from the model alone. The context's shared workspace (the item, strip and ticket lists, the
band, count, part and dosage scratch, the FP4 shadow) and the containers' device mirrors (arena, dense replica, row lists,
the incremental uploads) are what is under test: a stale key or a mirror that missed a row faults nothing and returns
plausible wrong numbers.

Two session kinds, one test each, seeds (1, 2, 3), COUNT records per seed (even indices "storm", odd "hip"):
  storm   one or two Storm, a StormContig and two StormDosage of one sample count on the library's own context
  hip     two or three HipMatrix on a HipContext the session creates and closes itself
tests/test_sweep_cases.py shows on the CPU, for these seeds and this count, that no mutation is invisible, that every
hand-over of a shared buffer between two query kinds occurs with both queries on the dense paths (not a Storm's lists or
arena), that every entry of the option tables is set, and that the named transitions occur.

Pass conditions (tests/_sweep.py, none of them new): integers equal; similarities and correlations the one NaN pattern
exactly on the integer mask and at most 1 ulp from float32 of the float64 value; top-k by count numpy's ranking, by a float
score the five properties of _sweep.check_topk_floats; LD scores within 2^-22 (sum |t| + 1), stratified ones within
2^-22 (sum |t a| + max |a|); keep and owner equal to tests/_prune.greedy with min_r2 2^-20 or more (relative) from every
in-window r^2; every device output sentinel-filled with guard rows and pitch columns that come back untouched.

A failure names (family, seed, index, step) and prints the steps up to the failing one and the replay command,
python -m tests._sweep --family session --seed S --case I --upto K. After a value mismatch the runner repeats the one query on
fresh containers built from the model: "a fresh container agrees: the session's state is at fault" is a bug in the library's
state keeping, "a fresh container differs too" one in the call itself."""
import time

import pytest

from tests import _sweep

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3)
# records per seed (six of each kind), and the wall time of one seed of a kind on one MI355X (host references included):
#   storm   0.88 / 0.96 / 0.73 s for seeds 1 / 2 / 3
#   hip     1.36 / 0.86 / 0.96 s
# Under the 3 s of the other families on purpose: well before the sixth session of a kind a seed's share of the hand-overs
# is used up and the option table walked (tests/test_sweep_cases.py); a further session would only repeat the scripted
# transitions.
COUNT = 12


def _sweep_sessions(hip_ctx, kind, seed):
    t0 = time.perf_counter()
    total = _sweep.Stats()
    for rec in _sweep.cases(_sweep.SESSION, seed, COUNT):
        if rec["kind"] == kind:
            total.merge(_sweep.run_case(_sweep.SESSION, rec, hip_ctx))
    assert total.cases == COUNT // 2
    print(f"\nsweep session {kind} seed {seed}: {total.cases} sessions in {time.perf_counter() - t0:.2f} s, worst {total.worst_ulp} ulp, "
          f"worst error / bound {total.worst_ratio:.4f}")


@pytest.mark.parametrize("seed", SEEDS)
def test_storm_sessions(lib, hip_ctx, seed):
    """Storm, StormContig and StormDosage on the library's own context: K5 eligibility lost to a bitmap block and regained
    behind clear, a dense replica widened by a square call, growth across 256 / 512 / 1024 rows and the first reallocation,
    incremental dosage uploads, clear with fewer rows, containers freed between another one's queries, and a tour of every
    hand-over of a shared buffer between two query kinds"""
    _sweep_sessions(hip_ctx, "storm", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_hip_sessions(lib, seed):
    """HipMatrix on a context of the session's own: upload into the middle under keep_shadow 1, set_rows_from_positions,
    import_device, clear, resize down and up inside the allocation and past it, destroy and create, between totals (sharded),
    rectangles, per-pair matrices and bands, similarities, the lag layout, top-k, and — the rows read as 2-bit dosages — the
    lag dot products, nobs, r / r^2 (plain and complete), LD scores (plain and stratified) and pruning; the option table is
    walked entry by entry"""
    _sweep_sessions(None, "hip", seed)
