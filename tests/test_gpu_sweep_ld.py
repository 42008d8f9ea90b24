"""The seeded parity sweep of the calls merged after the round-6 soak: the similarity matrices, the lag layout, top-k, the
2-bit dosage container with its n x n, rectangle and lag calls, the pairwise-complete forms, LD scores, stratified LD scores
and pruning. tests/_sweep.py draws every case from (family, seed) — shapes, lags, k, measures, missing shares, containers,
windows, pitches — builds its inputs, and compares every call, in its host and its _device form, with plain numpy on the
unpacked rows (float64 products of 0/1 or 0/1/2/3 matrices, exact; ratios and NaN masks from those integers). Nothing the
library computed is a reference here. Device outputs are sentinel-filled with guard rows and pitch columns, which must come
back untouched.

One test per family, seeds (1, 2, 3), COUNT cases per seed. A failure names (family, seed, index), prints the record and the
replay command: python -m tests._sweep --family F --seed S --case I. tests/test_sweep_cases.py shows on the CPU that these very
seeds and counts reach the edges and that the references agree with per-sample loops and the headers' host builds.

Pass conditions (tests/_sweep.py): integers equal; similarities and correlations the one NaN pattern exactly on the integer
mask and at most 1 ulp elsewhere (tests/test_gpu_similarity.py's `check` against the exactly rounded rational for the bit
containers, float32 of the float64 value for the dosages); top-k by count equal to numpy's ranking, by a float score the
five properties of _sweep.check_topk_floats; LD scores within 2^-22 (sum |t| + 1), stratified ones within
2^-22 (sum |t a| + max |a|) of the float64 sums (tests/test_gpu_ldscore*.py's bounds for this very comparison); keep and owner
equal to tests/_prune.greedy over the float64 r^2, min_r2 placed 2^-20 or more (relative) from every in-window r^2."""
import time

import pytest

from tests import _sweep

pytestmark = pytest.mark.gpu

SEEDS = (1, 2, 3)
# cases per seed, and the wall time of one seed of the family on one MI355X (host references included)
COUNT = {
    "bits": 32,         # 2.4 / 2.5 / 2.9 s for seeds 1 / 2 / 3
    "topk": 40,         # 2.0 / 1.9 / 2.5 s
    "dosage": 96,       # 2.6 / 2.0 / 2.4 s
    "dosage_lag": 96,   # 2.1 / 1.6 / 1.7 s
    "ldscore": 48,      # 1.9 / 1.1 / 1.3 s
    "prune": 120,       # 1.7 / 1.4 / 1.2 s
}


def _sweep_family(hip_ctx, family, seed):
    t0 = time.perf_counter()
    stats = _sweep.run_family(family, seed, COUNT[family], hip_ctx)
    assert stats.cases == COUNT[family]
    print(f"\nsweep {family} seed {seed}: {stats.cases} cases in {time.perf_counter() - t0:.2f} s, worst {stats.worst_ulp} ulp, "
          f"worst error / bound {stats.worst_ratio:.4f}" + (f", smallest margin {stats.min_margin:.3g}" if family == "prune" else ""))


@pytest.mark.parametrize("seed", SEEDS)
def test_bit_containers(lib, hip_ctx, seed):
    """StormContig, Storm (list-only, with a bitmap block, two of unequal width) and HipMatrix: pairw_similarity,
    square_similarity, pairw_lag_matrix for and / or / xor, pairw_lag_similarity for the four measures"""
    _sweep_family(hip_ctx, "bits", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_topk(lib, hip_ctx, seed):
    """pairw_topk, Storm.square_topk, HipMatrix.cross_topk over the five scores, k and panel_rows drawn. By count: idx and
    val equal to numpy's ranking. By a float score the reference is the float64 value, and a device value may sit one float
    from it, so two columns one ulp apart may swap: the five properties of _sweep.check_topk_floats are asserted instead. The
    fifth — no unlisted candidate's float32 reference exceeds the last listed value by more than 2 ulps — allows one ulp
    for each of the two values compared: the unlisted column's device float, which the kernel ranked at or below the last
    listed one, may lie 1 ulp under its reference, and the last listed device float 1 ulp over its own."""
    _sweep_family(hip_ctx, "topk", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_dosage_square_and_rectangle(lib, hip_ctx, seed):
    """pairw_dot, row_sums, pairw_corr, square_dot, row_missing, pairw_nobs, pairw_corr_complete; without a missing value the
    complete form gives the plain form's bits"""
    _sweep_family(hip_ctx, "dosage", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_dosage_lag_layout(lib, hip_ctx, seed):
    """pairw_lag_dot, pairw_lag_corr, pairw_lag_nobs, pairw_lag_corr_complete: the references at the pairs of the band, and the
    n x n call's bits there"""
    _sweep_family(hip_ctx, "dosage_lag", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_ld_scores(lib, hip_ctx, seed):
    """lag_ldscore (r2, r2_adj; plain and complete) and lag_ldscore_annot with and without positions, end to end from the
    float64 r^2 of the unpacked rows; a max_lag one below what the windows need is refused with nothing written"""
    _sweep_family(hip_ctx, "ldscore", seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_pruning(lib, hip_ctx, seed):
    """lag_prune, plain and complete, with and without priorities and positions, with owners, against the greedy over the
    edges of the float64 r^2"""
    _sweep_family(hip_ctx, "prune", seed)
