"""The host-only planners and the option validation answer what they answered before they moved (storm_hip_plan.cpp,
the option table): digests and records written by tests/golden/make_plan_digests.py from the commit before the move.
No device is touched."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_plan_digests", os.path.join(HERE, "golden", "make_plan_digests.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(gen.PLAN_FILE) as f:
    PLAN_GOLDEN = json.load(f)
with open(gen.OPTION_FILE) as f:
    OPTION_GOLDEN = json.load(f)


def test_golden_covers_the_grid():
    assert sorted(PLAN_GOLDEN) == sorted(f"{family}/{rows}x{words}" for rows in gen.ROWS for words in gen.WORDS
                                         for family in ("strip", "stream", "matrix"))
    assert set(OPTION_GOLDEN) == {"shipped", "probes"}
    n_cases = sum(len(gen.option_values(spec)) for spec in gen.OPTIONS.values()) + 2
    assert len(OPTION_GOLDEN["shipped"]) == len(OPTION_GOLDEN["probes"]) == n_cases


@pytest.mark.parametrize("rows", gen.ROWS)
def test_planner_output_is_unchanged(rows):
    for words in gen.WORDS:
        for family, digest in gen.plan_digests(rows, words).items():
            assert digest == PLAN_GOLDEN[f"{family}/{rows}x{words}"], f"{family} plan of {rows} rows x {words} words changed"


def _compare(got, want):
    assert set(got) == set(want)
    wrong = {case: (got[case], want[case]) for case in want if got[case] != want[case]}
    assert not wrong, wrong


def test_option_checks_are_unchanged():
    _compare(gen.option_checks_in_child(gen.shipped_lib()), OPTION_GOLDEN["shipped"])


def test_option_checks_of_the_tools_build_are_unchanged():
    if not os.path.exists(gen.probes_lib()):
        pytest.skip("libstorm_hip_probes.so is not built (make -C stormbitmaps_amd/csrc probes)")
    _compare(gen.option_checks_in_child(gen.probes_lib()), OPTION_GOLDEN["probes"])
