"""storm_prune_order.c — the order planner of the prune / clump calls — built stand-alone by the host C compiler: higher
priority first, ties (and -0.0 against +0.0) to the lower row, +-inf at the ends, a NaN refused with its row and nothing
written, NULL priorities the identity, 0, 1 and 2 rows. No device, no other source of the library."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NAN, TOO_MANY = 0, 1, 2
GUARD = np.uint32(0xDEADBEEF)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    cc = shutil.which("cc") or shutil.which("gcc")
    assert cc, "a host C compiler"
    so = tmp_path_factory.mktemp("prune_order") / "libprune_order.so"
    csrc = os.path.join(ROOT, "stormbitmaps_amd", "csrc")
    subprocess.run([cc, "-O2", "-std=gnu11", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I", csrc,
                    os.path.join(csrc, "storm_prune_order.c"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.storm_prune_order_plan.restype = C.c_int
    lib.storm_prune_order_plan.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]

    def run(priority, n, want_rank=True):
        order = np.full(n + 2, GUARD, dtype=np.uint32)
        rank = np.full(n + 2, GUARD, dtype=np.uint32)
        bad = C.c_uint64(777)
        p = None if priority is None else np.ascontiguousarray(priority, dtype=np.float32)
        code = lib.storm_prune_order_plan(None if p is None else p.ctypes.data, n, order.ctypes.data,
                                          rank.ctypes.data if want_rank else None, C.byref(bad))
        assert (order[n:] == GUARD).all() and (rank[n:] == GUARD).all()
        return code, order[:n], rank[:n], bad.value
    run.lib = lib
    return run


def reference(priority):
    p = np.asarray(priority, dtype=np.float32)
    return np.lexsort((np.arange(len(p)), -p)).astype(np.uint32)


def test_null_priorities_are_the_identity(plan):
    for n in (0, 1, 2, 5, 1000):
        code, order, rank, _ = plan(None, n)
        assert code == OK and np.array_equal(order, np.arange(n)) and np.array_equal(rank, np.arange(n))


def test_the_smallest_shapes(plan):
    code, order, rank, _ = plan(np.zeros(0, np.float32), 0)
    assert code == OK and order.size == 0
    code, order, rank, _ = plan([3.0], 1)
    assert code == OK and order.tolist() == [0] and rank.tolist() == [0]
    for p, want in (([1.0, 2.0], [1, 0]), ([2.0, 1.0], [0, 1]), ([1.0, 1.0], [0, 1]), ([-np.inf, np.inf], [1, 0])):
        code, order, rank, _ = plan(p, 2)
        assert code == OK and order.tolist() == want and rank[order].tolist() == [0, 1]


def test_higher_first_and_ties_to_the_lower_row(plan):
    rng = np.random.default_rng(11)
    for n in (3, 7, 64, 65, 1000, 4097):
        for p in (rng.random(n, dtype=np.float32), rng.integers(0, 4, n).astype(np.float32), np.zeros(n, np.float32),
                  -np.arange(n, dtype=np.float32), np.arange(n, dtype=np.float32)):
            code, order, rank, _ = plan(p, n)
            assert code == OK and np.array_equal(order, reference(p))
            assert np.array_equal(rank[order], np.arange(n))
            code, order2, rank2, _ = plan(p, n, want_rank=False)           # rank may be NULL
            assert code == OK and np.array_equal(order2, order) and (rank2 == GUARD).all()
    code, order, _, _ = plan(np.zeros(9, np.float32), 9)
    assert order.tolist() == list(range(9))                                # all equal: the identity, as NULL


def test_infinities_and_the_two_zeros(plan):
    p = np.float32([0.5, -np.inf, np.inf, 0.0, -0.0, np.inf, -np.inf, 1e30])
    code, order, rank, _ = plan(p, len(p))
    assert code == OK and order.tolist() == [2, 5, 7, 0, 3, 4, 1, 6]       # -0.0 ties with +0.0: row 3 before row 4


def test_a_nan_priority_is_refused_with_its_row_and_nothing_written(plan):
    p = np.float32([1.0, 2.0, np.nan, 3.0, np.nan])
    code, order, rank, bad = plan(p, 5)
    assert code == NAN and bad == 2                                        # the first such row
    assert (order == GUARD).all() and (rank == GUARD).all()
    code, _, _, bad = plan(np.float32([np.nan]), 1)
    assert code == NAN and bad == 0


def test_more_rows_than_uint32_holds_are_refused_before_anything_is_read(plan):
    assert plan.lib.storm_prune_order_plan(None, 1 << 32, None, None, None) == TOO_MANY    # NULL arrays: nothing is touched
    one = np.float32([np.nan])
    assert plan.lib.storm_prune_order_plan(one.ctypes.data, 1 << 32, None, None, None) == TOO_MANY
