"""The environment switches of INTEGRATION.md §G, on fresh processes.

The library reads its environment once per process (the device configuration at the first call, STORM_HIP_OPTIONS with the
first context, STORM_HIP_VARIANT & co. with every context), so no in-process test reaches it. Here the parent never loads the
library: it computes every expectation from the seeded inputs of tests/_env_child.py with the CPU oracle and the numpy
references of tests/_sweep.py, starts `python -m tests._env_child` with the variables set — one child at a time, each with a
time limit of 120 s — and reads the child's JSON. Every case asserts the results AND an observable that shows the switch was
read (a STORM_hip_last_pass mask, a stderr line, a refusal); where the library offers none the case says so.

A child that times out, dies of a signal or aborts fails its test at once, and every later test of this file fails without
starting another process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import _env_child as child
from tests._sweep import Stats, bit_counts, bit_ops, close_floats, corr_complete64, dosage_sums, upper

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAILED = child.ALL_PAIRS_FAILED
# include/storm_hip.h: STORM_HIP_RAN_*
RAN_POPCOUNT, RAN_LIST_PROBE, RAN_LISTS_MATRIX, RAN_TILES_OUT = 1, 32, 64, 128
RAN_MATRIX_CORES = 2 | 4 | 8 | 16            # FP4 tiles, FP4 strips, bit stream, bit strips
ONE_SLOT = "the output lives on ONE device"  # one_slot_or_refuse (storm_host.c)
_crashed = []


def run_child(env, *sections):
    """(results, stderr) of one child under `env` on top of an environment without any STORM_HIP_ switch (which library is
    loaded, STORM_HIP_LIB / STORM_HIP_RCCL, is the caller's business and stays)"""
    if _crashed:
        pytest.fail("no further child is started: an earlier one crashed or hung (%s)" % _crashed[0])
    full = {k: v for k, v in os.environ.items() if not k.startswith("STORM_HIP_") or k in ("STORM_HIP_LIB", "STORM_HIP_RCCL")}
    full.update(env)
    try:
        r = subprocess.run([sys.executable, "-m", "tests._env_child", *sections], cwd=ROOT, env=full, capture_output=True,
                           text=True, timeout=120)
    except subprocess.TimeoutExpired:
        _crashed.append("time limit under %r" % (env,))
        pytest.fail("the child under %r ran into its time limit" % (env,))
    if r.returncode < 0 or r.returncode in (134, 139):
        _crashed.append("exit status %d under %r" % (r.returncode, env))
        pytest.fail("the child under %r ended with status %d: %s" % (env, r.returncode, r.stderr[-2000:]))
    assert r.returncode == 0, (env, r.returncode, r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1]), r.stderr


def _dense01(rows, width):
    d = np.zeros((len(rows), width), dtype=np.uint8)
    for i, r in enumerate(rows):
        d[i, r] = 1
    return d


def _tri(counts):
    return np.triu(counts, 1).astype(np.uint32)


@pytest.fixture(scope="module")
def ref(orc):
    """every expectation, from the inputs alone; computed once and left unchanged"""
    x = child.inputs()
    n0 = child.CONTIG_ROWS
    w = {"x": x}
    w["contig"] = orc.contig(child.CONTIG_BITS, x["contig"][:n0]).pairw()
    w["contig_more"] = orc.contig(child.CONTIG_BITS, x["contig"]).pairw()
    c, a, b = bit_counts(_dense01(x["contig"], child.CONTIG_BITS))
    assert int(np.triu(c, 1).sum()) == w["contig_more"] and int(np.triu(c[:n0, :n0], 1).sum()) == w["contig"]
    w["contig_matrix"] = _tri(c)
    w["sparse_contig"] = orc.contig(child.CONTIG_BITS, x["sparse_contig"]).pairw()
    w["mixed"] = orc.storm(x["mixed"]).pairw()
    edited = list(x["mixed"])
    edited[child.VICTIM] = x["mixed_edited_row"]
    o = orc.storm(edited)
    w["mixed_edited"] = o.pairw()
    assert w["mixed_edited"] != w["mixed"]
    w["mixed_matrix"] = _tri(o.pair_counts())
    assert int(w["mixed_matrix"].sum(dtype=np.uint64)) == w["mixed_edited"]
    w["mixed_serialized_bytes"] = o.serialized_size()
    d = _dense01(x["lists"], 2 * 65536)
    c, a, b = bit_counts(d)
    w["lists_matrix"] = {op: _tri(m) for op, m in bit_ops(c, a, b).items()}
    w["lists"] = int(w["lists_matrix"]["and"].sum(dtype=np.uint64))
    assert w["lists"] == orc.storm(x["lists"]).pairw()
    n = len(x["lists"])
    words = (n + child.DEV_PAD + 1) // 2
    win = np.full((n, 2 * words), child.SENTINEL, dtype=np.uint32)
    win[:, :n][upper(n)] = w["lists_matrix"]["and"][upper(n)]
    w["lists_device"] = win                              # entries i >= j and the columns beyond n stay as they were
    rect = bit_counts(d[:100], d[100:])[0]
    w["square_matrix"] = rect.astype(np.uint32)
    w["square_total"] = int(rect.sum())
    w["diag"] = orc.wrapper_diag(x["diag"])
    w["square"] = orc.wrapper_square(x["square_a"], x["square_b"])
    w["r2"] = corr_complete64(dosage_sums(x["dosage"]), "r2")
    return w


# ------------------------------------------------------------------------------------------ what a child returned
def check_matrix(got, want, what, rc=0):
    assert got["rc"] == rc, (what, got["rc"], got["error"])
    assert got["shape"] == list(want.shape), (what, got["shape"])
    assert (got["sha"], got["sum"]) == (child.sha(want), int(want.sum(dtype=np.uint64))), \
        "%s differs from the reference (sum %d, reference %d)" % (what, got["sum"], int(want.sum(dtype=np.uint64)))


def values(entries):
    return [e["value"] for e in entries]


def check_totals(out, ref):
    """every all-pairs total a child holds equals the reference's"""
    want = {}
    if "contig" in out:
        want["contig"] = (values(out["contig"]["totals"]), [ref["contig"]] * 3)
        if "after_add" in out["contig"]:
            want["contig after the add"] = ([out["contig"]["after_add"]["value"]], [ref["contig_more"]])
    if "sparse_contig" in out:
        want["sparse contig"] = (values(out["sparse_contig"]["totals"]), [ref["sparse_contig"]] * 2)
    if "mixed" in out:
        m = out["mixed"]
        assert m["edit_rcs"] == [1, 1] and m["serialized_bytes"] == ref["mixed_serialized_bytes"]
        want["STORM_t"] = (values(m["totals"]), [ref["mixed"]] * 2)
        want["STORM_t after the edit"] = ([m["after_edit"]["value"]], [ref["mixed_edited"]])
        want["serialized"] = ([m["serialized"]["value"]], [ref["mixed_edited"]])
    if "lists" in out:
        want["list-only STORM_t"] = ([out["lists"]["total"]["value"]], [ref["lists"]])
    if "wrappers" in out:
        want["wrapper_diag"] = (values(out["wrappers"]["diag"]), [ref["diag"]] * 2)
        want["wrapper_square"] = ([out["wrappers"]["square"]["value"]], [ref["square"]])
    for what, (got, expected) in want.items():
        assert got == expected, (what, got, expected)


def check_host_matrices(out, ref):
    """the per-pair matrices that go to host memory: every configuration computes them (several slots: in bands)"""
    check_matrix(out["contig"]["matrix"], ref["contig_matrix"], "STORM_contig_pairw_matrix")
    check_matrix(out["mixed"]["matrix"], ref["mixed_matrix"], "STORM_pairw_matrix (mixed blocks)")
    for op in child.OPS:
        check_matrix(out["lists"]["matrix_" + op], ref["lists_matrix"][op], "STORM_pairw_matrix (lists) " + op)


def check_one_slot_calls(out, ref):
    """the calls that need ONE device slot and one process, where they are served"""
    check_matrix(out["lists"]["matrix_device"], ref["lists_device"], "STORM_pairw_matrix_device")
    assert out["lists"]["square_total"]["value"] == ref["square_total"]
    check_matrix(out["lists"]["square_matrix"], ref["square_matrix"], "STORM_square_matrix")
    check_dosage(out, ref)


def check_dosage(out, ref):
    d = out["dosage"]
    assert d["rc"] == 0, (d["rc"], d["error"])
    n = ref["x"]["dosage"].shape[0]
    bits = np.array(d["r2_bits"], dtype=np.uint32).reshape(n, n)
    assert (bits[~upper(n)] == 0).all()
    close_floats(Stats(), bits, *ref["r2"], upper(n), "STORM_dosage_pairw_corr_complete r2")


def check_everything(out, ref):
    check_totals(out, ref)
    check_host_matrices(out, ref)
    check_one_slot_calls(out, ref)


def check_refused(out, code_device=-5):
    """several device slots: what writes to ONE device's memory or reads one slot's operands is refused, in words"""
    lists = out["lists"]
    assert lists["matrix_device"]["rc"] == code_device and ONE_SLOT in lists["matrix_device"]["error"]
    assert lists["matrix_device"]["sum"] == child.SENTINEL * np.prod(lists["matrix_device"]["shape"])     # nothing written
    assert out["dosage"]["rc"] == -5 and ONE_SLOT in out["dosage"]["error"]
    assert not any(out["dosage"]["r2_bits"])
    check_square_refused(out)


def check_square_refused(out):
    """tests/test_gpu_square.py::test_shard_world_of_two_is_refused, reached through the environment"""
    lists = out["lists"]
    assert lists["square_total"]["value"] == FAILED and "ONE" in lists["square_total"]["error"]
    assert lists["square_matrix"]["rc"] == -3 and "ONE" in lists["square_matrix"]["error"]
    assert lists["square_matrix"]["sum"] == 9 * 100 * 100                                                   # nothing written


def dense_masks(out):
    return [e["pass"][0] for e in out["contig"]["totals"] + [out["contig"]["after_add"]]]


@pytest.fixture(scope="module")
def control(ref):
    out, err = run_child({})
    check_everything(out, ref)
    return out, err


# ------------------------------------------------------------------------------------------ the cases
def test_control_without_any_switch(control):
    out, err = control
    # the masks the other cases compare theirs with
    for mask in dense_masks(out):
        assert mask & RAN_MATRIX_CORES and not mask & RAN_POPCOUNT, mask
    assert all(e["pass"][0] & RAN_LIST_PROBE and e["pass"][2] > 0 for e in out["sparse_contig"]["totals"])
    assert out["lists"]["matrix_and"]["pass"][0] == RAN_LISTS_MATRIX
    assert out["lists"]["matrix_device"]["pass"][0] == RAN_LISTS_MATRIX
    assert {k: out["ctx"][k] for k in ("variant", "seg_rows", "chunks_per_item")} == {"variant": -1, "seg_rows": 256, "chunks_per_item": 0}
    assert "STORM_HIP_" not in err and "[rowlists_create]" not in err and "[build_arena]" not in err


@pytest.mark.parametrize("more", [{}, {"STORM_HIP_SEG_ROWS": "100", "STORM_HIP_CHUNKS_PER_ITEM": "2"}], ids=["alone", "seg_rows_chunks"])
def test_variant_2_runs_the_popcount_kernel(ref, control, more):
    out, err = run_child(dict({"STORM_HIP_VARIANT": "2"}, **more))
    check_everything(out, ref)
    assert dense_masks(out) == [RAN_POPCOUNT] * 4 and dense_masks(out) != dense_masks(control[0])
    # a context of the device library itself reads the same three variables: read back as options
    want = {"variant": 2, "seg_rows": int(more.get("STORM_HIP_SEG_ROWS", 256)), "chunks_per_item": int(more.get("STORM_HIP_CHUNKS_PER_ITEM", 0))}
    assert {k: out["ctx"][k] for k in want} == want
    assert out["ctx"]["variant_used"] == 2 and out["ctx"]["total"] == ref["diag"]
    assert "ignored" not in err


def test_variant_seg_rows_chunks_refuse_what_the_options_refuse(ref, control):
    """STORM_HIP_SEG_ROWS=0 divided by zero in the first popcount pass, a word stood for 0, and STORM_HIP_VARIANT took
    numbers the option refuses (5: a form of the tools build): they are the options' values now, reported and ignored
    otherwise"""
    out, err = run_child({"STORM_HIP_VARIANT": "2", "STORM_HIP_SEG_ROWS": "0", "STORM_HIP_CHUNKS_PER_ITEM": "many"})
    check_everything(out, ref)
    assert dense_masks(out) == [RAN_POPCOUNT] * 4
    assert {k: out["ctx"][k] for k in ("variant", "seg_rows", "chunks_per_item")} == {"variant": 2, "seg_rows": 256, "chunks_per_item": 0}
    assert 'libstorm_hip: STORM_HIP_SEG_ROWS: "0" ignored' in err and 'libstorm_hip: STORM_HIP_CHUNKS_PER_ITEM: "many" ignored' in err
    out, err = run_child({"STORM_HIP_VARIANT": "9"}, "contig", "ctx")
    check_totals(out, ref)
    assert dense_masks(out) == dense_masks(control[0]) and out["ctx"]["variant"] == -1
    assert 'libstorm_hip: STORM_HIP_VARIANT: "9" ignored' in err


def test_options_variant_2_and_no_matrix_lists(ref, control):
    out, err = run_child({"STORM_HIP_OPTIONS": "variant=2,matrix_lists=0"})
    check_everything(out, ref)
    assert dense_masks(out) == [RAN_POPCOUNT] * 4
    for form in ("matrix_and", "matrix_or", "matrix_xor", "matrix_device"):
        assert out["lists"][form]["pass"][0] == RAN_TILES_OUT, form
        assert control[0]["lists"][form]["pass"][0] == RAN_LISTS_MATRIX, form
    assert out["ctx"]["variant"] == -1       # (the options are for the contexts behind the storm.h handles alone)
    assert "ignored" not in err


# sixteen distinct keys at their defaults — all the library remembers — and a seventeenth
SIXTEEN = ("variant=-1,probe_bundle=-1,sparse_probe=-1,matrix_lists=-1,matrix_lists_kernel=0,matrix_lists_hash_min_log2=6,"
           "matrix_lists_density=80,seg_rows=256,chunks_per_item=0,k2_stages_per_item=32,k2_max_run=0,k2_strip_operands=0,"
           "k2_stream_max_rows=8192,k2_shard_pairs=0,k2_wave_below=400,k2_part_min_chunks=8")


def test_options_with_bad_entries_reports_each_and_applies_none_cut(ref, control):
    """A typo is reported, not dropped: one stderr line per bad entry. The string is longer than 511 bytes, which is where a
    fixed buffer used to cut it: byte 511 falls inside `matrix_lists_density=080`, whose cut form `matrix_lists_density=0` is
    valid and would send the list-only matrix to the dense replica (RAN_TILES_OUT). The copy is now as long as the string."""
    head = "varient=2,variant=,variant=2x,novalue," + SIXTEEN + ",k2_part_narrow=1,"
    tail = "matrix_lists_density=080"
    pad = "seg_rows=" + "0" * (511 - len(head) - len("seg_rows=256,") - len("matrix_lists_density=0")) + "256,"
    options = head + pad + tail
    assert len(SIXTEEN.split(",")) == 16 and len(options) > 511 and options[:511].endswith(",matrix_lists_density=0")
    out, err = run_child({"STORM_HIP_OPTIONS": options})
    check_everything(out, ref)
    lines = [ln for ln in err.splitlines() if "STORM_HIP_OPTIONS: entry" in ln]
    assert len(lines) == 5, lines
    for line, entry in zip(lines, ('"varient=2"', '"variant="', '"variant=2x"', '"novalue"', '"k2_part_narrow=1"')):
        assert line.startswith("libstorm_hip: STORM_HIP_OPTIONS: entry " + entry + " ignored"), line
    assert "was not applied" not in err
    assert dense_masks(out) == dense_masks(control[0])
    assert out["lists"]["matrix_and"]["pass"][0] == RAN_LISTS_MATRIX      # density 80, not 0


def test_contig_lists_0_keeps_a_sparse_contig_on_its_dense_mirror(ref, control):
    out, err = run_child({"STORM_HIP_CONTIG_LISTS": "0"})
    check_everything(out, ref)
    for e, c in zip(out["sparse_contig"]["totals"], control[0]["sparse_contig"]["totals"]):
        assert not e["pass"][0] & RAN_LIST_PROBE and e["pass"][2] == 0 and e["pass"][0] & RAN_MATRIX_CORES, e["pass"]
        assert c["pass"][0] & RAN_LIST_PROBE and c["pass"][2] > 0


def test_always_fingerprint(ref):
    """Observable: none. The "state, fingerprint" lap of STORM_HIP_TIMING is printed on every STORM_t total with or without
    the switch (the walk itself runs behind the launches and has no lap of its own), and an edit through the public row
    functions is seen either way, by the mutation epoch. What is asserted: the results, the total after the
    header-preserving edit among them, and that the laps are there."""
    out, err = run_child({"STORM_HIP_ALWAYS_FINGERPRINT": "1", "STORM_HIP_TIMING": "1"})
    check_everything(out, ref)
    assert err.count("[storm_host] state, fingerprint") >= 4


@pytest.mark.parametrize("kernel", [1, 2])
def test_lists_no_deal(ref, kernel):
    """Observable of STORM_HIP_LISTS_NO_DEAL itself: none public (it skips a launch that reorders cells inside the lists'
    arena). The mask shows that the kernels which read that arena ran."""
    out, err = run_child({"STORM_HIP_LISTS_NO_DEAL": "1", "STORM_HIP_OPTIONS": "matrix_lists=1,matrix_lists_kernel=%d" % kernel},
                         "lists")
    for op in child.OPS:
        check_matrix(out["lists"]["matrix_" + op], ref["lists_matrix"][op], "STORM_pairw_matrix (lists) " + op)
        assert out["lists"]["matrix_" + op]["pass"][0] == RAN_LISTS_MATRIX
    check_matrix(out["lists"]["matrix_device"], ref["lists_device"], "STORM_pairw_matrix_device")
    assert "ignored" not in err


def test_timing_changes_no_result(ref):
    out, err = run_child({"STORM_HIP_TIMING": "1"})
    check_everything(out, ref)
    assert "[rowlists_create]" in err and "[build_arena]" in err and "[storm_host] pass" in err
    assert "[rowlists_matrix] kernel by events" in err                    # the device form's branch with events
    assert out["lists"]["matrix_device"]["pass"][0] == RAN_LISTS_MATRIX


def _sum_of_partials(outs, ref):
    """per call family the partials of the ranks add up to the reference's total"""
    def add(path):
        total = 0
        for o in outs:
            e = o
            for k in path:
                e = e[k]
            assert e["value"] != FAILED, (path, e["error"])
            total += e["value"]
        return total
    for i in range(3):
        assert add(("contig", "totals", i)) == ref["contig"]
    assert add(("contig", "after_add")) == ref["contig_more"]
    for i in range(2):
        assert add(("sparse_contig", "totals", i)) == ref["sparse_contig"]
        assert add(("mixed", "totals", i)) == ref["mixed"]
        assert add(("wrappers", "diag", i)) == ref["diag"]
    assert add(("mixed", "after_edit")) == ref["mixed_edited"]
    assert add(("mixed", "serialized")) == ref["mixed_edited"]
    assert add(("lists", "total")) == ref["lists"]


def test_shard_r_of_3_partials_add_up(ref):
    outs = [run_child({"STORM_HIP_SHARD": "%d/3" % r})[0] for r in range(3)]
    _sum_of_partials(outs, ref)
    parts = [o["contig"]["totals"][0]["value"] for o in outs]
    assert sum(p > 0 for p in parts) >= 2 and all(p < ref["contig"] for p in parts), parts
    for o in outs:
        # STORM_wrapper_square is not split over shards: every process returns the whole rectangle
        assert o["wrappers"]["square"]["value"] == ref["square"]
        # the per-pair matrices and the dosage statistics are whole in every process; the rectangle of two containers is
        # refused in a world of several shards
        check_host_matrices(o, ref)
        check_matrix(o["lists"]["matrix_device"], ref["lists_device"], "STORM_pairw_matrix_device")
        check_dosage(o, ref)
        check_square_refused(o)


@pytest.mark.parametrize("value", ["3/3", "1/0", "1", "x"])
def test_malformed_shard_is_reported_and_leaves_the_process_unsharded(ref, value):
    out, err = run_child({"STORM_HIP_SHARD": value}, "contig", "total_only")
    assert values(out["contig"]["totals"]) == [ref["contig"]] * 3
    assert err.count('libstorm_hip: STORM_HIP_SHARD: "%s" ignored (rank/world expected, rank < world)' % value) == 1, err[-1000:]


@pytest.mark.parametrize("threads", [None, "0", "1"])
def test_three_slots_on_one_card(ref, threads):
    """STORM_HIP_DEVICES=0,0,0: every total over three shards, from the caller's thread (the same ordinal three times, or
    STORM_HIP_HOST_THREADS=0) or through the worker pool (=1; which thread drives which slot is asserted on the device stub,
    tests/test_host_pool_sanitize.py). The host forms of the per-pair matrices are written in bands by the three slots;
    what needs one slot is refused."""
    env = {"STORM_HIP_DEVICES": "0,0,0"}
    if threads is not None:
        env["STORM_HIP_HOST_THREADS"] = threads
    out, err = run_child(env)
    check_totals(out, ref)
    check_host_matrices(out, ref)
    check_refused(out)


def test_two_slots_times_two_shards_is_a_world_of_four(ref):
    outs = [run_child({"STORM_HIP_DEVICES": "0,0", "STORM_HIP_SHARD": "%d/2" % r}, "contig", "sparse_contig", "mixed", "lists",
                      "wrappers", "dosage")[0] for r in range(2)]
    _sum_of_partials(outs, ref)
    parts = [o["contig"]["totals"][0]["value"] for o in outs]
    assert all(0 < p < ref["contig"] for p in parts), parts
    for o in outs:
        check_refused(o)


def test_devices_all(ref):
    out, err = run_child({"STORM_HIP_DEVICES": "all"})
    check_totals(out, ref)
    check_host_matrices(out, ref)
    if out["ctx"]["device_count"] > 1:
        check_refused(out)
    else:
        check_one_slot_calls(out, ref)


@pytest.mark.parametrize("value", ["0,x", "x", "0,,1"])
def test_malformed_devices_is_reported_and_falls_back_to_device_0_alone(ref, value):
    out, err = run_child({"STORM_HIP_DEVICES": value}, "contig", "total_only", "dosage")
    assert values(out["contig"]["totals"]) == [ref["contig"]] * 3
    assert err.count('libstorm_hip: STORM_HIP_DEVICES: "%s" ignored' % value) == 1 and "device 0 alone" in err, err[-1000:]
    check_dosage(out, ref)                                                # ONE slot: with several this is refused (-5)


@pytest.mark.parametrize("value", ["-1", "99"])
def test_an_ordinal_that_names_no_device_fails_the_call_in_words(value):
    out, err = run_child({"STORM_HIP_DEVICES": value}, "contig", "total_only")
    for e in out["contig"]["totals"]:
        assert e["value"] == FAILED and ("device %s out of range" % value) in e["error"], e
    assert ("storm_hip_ctx_create: device %s out of range" % value) in err
