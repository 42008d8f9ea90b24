"""Pins what the host-only planners and the option validation of libstorm_hip.so answer.

    python tests/golden/make_plan_digests.py            # rewrites plan_digests.json and option_checks.json

Run against a build of the commit whose behaviour is to be kept (the files in the tree were written by the commit
before the planners moved to storm_hip_plan.cpp and the options into one table); tests/test_plan_golden.py recomputes
both with the library in the tree and compares. STORM_HIP_LIB selects the library; the tools build (`make probes`,
libstorm_hip_probes.so next to the shipped library) is recorded as well when it is there. No device is touched.
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
PLAN_FILE = os.path.join(HERE, "plan_digests.json")
OPTION_FILE = os.path.join(HERE, "option_checks.json")

ROWS = (1, 2, 255, 256, 257, 1000, 2048, 4096, 6144, 8192, 10000, 20000)
WORDS = (1, 70, 1024, 1094, 8192)


def plan_digests(rows, words):
    """One SHA-256 per planner family over its sub-cases in a fixed order."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from stormbitmaps_amd import dist
    out = {}
    h = hashlib.sha256()
    shapings = (({}, (1, 2, 3, 8)),
                (dict(max_run=64, tail_run=16, tail_slices=1, lpt_rounds=0), (1, 2)),
                (dict(n_cus=64), (1, 2)))
    for kw, worlds in shapings:
        for world in worlds:
            for rank in range(world):
                for form in (0, 1):
                    for pair_space in (0, 1):
                        items, run = dist.strip_plan(rows, words, rank, world, form, pair_space, return_run=True, **kw)
                        h.update(items.tobytes() + b"|%d;" % run)
    out["strip"] = h.hexdigest()
    h = hashlib.sha256()
    for world in (1, 2, 8):
        for rank in range(world):
            for n_cus in (256, 64):
                segs, groups = dist.stream_plan(rows, words, rank, world, n_cus)
                h.update(segs.tobytes() + b"|%d;" % groups)
    out["stream"] = h.hexdigest()
    h = hashlib.sha256()
    for slots_per_cu in (0, 1, 2):
        for min_chunks in (1, 8):
            for n_rows_b in (0, 300):
                for n_cus in (256, 64):
                    items = dist.matrix_plan(rows, words, n_rows_b, n_cus=n_cus, slots_per_cu=slots_per_cu, min_chunks=min_chunks)
                    h.update(items.tobytes() + b";")
    out["matrix"] = h.hexdigest()
    return out


def all_plan_digests():
    return {f"{family}/{rows}x{words}": digest
            for rows in ROWS for words in WORDS for family, digest in plan_digests(rows, words).items()}


# key -> (kind, a, b, values of the tools build only): "range" [a, b]; "set" a = the values; "any": every value is taken
# (booleans, clamped and free options)
OPTIONS = {
    "variant": ("range", -1, 5, (5,)),
    "probe_bundle": ("set", (-1, 1, 4), None, ()),
    "sparse_probe": ("range", -1, 1, ()),
    "result_mailbox": ("any", 0, 0, ()),
    "sync_poll_us": ("range", 0, 1000000, ()),
    "matrix_lists": ("range", -1, 1, ()),
    "matrix_lists_kernel": ("range", 0, 2, ()),
    "matrix_lists_hash_min_log2": ("range", 3, 7, ()),
    "matrix_lists_debug": ("any", 0, 0, ()),
    "matrix_lists_density": ("range", 0, 10000, ()),
    "seg_rows": ("range", 1, 1 << 20, ()),
    "k2_stages_per_item": ("range", 1, 65536, ()),
    "k2_max_run": ("range", 0, 4096, ()),
    "k2_ring": ("set", (3, 4, 5, 11, 12, 13, 14, 15, 16, 17, 18, 26), None, (3, 5, 11, 12, 13, 14, 15, 16, 17, 18, 26)),
    "k2_shadow_budget_mb": ("range", 0, 1 << 22, ()),
    "k2_tile_shape": ("set", (0, 1, 2, 3, 4, 5, 6, 16, 32), None, (1, 16)),
    "k2_ring_sync": ("any", 0, 0, ()),
    "k2_wave_below": ("range", 0, 1 << 30, ()),
    "k2_part_slots": ("range", 0, 2, ()),
    "k2_part_min_chunks": ("range", 1, 4096, ()),
    "k2_part_narrow": ("any", 0, 0, ()),
    "k2_part_cost_diag": ("range", 10, 100, ()),
    "k2_ring_cost_diag": ("range", 5, 100, ()),
    "k2_ring_cost_ragged": ("range", 5, 100, ()),
    "k2_tile_cost_diag": ("range", 5, 100, ()),
    "k2_tile_cost_ragged": ("range", 5, 100, ()),
    "k2_strip_operands": ("range", 0, 6, (1, 3)),
    "k2_shard_pairs": ("any", 0, 0, ()),
    "k2_matrix_pad": ("any", 0, 0, ()),
    "k2_fold_inline": ("any", 0, 0, ()),
    "k2_wave_ring": ("set", (0, 3, 4, 6, 8), None, ()),
    "k2_stream_max_rows": ("range", 0, 1 << 31, ()),
    "k2_stream_groups_per_cu": ("range", 0, 255, ()),
    "k2_stream_min_piece": ("range", 1, 4096, ()),
    "k2_stream_min_run": ("range", 1, 4096, ()),
    "k2_stream_w3_1": ("range", 10, 1000, ()),
    "k2_stream_w3_2": ("range", 10, 1000, ()),
    "k2_shape": ("set", (16, 32), None, (32,)),
    "keep_shadow": ("any", 0, 0, ()),
    "k2_matrix_parts": ("any", 0, 0, ()),
    "k2_matrix_min_part": ("set", (4, 8, 32, 4096), None, ()),       # a multiple of 4 in 4 .. 4096
    "k2_matrix_split": ("any", 0, 0, ()),
    "k2_pitch_pad": ("set", (-1, 0, 128, 384, 65536), None, ()),     # -1 or a multiple of 128 in 0 .. 65536
    "k2_lds_pad": ("range", 0, 120 * 1024, ()),
    "k2_persistent": ("any", 0, 0, (1,)),
    "k2_lpt_rounds": ("range", 0, 63, ()),
    "k2_tail_slices": ("range", 0, 255, ()),
    "k2_tail_run": ("range", 1, 4096, ()),
    "k2_debug": ("any", 0, 0, (1, 16)),
    "time_kernels": ("any", 0, 0, ()),
    "chunks_per_item": ("range", 0, 4096, ()),
}


def option_values(spec):
    kind, a, b, tools = spec
    values = [-2, 1 << 40, *tools]
    if kind == "range":
        values += [a - 1, a, b, b + 1]
    elif kind == "set":
        members = sorted(a)
        values += [members[0] - 1, members[-1] + 1, *members]
        values += [next(v for v in range(members[0], members[-1]) if v not in members)]   # between two members
    else:
        values += [0, 1, 5]
    return sorted(set(values))


def option_checks(lib_path):
    """{"key=value": [return code, error text ("" on success)]} of storm_hip_option_check, from a fresh process image."""
    lib = C.CDLL(lib_path)
    lib.storm_hip_option_check.restype = C.c_int
    lib.storm_hip_option_check.argtypes = [C.c_char_p, C.c_int64]
    lib.storm_hip_last_error.restype = C.c_char_p
    out = {}
    cases = [(key, v) for key, spec in OPTIONS.items() for v in option_values(spec)]
    cases += [("no_such_option", 0), ("", 0)]
    for key, v in cases:
        rc = lib.storm_hip_option_check(key.encode(), v)
        out[f"{key}={v}"] = [rc, (lib.storm_hip_last_error() or b"").decode() if rc else ""]
    return out


def probes_lib():
    return os.path.join(ROOT, "stormbitmaps_amd", "libstorm_hip_probes.so")


def shipped_lib():
    return os.environ.get("STORM_HIP_LIB") or os.path.join(ROOT, "stormbitmaps_amd", "libstorm_hip.so")


def option_checks_in_child(lib_path):
    """The tools build exports the same symbols as the shipped one: load it in a process of its own."""
    code = "import json, sys; sys.path.insert(0, %r); import make_plan_digests as m; print(json.dumps(m.option_checks(%r)))" % (HERE, lib_path)
    return json.loads(subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True).stdout)


if __name__ == "__main__":
    with open(PLAN_FILE, "w") as f:
        json.dump(all_plan_digests(), f, indent=0, sort_keys=True)
        f.write("\n")
    checks = {"shipped": option_checks_in_child(shipped_lib())}
    if os.path.exists(probes_lib()):
        checks["probes"] = option_checks_in_child(probes_lib())
    with open(OPTION_FILE, "w") as f:
        json.dump(checks, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{PLAN_FILE}: {len(ROWS) * len(WORDS)} shapes x 3 families; {OPTION_FILE}: {', '.join(checks)}")
