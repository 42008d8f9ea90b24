"""Pins what the sparse arena's host-only planners answer (storm_hip_plan.cpp: plan_arena_columns, plan_arena_probe,
plan_probe_launch, plan_sparse_segments).

    python tests/golden/make_arena_digests.py            # rewrites arena_plan_digests.json

Run in a tree whose behaviour is to be kept (the file in the tree was written when the planner code had only been
moved out of build_arena, statement by statement, before it was reshaped); tests/test_arena_plan.py recomputes the
digests with the tree's code and compares. The cases come from fixed numpy seeds; tests/arena_plan/driver.cpp is built
with the host compiler and links storm_hip_plan.cpp only. No device is touched.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
DIGEST_FILE = os.path.join(HERE, "arena_plan_digests.json")
SOURCES = [os.path.join(ROOT, "tests", "arena_plan", "driver.cpp"),
           os.path.join(ROOT, "stormbitmaps_amd", "csrc", "storm_hip_plan.cpp")]
INCLUDES = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "stormbitmaps_amd", "csrc")]


def build_driver(exe, sanitize=False):
    flags = ["-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"] \
        if sanitize else ["-O2"]
    return subprocess.run(["g++", "-std=c++17", "-Wall", *flags, *INCLUDES, *SOURCES, "-o", str(exe)],
                          capture_output=True, text=True)


# ---- cases: a list of rows, a row = [(block id, kind, positions or None, ptr), ...] with ascending ids ----
def _positions(rng, n, lo=0, hi=65536):
    return np.sort(rng.choice(np.arange(lo, hi), size=n, replace=False)).astype(np.int64)


def _one_column(rng, n_bitmap, n_list, n_pos, lo=0, hi=65536, bitmaps_first=True):
    rows = [[(0, 1, None, 0)] for _ in range(n_bitmap)] if bitmaps_first else []
    for _ in range(n_list):
        n = int(rng.integers(max(1, n_pos - n_pos // 4), n_pos + n_pos // 4 + 1)) if n_pos > 4 else n_pos
        rows.append([(0, 0, _positions(rng, n, lo, hi), 0)])
    if not bitmaps_first:
        rows += [[(0, 1, None, 0)] for _ in range(n_bitmap)]
    return rows


def case_rows(name):
    rng = np.random.default_rng(sum(name.encode()) + 20260)
    if name == "A":
        return _one_column(rng, 0, 2, 5)
    if name == "B":
        return _one_column(rng, 3, 1, 5, bitmaps_first=False)
    if name == "C":
        return _one_column(rng, 5, 300, 10)
    if name in ("D128", "D129", "D513"):
        return _one_column(rng, 0, int(name[1:]), 40)
    if name == "E":
        return [[(0, 0, _positions(rng, 800), 0)] for _ in range(700)]
    if name == "F":
        rows = []
        for r in range(300):
            if r % 5 == 4:
                rows.append([])
                continue
            rows.append([(3 * c + 1, 0, _positions(rng, 0 if (r % 7 == 3 and c % 5 == 0) else int(rng.integers(8, 17))), 0)
                         for c in range(34)])
        return rows
    if name == "G0":
        return _one_column(rng, 0, 200, 20, 0, 8192)
    if name == "G7":
        return _one_column(rng, 0, 200, 20, 7 * 8192, 65536)
    raise KeyError(name)


VALID_CASES = ("A", "B", "C", "D128", "D129", "D513", "E", "F", "G0", "G7")
PROBE_CASES = tuple(c for c in VALID_CASES if c != "B")   # B has one list: no probe column


def case_text(rows, last_offset=None, overrides=()):
    offsets, blocks = [0], []
    for row in rows:
        for bid, kind, pos, ptr in row:
            if kind == 0 and not isinstance(pos, int):
                blocks.append(f"{bid} 0 {len(pos)} {ptr} " + " ".join(map(str, pos)))
            else:   # a bitmap block, or a list whose stated length has no values behind it
                blocks.append(f"{bid} {kind} {pos or 0} {ptr}")
        offsets.append(len(blocks))
    if last_offset is not None:
        offsets[-1] = last_offset
    lines = [f"{len(rows)} {len(blocks)}", " ".join(map(str, offsets)), *blocks, str(len(overrides))]
    lines += [" ".join(map(str, o)) for o in overrides]
    return "\n".join(lines) + "\n"


def invalid_cases():
    """name -> (case text, error text); every one is refused with STORM_HIP_EINVAL."""
    rng = np.random.default_rng(77)
    two = lambda: [[(0, 0, _positions(rng, 6), 0)], [(0, 0, _positions(rng, 6), 0)]]
    out = {}
    out["ids_not_ascending"] = (case_text([[(2, 0, _positions(rng, 4), 0), (1, 0, _positions(rng, 4), 0)]]),
                                "sparse_create: block ids of row 0 are not ascending")
    out["kind_2"] = (case_text([[(0, 2, None, 0)]]), "sparse_create: block kind 2")
    rows = two()
    rows[1] = [(0, 0, rows[1][0][2], 1)]
    out["odd_list_pointer"] = (case_text(rows),
                               "sparse_create: block 1 has no data (or a list that is too long or not 2-byte aligned)")
    out["block_n_65537"] = (case_text([[(0, 0, 65537, 0)]]),
                            "sparse_create: block 0 has no data (or a list that is too long or not 2-byte aligned)")
    out["csr_short"] = (case_text(two(), last_offset=1), "sparse_create: row_block_offset must run from 0 to n_blocks = 2")
    out["run_ends_backwards"] = (case_text(two(), overrides=[(1, 3, 0)]), "sparse_create: a list block is not strictly ascending")
    return out


def run_case(exe, text, tmp_dir, name):
    path = os.path.join(str(tmp_dir), f"case_{name}.txt")
    with open(path, "w") as f:
        f.write(text)
    run = subprocess.run([str(exe), path], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (name, run.returncode, run.stderr[-3000:])
    return json.loads(run.stdout), run.stderr


def digests_of(doc):
    """One SHA-256 per section of the driver's output."""
    return {section: hashlib.sha256(json.dumps(doc[section], sort_keys=True, separators=(",", ":")).encode()).hexdigest()
            for section in sorted(doc)}


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "arena_plan")
        build = build_driver(exe)
        if build.returncode:
            sys.exit(build.stderr)
        out = {}
        for name in VALID_CASES:
            for section, digest in digests_of(run_case(exe, case_text(case_rows(name)), tmp, name)[0]).items():
                out[f"{name}/{section}"] = digest
        for name, (text, _) in invalid_cases().items():
            out[f"H_{name}/status"] = digests_of(run_case(exe, text, tmp, name)[0])["status"]
    with open(DIGEST_FILE, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{DIGEST_FILE}: {len(out)} sections")
