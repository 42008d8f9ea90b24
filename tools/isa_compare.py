#!/usr/bin/env python3
"""Are two builds' device code the same, kernel by kernel?

    hipcc <the Makefile's HIPFLAGS> [-DSTORM_HIP_PROBES] --cuda-device-only -S -c X.hip -o DIR/X.s   (for both trees)
    tools/isa_compare.py [--by-name] BEFORE_DIR AFTER_DIR [more pairs ...]

For every .s file of BEFORE_DIR: the set of kernel names, and per kernel its instruction text with the .amdhsa_kernel
descriptor that follows it, and its metadata entry (.vgpr_count, .sgpr_count, .group_segment_fixed_size, ...), compared by kernel name so
that the order of definitions does not matter (function-local label numbers are dropped with it). Lines that name files
(.file, .ident, paths) are dropped. Prints one line per file and every difference; exit status 1 if there is one.
--by-name: kernels are paired by their demangled name up to the parameter list (c++filt), for a change of signatures; the
mangled name reads as that name in both texts.
"""
import difflib
import os
import re
import subprocess
import sys

LOCAL_LABEL = re.compile(r"\.L(BB|func_end|func_begin|tmp|JTI)\d+(_\d+)?")
LOOP_HEADER = re.compile(r"(Header=|Loop )BB\d+_")   # (a loop comment names a label with the function's number in the file)


def clean(lines):
    out = []
    for ln in lines:
        s = ln.strip()
        if s.startswith((".file", ".ident", "; %bb.")) or "/" in s and (".hip" in s or ".inc" in s or ".h" in s):
            continue
        ln = LOOP_HEADER.sub(lambda m: m.group(1) + "BB_", ln.rstrip())
        out.append(LOCAL_LABEL.sub(lambda m: ".L" + m.group(1) + (m.group(2) and "_" + m.group(2).split("_")[1] or ""), ln))
    return out


def kernels_of(path):
    lines = open(path).read().split("\n")
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    found = {name: {} for name in names}
    i = 0
    while i < len(lines):
        ln = lines[i]
        head = ln.split(":")[0]
        if ln and not ln[0].isspace() and ln.endswith("; @" + head) and head in found:   # a kernel's body and, behind it, its descriptor
            j = i
            while not lines[j].startswith(".Lfunc_end"):
                j += 1
            found[head]["text"] = clean(lines[i:j])
            assert any(".end_amdhsa_kernel" in t for t in found[head]["text"]), head
            i = j
        elif ln.startswith("amdhsa.kernels:"):
            entry = []
            j = i + 1
            while j < len(lines) and (lines[j].startswith("  ") or not lines[j].strip()):
                if lines[j].startswith("  - ") and entry:
                    _file_entry(found, entry)
                    entry = []
                entry.append(lines[j])
                j += 1
            if entry:
                _file_entry(found, entry)
            i = j
        i += 1
    return found


def by_name(found):
    """The same kernels under 'ns::kernel<args>': the demangled name without 'void ' and the parameter list."""
    out = {}
    names = list(found)
    dems = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n") if names else []
    for name, dem in zip(names, dems):
        k = found[name]
        dem = dem[5:] if dem.startswith("void ") else dem
        depth, base = 0, dem
        for i, ch in enumerate(dem):
            depth += (ch == "<") - (ch == ">")
            if ch == "(" and depth == 0:
                base = dem[:i]
                break
        out[base] = {part: [ln.replace(name, base) for ln in lines] for part, lines in k.items()}
    return out


def _file_entry(found, entry):
    name = next(ln.split(":", 1)[1].strip() for ln in entry if ln.strip().lstrip("- ").startswith(".name:"))
    found[name]["metadata"] = clean(entry)


def compare(before_dir, after_dir, pair_by_name=False):
    differ = False
    for fn in sorted(f for f in os.listdir(before_dir) if f.endswith(".s")):
        a, b = kernels_of(os.path.join(before_dir, fn)), kernels_of(os.path.join(after_dir, fn))
        if pair_by_name:
            a, b = by_name(a), by_name(b)
        report = []
        if set(a) != set(b):
            report.append(f"  kernel names differ: only before {sorted(set(a) - set(b))}, only after {sorted(set(b) - set(a))}")
        for name in sorted(set(a) & set(b)):
            for part in ("text", "metadata"):
                if part not in a[name] or part not in b[name]:
                    report.append(f"  {name}: no {part} found")
                elif a[name][part] != b[name][part]:
                    report.append(f"  {name}: {part} differs")
                    report += ["    " + d for d in list(difflib.unified_diff(a[name][part], b[name][part], lineterm="", n=1))[:40]]
        print(f"{os.path.join(os.path.basename(before_dir), fn)}: {len(a)} kernels, " + ("DIFFERENT" if report else "identical"))
        for ln in report:
            print(ln)
        differ = differ or bool(report)
    return differ


if __name__ == "__main__":
    args = [x for x in sys.argv[1:] if x != "--by-name"]
    if len(args) < 2 or len(args) % 2:
        sys.exit(__doc__)
    bad = False
    for k in range(0, len(args), 2):
        bad = compare(args[k], args[k + 1], pair_by_name="--by-name" in sys.argv) or bad
    sys.exit(1 if bad else 0)
