"""STORM_intersect_cardinality_square at the drop-in boundary, without a GPU: the symbol the reference declares
(storm.h:231) and never defines is exported with the reference's parameter list, the two rectangle extensions
(STORM_square_matrix, STORM_square_matrix_device) are exported, NULL handles are refused, and a real pair is refused
with a reason rather than computed on the CPU when no device is visible (with one, it is computed)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from stormbitmaps_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
FAILED = (1 << 64) - 1

# the reference's prototype, word for word (storm.h:231 of the upstream project)
REFERENCE_PROTOTYPE = ("uint64_t STORM_intersect_cardinality_square(const STORM_t* STORM_RESTRICT bitmap1, "
                       "const STORM_t* STORM_RESTRICT bitmap2);")

# A caller written against the reference header: it redeclares the prototype exactly as the reference has it (a
# conflicting declaration in include/storm.h would not compile) and calls it.
C_CALLER = r"""
#include <stdint.h>
#include <stdio.h>
#include "storm.h"
uint64_t STORM_intersect_cardinality_square(const STORM_t* STORM_RESTRICT bitmap1, const STORM_t* STORM_RESTRICT bitmap2);
int main(void) {
    STORM_t* a = STORM_new();
    STORM_t* b = STORM_new();
    const uint32_t r0[] = {1, 5, 70000}, r1[] = {5, 9}, r2[] = {1, 5, 9, 70000};
    if (STORM_intersect_cardinality_square(NULL, b) != (uint64_t)-1) return 2;
    if (STORM_intersect_cardinality_square(a, NULL) != (uint64_t)-1) return 3;
    if (STORM_intersect_cardinality_square(a, b) != 0) return 4;  /* both empty */
    STORM_add(a, r0, 3);
    STORM_add(a, r1, 2);
    if (STORM_intersect_cardinality_square(a, b) != 0) return 5;  /* b empty */
    STORM_add(b, r2, 4);
    /* |r0 & r2| + |r1 & r2| = 3 + 2 */
    printf("%llu\n", (unsigned long long)STORM_intersect_cardinality_square(a, b));
    printf("%s\n", STORM_hip_error());
    STORM_free(a);
    STORM_free(b);
    return 0;
}
"""


def _no_gpu(lib):
    return lib.storm_hip_device_count() == 0


def test_square_symbols_are_exported(lib):
    for name in ("STORM_intersect_cardinality_square", "STORM_square_matrix", "STORM_square_matrix_device",
                 "storm_hip_rowlists_square_total", "storm_hip_rowlists_square_matrix_device",
                 "storm_hip_cross_dense_total", "storm_hip_matrix_create_from_blocks_wide"):
        assert hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"STORM_intersect_cardinality_square", "STORM_square_matrix", "STORM_square_matrix_device"} <= names


def test_header_declares_the_reference_prototype():
    src = open(os.path.join(INC, "storm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = re.search(r"uint64_t\s+STORM_intersect_cardinality_square\s*\([^;]*\);", src)
    assert decl, "include/storm.h does not declare STORM_intersect_cardinality_square"
    norm = lambda s: re.sub(r"\s*([(),;*])\s*", r"\1", re.sub(r"\s+", " ", s)).strip()
    assert norm(decl.group(0)) == norm(REFERENCE_PROTOTYPE)
    assert re.search(r"int\s+STORM_square_matrix\s*\(\s*STORM_t\s*\*\s*a\s*,\s*STORM_t\s*\*\s*b\s*,\s*int\s+op\s*,", src)
    assert re.search(r"int\s+STORM_square_matrix_device\s*\(", src)


def test_null_handles_and_buffers_are_refused(lib):
    sq = lib.STORM_intersect_cardinality_square
    sq.restype, sq.argtypes = C.c_uint64, [C.c_void_p, C.c_void_p]
    h = lib.STORM_new()
    buf = np.full(4, 7, dtype=np.uint32)
    try:
        assert sq(None, None) == FAILED
        assert sq(h, None) == FAILED
        assert sq(None, h) == FAILED
        assert b"NULL" in lib.STORM_hip_error()
        assert sq(h, h) == 0                              # empty: no device needed
        p = buf.ctypes.data_as(C.c_void_p)
        for fn in (lib.STORM_square_matrix, lib.STORM_square_matrix_device):
            assert fn(None, h, 0, p, 2, 2) == -1
            assert fn(h, None, 0, p, 2, 2) == -1
            assert fn(h, h, 0, None, 2, 2) == -2
        assert lib.STORM_square_matrix(h, h, 0, p, 2, 2) == 0   # empty: nothing to write
        assert (buf == 7).all()
    finally:
        lib.STORM_free(h)


def test_a_real_pair_is_refused_without_a_device(lib):
    a, b = lib.STORM_new(), lib.STORM_new()
    try:
        for h, rows in ((a, ([1, 5, 70000], [5, 9])), (b, ([1, 5, 9, 70000],))):
            for r in rows:
                v = np.array(r, dtype=np.uint32)
                assert lib.STORM_add(h, v.ctypes.data_as(C.c_void_p), v.size) == 1
        sq = lib.STORM_intersect_cardinality_square
        sq.restype, sq.argtypes = C.c_uint64, [C.c_void_p, C.c_void_p]
        got = sq(a, b)
        out = np.full((2, 1), 7, dtype=np.uint32)
        rc = lib.STORM_square_matrix(a, b, 0, out.ctypes.data_as(C.c_void_p), 2, 1)
        if _no_gpu(lib):
            assert got == FAILED
            assert lib.STORM_hip_error()          # the reason is given
            assert rc == -3 and (out == 7).all()  # and nothing was computed on the CPU
        else:
            assert got == 5
            assert rc == 0 and out[:, 0].tolist() == [3, 2]
    finally:
        lib.STORM_free(a)
        lib.STORM_free(b)


def test_a_c_caller_of_the_reference_prototype_links_and_runs(lib, tmp_path):
    src = tmp_path / "square_caller.c"
    exe = tmp_path / "square_caller"
    src.write_text(C_CALLER)
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", INC, "-o", str(exe), str(src), "-L", libdir,
                    "-lstorm_hip", "-Wl,-rpath," + libdir], check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stderr[-2000:])
    value, reason = res.stdout.splitlines()[:2]
    if _no_gpu(lib):
        assert int(value) == FAILED and reason, res.stdout
    else:
        assert int(value) == 5, res.stdout
