"""The per-pair similarity entry points at the drop-in boundary, without a GPU: the six STORM_*_similarity* functions and
the shim functions behind them are exported, declared in the headers and bound in the Python table; arguments are
checked before any device is touched (-1 / -2 / -4 / -3 with a reason), empty containers write nothing, and a real
container is refused with a reason rather than computed on the CPU when no device is visible."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from stormbitmaps_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")

STORM_FNS = ("STORM_contig_pairw_similarity", "STORM_contig_pairw_similarity_device", "STORM_pairw_similarity",
             "STORM_pairw_similarity_device", "STORM_square_similarity", "STORM_square_similarity_device")
SHIM_FNS = ("storm_hip_similarity_finish_device", "storm_hip_pairw_similarity_device", "storm_hip_pairw_similarity",
            "storm_hip_cross_dense_similarity_device", "storm_hip_cross_dense_similarity",
            "storm_hip_rowlists_pairw_similarity_device", "storm_hip_rowlists_pairw_similarity",
            "storm_hip_rowlists_square_similarity_device", "storm_hip_rowlists_square_similarity")
JACCARD, COSINE, LD_D, LD_R2 = range(4)
SENTINEL = np.float32(-7.5)

C_CALLER = r"""
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "storm.h"
int main(void) {
    float out[4];
    const uint32_t r0[] = {1, 5, 9}, r1[] = {5, 9, 11};
    STORM_t* s = STORM_new();
    STORM_contiguous_t* c = STORM_contig_new(64);
    for (int i = 0; i < 4; ++i) out[i] = -7.5f;
    if (STORM_SIM_JACCARD != 0 || STORM_SIM_COSINE != 1 || STORM_SIM_LD_D != 2 || STORM_SIM_LD_R2 != 3) return 2;
    if (STORM_pairw_similarity(NULL, STORM_SIM_JACCARD, 0, out, 2, 2) != -1) return 3;
    if (STORM_contig_pairw_similarity(c, STORM_SIM_LD_R2, 0, NULL, 2, 2) != -2) return 4;
    if (STORM_square_similarity(s, s, STORM_SIM_COSINE, 0, out, 2, 2) != 0) return 5;   /* empty */
    if (STORM_pairw_similarity_device(s, 4, 0, out, 2, 2) != -3 || !STORM_hip_error()[0]) return 6;
    STORM_add(s, r0, 3);
    STORM_add(s, r1, 3);
    STORM_contig_add(c, r0, 3);
    STORM_contig_add(c, r1, 3);
    if (STORM_pairw_similarity(s, STORM_SIM_JACCARD, 0, out, 1, 2) != -4) return 7;
    if (STORM_contig_pairw_similarity(c, STORM_SIM_JACCARD, 0, out, 2, 1) != -4) return 8;
    for (int i = 0; i < 4; ++i) if (out[i] != -7.5f) return 9;
    /* |r0 & r1| = 2, |r0 | r1| = 4 */
    const int rc = STORM_pairw_similarity(s, STORM_SIM_JACCARD, 0, out, 2, 2);
    printf("%d %.9g\n", rc, (double)out[1]);
    printf("%s\n", STORM_hip_error());
    STORM_free(s);
    STORM_contig_free(c);
    return 0;
}
"""


def _no_gpu(lib):
    return lib.storm_hip_device_count() == 0


def _decl(src, name):
    return re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, src)


def _strip_comments(src):
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_similarity_symbols_are_exported_declared_and_bound(lib):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    storm_h = _strip_comments(open(os.path.join(INC, "storm.h")).read())
    shim_h = _strip_comments(open(os.path.join(INC, "storm_hip.h")).read())
    for name in STORM_FNS + SHIM_FNS:
        assert hasattr(lib, name), name
        assert name in names, name
        assert name in _lib.SIGNATURES, name
    for name in STORM_FNS:
        d = _decl(storm_h, name)
        assert d, name
        assert re.search(r"int\s+measure\s*,\s*uint64_t\s+n_bits\s*,\s*float\s*\*", d.group(1)), name
        assert re.search(r"uint64_t\s+out_rows\s*,\s*uint64_t\s+out_ld\s*$", d.group(1).strip()), name
    for name in SHIM_FNS:
        assert _decl(shim_h, name), name
    prim = re.sub(r"\s+", " ", _decl(shim_h, "storm_hip_similarity_finish_device").group(1))
    assert prim == ("storm_hip_ctx_t* ctx, void* d_io, uint64_t ld, uint64_t n_rows, uint64_t n_cols, "
                    "const uint32_t* d_counts_rows, const uint32_t* d_counts_cols, int triangle, int measure, uint64_t n_bits")
    for k, name in enumerate(("JACCARD", "COSINE", "LD_D", "LD_R2")):
        assert re.search(r"#define\s+STORM_SIM_%s\s+%d\b" % (name, k), storm_h)
    assert re.search(r"#define\s+STORM_HIP_RAN_SIMILARITY\s+512u", shim_h)


def _containers(lib, rows):
    s, c = lib.STORM_new(), lib.STORM_contig_new(4096)
    for r in rows:
        v = np.array(r, dtype=np.uint32)
        assert lib.STORM_add(s, v.ctypes.data_as(C.c_void_p), v.size) == 1
        assert lib.STORM_contig_add(c, v.ctypes.data_as(C.c_void_p), v.size) == v.size
    return s, c


def _calls(lib, s, c):
    """every entry point as f(measure, n_bits, out pointer, out_rows, out_ld) on the same two rows-by-two-rows shape"""
    return [
        ("STORM_contig_pairw_similarity", lambda *a: lib.STORM_contig_pairw_similarity(c, *a)),
        ("STORM_contig_pairw_similarity_device", lambda *a: lib.STORM_contig_pairw_similarity_device(c, *a)),
        ("STORM_pairw_similarity", lambda *a: lib.STORM_pairw_similarity(s, *a)),
        ("STORM_pairw_similarity_device", lambda *a: lib.STORM_pairw_similarity_device(s, *a)),
        ("STORM_square_similarity", lambda *a: lib.STORM_square_similarity(s, s, *a)),
        ("STORM_square_similarity_device", lambda *a: lib.STORM_square_similarity_device(s, s, *a)),
    ]


def test_null_handles_and_buffers_are_refused(lib):
    s, c = _containers(lib, ([1, 5, 9], [5, 9, 11]))
    buf = np.full(4, SENTINEL, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    try:
        assert lib.STORM_contig_pairw_similarity(None, JACCARD, 0, p, 2, 2) == -1
        assert lib.STORM_contig_pairw_similarity_device(None, JACCARD, 0, p, 2, 2) == -1
        assert lib.STORM_pairw_similarity(None, JACCARD, 0, p, 2, 2) == -1
        assert lib.STORM_pairw_similarity_device(None, JACCARD, 0, p, 2, 2) == -1
        for fn in (lib.STORM_square_similarity, lib.STORM_square_similarity_device):
            assert fn(None, s, JACCARD, 0, p, 2, 2) == -1
            assert fn(s, None, JACCARD, 0, p, 2, 2) == -1
        for name, call in _calls(lib, s, c):
            assert call(JACCARD, 0, None, 2, 2) == -2, name
        assert (buf == SENTINEL).all()
    finally:
        lib.STORM_free(s)
        lib.STORM_contig_free(c)


def test_short_buffers_give_minus_4_and_write_nothing(lib):
    s, c = _containers(lib, ([1, 5, 9], [5, 9, 11]))
    buf = np.full(4, SENTINEL, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    try:
        for name, call in _calls(lib, s, c):
            for measure in (JACCARD, LD_R2):
                assert call(measure, 64, p, 1, 2) == -4, name
                assert call(measure, 64, p, 2, 1) == -4, name
        assert (buf == SENTINEL).all()
    finally:
        lib.STORM_free(s)
        lib.STORM_contig_free(c)


def test_bad_measure_and_bad_n_bits_give_minus_3_with_a_reason(lib):
    s, c = _containers(lib, ([1, 5, 9], [5, 9, 11]))
    buf = np.full(4, SENTINEL, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    try:
        for name, call in _calls(lib, s, c):
            for measure, n_bits, word in ((4, 64, b"measure"), (-1, 64, b"measure"), (LD_D, (1 << 32) + 1, b"n_bits"),
                                          (LD_R2, 1 << 40, b"n_bits")):
                assert call(measure, n_bits, p, 2, 2) == -3, (name, measure, n_bits)
                reason = lib.STORM_hip_error()
                assert reason and word in reason and name.encode() in reason, (name, reason)
            if "contig" not in name:     # a STORM_t declares no universe; a STORM_contiguous_t's is its vector_length
                for measure in (LD_D, LD_R2):
                    assert call(measure, 0, p, 2, 2) == -3, (name, measure)
                    assert b"n_bits" in lib.STORM_hip_error()
        assert (buf == SENTINEL).all()
    finally:
        lib.STORM_free(s)
        lib.STORM_contig_free(c)


def test_empty_containers_return_0_and_write_nothing(lib):
    s, c = _containers(lib, ())
    full, _c = _containers(lib, ([1, 5, 9],))
    buf = np.full(4, SENTINEL, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    try:
        for name, call in _calls(lib, s, c):
            for measure, n_bits in ((JACCARD, 0), (COSINE, 0), (LD_D, 64), (LD_R2, 64)):
                assert call(measure, n_bits, p, 2, 2) == 0, (name, measure)
                assert call(measure, n_bits, p, 0, 0) == 0, (name, measure)
        for fn in (lib.STORM_square_similarity, lib.STORM_square_similarity_device):   # one empty side
            assert fn(s, full, JACCARD, 0, p, 2, 2) == 0
            assert fn(full, s, JACCARD, 0, p, 2, 2) == 0
        assert (buf == SENTINEL).all()
    finally:
        for h in (s, full):
            lib.STORM_free(h)
        for h in (c, _c):
            lib.STORM_contig_free(h)


def test_a_real_container_is_refused_without_a_device(lib):
    s, c = _containers(lib, ([1, 5, 9], [5, 9, 11]))
    buf = np.full(4, SENTINEL, dtype=np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    try:
        if _no_gpu(lib):
            for name, call in _calls(lib, s, c):
                for measure in (JACCARD, COSINE, LD_D, LD_R2):
                    assert call(measure, 64, p, 2, 2) == -3, (name, measure)
                    assert lib.STORM_hip_error(), name          # the reason is given
            assert (buf == SENTINEL).all()                      # and nothing was computed on the CPU
            ctx = C.c_void_p()
            assert lib.storm_hip_ctx_create(0, None, C.byref(ctx)) != 0
        else:                                                   # (host forms only: `buf` is host memory)
            for name, call in _calls(lib, s, c):
                if not name.endswith("_device"):
                    buf[:] = SENTINEL
                    assert call(JACCARD, 0, p, 2, 2) == 0, name
                    assert buf[1] == np.float32(0.5), (name, buf)   # |r0 & r1| = 2, |r0 | r1| = 4
        counts = np.ones(2, dtype=np.uint32).ctypes.data_as(C.c_void_p)
        assert lib.storm_hip_similarity_finish_device(None, p, 2, 2, 2, counts, counts, 0, JACCARD, 64) == -1   # STORM_HIP_EINVAL
    finally:
        lib.STORM_free(s)
        lib.STORM_contig_free(c)


def test_a_c_caller_of_storm_h_links_and_runs(lib, tmp_path):
    src = tmp_path / "similarity_caller.c"
    exe = tmp_path / "similarity_caller"
    src.write_text(C_CALLER)
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.run(["gcc", "-std=gnu11", "-Wall", "-Werror", "-I", INC, "-o", str(exe), str(src), "-L", libdir,
                    "-lstorm_hip", "-Wl,-rpath," + libdir], check=True, capture_output=True, text=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stdout, res.stderr[-2000:])
    first, reason = (res.stdout.splitlines() + [""])[:2]
    rc, value = first.split()
    if _no_gpu(lib):
        assert int(rc) == -3 and float(value) == -7.5 and reason, res.stdout
    else:
        assert int(rc) == 0 and float(value) == 0.5, res.stdout
