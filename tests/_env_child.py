"""One process's worth of storm.h calls for tests/test_gpu_env_switches.py — a helper module, not a test.

Everything the library reads from the environment (STORM_HIP_DEVICES, _SHARD, _OPTIONS, _VARIANT, _TIMING, ...) is read once
per process, so the switches are tested on children: the parent sets the variables, runs `python -m tests._env_child
[section ...]` and compares what comes back with references of its own. This module sets no environment variable.

    inputs()   the fixed seeded inputs, numpy only — the parent calls it too, and never loads the library
    main()     the battery: prints ONE JSON object (the last line of stdout) with every result, the STORM_hip_last_pass words
               after each call, every return code and every STORM_hip_error() text

Sections (all of them without arguments): contig, sparse_contig, mixed, lists, wrappers, dosage, ctx."""
import ctypes as C
import hashlib
import json
import sys

import numpy as np

ALL_PAIRS_FAILED = (1 << 64) - 1
SECTIONS = ("contig", "sparse_contig", "mixed", "lists", "wrappers", "dosage", "ctx")
OPS = ("and", "or", "xor")
CONTIG_BITS, CONTIG_ROWS, CONTIG_MORE = 4096, 1040, 30
VICTIM = 17                       # the row of the mixed STORM_t that is edited
DEV_PAD = 7                       # columns of the device window beyond the matrix
SENTINEL = 0xA5A5A5A5


def _choice_rows(rng, n_rows, universe, count):
    return [np.sort(rng.choice(universe, size=count, replace=False)).astype(np.uint32) for _ in range(n_rows)]


def _block_rows(rng, counts):
    """rows of a STORM_t from per-block position counts [n_rows][n_blocks] (0: no block)"""
    rows = []
    for per_block in counts:
        parts = [b * 65536 + np.sort(rng.choice(65536, size=c, replace=False)) for b, c in enumerate(per_block) if c]
        rows.append(np.concatenate(parts).astype(np.uint32))
    return rows


def inputs():
    """the same arrays in the parent and in every child"""
    rng = np.random.default_rng(20261021)
    x = {}
    # 1040 + 30 rows of 4096 bits, 600 set: denser than a sparse row (<= 4096 / 16), so the dense mirror answers
    x["contig"] = _choice_rows(rng, CONTIG_ROWS + CONTIG_MORE, CONTIG_BITS, 600)
    # every row sparse: the container's list mirror (a private STORM_t, the list-probe kernel) answers
    x["sparse_contig"] = _choice_rows(rng, 300, CONTIG_BITS, 40)
    # 130 rows over 3 block columns of 65536: lists (< 4096 positions) and bitmaps (>= 4096) mixed, some blocks absent
    counts = [[(5000 if (3 * i + b) % 5 == 0 else 0 if (i + 2 * b) % 7 == 0 else int(rng.integers(20, 300))) for b in range(3)]
              for i in range(130)]
    counts[VICTIM] = [250, 5000, 60]
    x["mixed"] = _block_rows(rng, counts)
    # the victim with the same block ids and the same count per block at other positions (every block header stays)
    edited = []
    for b, c in enumerate(counts[VICTIM]):
        old = x["mixed"][VICTIM]
        free = np.setdiff1d(np.arange(65536, dtype=np.uint32), old[old // 65536 == b] % 65536)
        edited.append(b * 65536 + np.sort(rng.choice(free, size=c, replace=False)))
    x["mixed_edited_row"] = np.concatenate(edited).astype(np.uint32)
    # lists only: 200 rows of 100 positions in 2 x 65536 bits (0.08 % dense: the per-pair matrix comes from the lists, K5)
    x["lists"] = _choice_rows(rng, 200, 2 * 65536, 100)
    x["diag"] = rng.integers(0, 1 << 64, size=(300, 16), dtype=np.uint64) & rng.integers(0, 1 << 64, size=(300, 16), dtype=np.uint64)
    x["square_a"] = rng.integers(0, 1 << 64, size=(130, 16), dtype=np.uint64) & rng.integers(0, 1 << 64, size=(130, 16), dtype=np.uint64)
    x["square_b"] = rng.integers(0, 1 << 64, size=(70, 16), dtype=np.uint64)
    g = rng.integers(0, 3, size=(129, 257), dtype=np.uint8)
    g[rng.random(g.shape) < 0.10] = 3                       # 10 % missing
    x["dosage"] = g
    return x


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------ the battery
class _Battery:
    def __init__(self):
        import stormbitmaps_amd as sb
        self.sb = sb
        self.lib = sb.load()
        for name in ("STORM_bitmap_cont_add",):
            getattr(self.lib, name).argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
            getattr(self.lib, name).restype = C.c_int
        self.lib.STORM_bitmap_cont_clear.argtypes = [C.c_void_p]
        self.lib.STORM_bitmap_cont_clear.restype = C.c_int
        self.x = inputs()
        self.out = {}

    def last_pass(self):
        words = (C.c_uint64 * 4)()
        assert self.lib.STORM_hip_last_pass(words) == 0
        return [int(w) for w in words]

    def error(self):
        msg = self.lib.STORM_hip_error()
        return msg.decode(errors="replace") if msg else ""

    def total(self, value):
        value = int(value)
        return {"value": value, "pass": self.last_pass(), "error": self.error() if value == ALL_PAIRS_FAILED else None}

    def matrix(self, rc, arr):
        rc = int(rc)
        return {"rc": rc, "pass": self.last_pass(), "error": self.error() if rc else None, "shape": list(arr.shape),
                "sha": sha(arr), "sum": int(arr.sum(dtype=np.uint64))}

    # ---- sections
    def contig(self):
        lib, rows = self.lib, self.x["contig"]
        c = self.sb.StormContig(CONTIG_BITS)
        for r in rows[:CONTIG_ROWS]:
            assert c.add(r) == r.size
        o = {"totals": [self.total(lib.STORM_contig_pairw_intersect_cardinality(c._h)) for _ in range(3)]}
        if "total_only" not in sys.argv:
            for r in rows[CONTIG_ROWS:]:
                assert c.add(r) == r.size
            o["after_add"] = self.total(lib.STORM_contig_pairw_intersect_cardinality(c._h))
            n = c.n_rows
            m = np.zeros((n, n), dtype=np.uint32)
            o["matrix"] = self.matrix(lib.STORM_contig_pairw_matrix(c._h, 0, m.ctypes.data_as(C.c_void_p), n, n), m)
        c.free()
        self.out["contig"] = o

    def sparse_contig(self):
        c = self.sb.StormContig(CONTIG_BITS)
        for r in self.x["sparse_contig"]:
            assert c.add(r) == r.size
        self.out["sparse_contig"] = {"totals": [self.total(self.lib.STORM_contig_pairw_intersect_cardinality(c._h)) for _ in range(2)]}
        c.free()

    def _storm(self, rows):
        s = self.sb.Storm()
        for r in rows:
            assert s.add(r) == 1
        return s

    def mixed(self):
        lib = self.lib
        s = self._storm(self.x["mixed"])
        o = {"totals": [self.total(lib.STORM_pairw_intersect_cardinality(s._h)) for _ in range(2)]}
        # conts[VICTIM] (sizeof(STORM_bitmap_cont_t) = 32, tests/test_abi.py): cleared and filled again through the public
        # row functions, which leaves every block header as it was
        row = C.cast(s._h, C.POINTER(C.c_void_p))[0] + VICTIM * 32
        new = self.x["mixed_edited_row"]
        o["edit_rcs"] = [int(lib.STORM_bitmap_cont_clear(C.c_void_p(row))),
                         int(lib.STORM_bitmap_cont_add(C.c_void_p(row), new.ctypes.data_as(C.c_void_p), new.size))]
        o["after_edit"] = self.total(lib.STORM_pairw_intersect_cardinality(s._h))
        n = s.n_rows
        m = np.zeros((n, n), dtype=np.uint32)
        o["matrix"] = self.matrix(lib.STORM_pairw_matrix(s._h, 0, m.ctypes.data_as(C.c_void_p), n, n), m)
        buf = s.serialize()
        o["serialized_bytes"] = int(buf.size)
        o["serialized"] = self.total(lib.STORM_serialized_pairw_intersect_cardinality(buf.ctypes.data_as(C.c_void_p), buf.size))
        s.free()
        self.out["mixed"] = o

    def lists(self):
        lib, rows = self.lib, self.x["lists"]
        s = self._storm(rows)
        n = s.n_rows
        o = {"total": self.total(lib.STORM_pairw_intersect_cardinality(s._h))}
        for k, op in enumerate(OPS):
            m = np.zeros((n, n), dtype=np.uint32)
            o["matrix_" + op] = self.matrix(lib.STORM_pairw_matrix(s._h, k, m.ctypes.data_as(C.c_void_p), n, n), m)
        # the device form, into a window with a pitch and a sentinel: device memory borrowed from a matrix of the device
        # library on a context of this section's own
        ctx = self.sb.HipContext(0)
        words = (n + DEV_PAD + 1) // 2
        win = ctx.matrix(n, words)
        win.upload(np.full((n, words), SENTINEL | SENTINEL << 32, dtype=np.uint64))
        ctx.synchronize()
        rc = lib.STORM_pairw_matrix_device(s._h, 0, C.c_void_p(win.device_ptr), n, 2 * win.stride_words)
        got = win.download().view(np.uint32)
        o["matrix_device"] = self.matrix(rc, got)
        win.close()
        ctx.close()
        # the rectangle of two containers: one device slot and one process, or refused
        a, b = self._storm(rows[:100]), self._storm(rows[100:])
        o["square_total"] = self.total(lib.STORM_intersect_cardinality_square(a._h, b._h))
        m = np.full((100, 100), 9, dtype=np.uint32)
        o["square_matrix"] = self.matrix(lib.STORM_square_matrix(a._h, b._h, 0, m.ctypes.data_as(C.c_void_p), 100, 100), m)
        for h in (a, b, s):
            h.free()
        self.out["lists"] = o

    def wrappers(self):
        lib, x = self.lib, self.x
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        d, a, b = x["diag"], x["square_a"], x["square_b"]
        self.out["wrappers"] = {
            "diag": [self.total(lib.STORM_wrapper_diag(d.shape[0], p(d), d.shape[1], None)) for _ in range(2)],
            "square": self.total(lib.STORM_wrapper_square(a.shape[0], p(a), b.shape[0], p(b), a.shape[1], None))}

    def dosage(self):
        g = self.x["dosage"]
        d = self.sb.StormDosage(g.shape[1])
        for row in g:
            d.add(row)
        n = d.n_rows
        m = np.zeros((n, n), dtype=np.float32)
        rc = int(self.lib.STORM_dosage_pairw_corr_complete(d._h, 0, m.ctypes.data_as(C.c_void_p), n, n))
        self.out["dosage"] = {"rc": rc, "pass": self.last_pass(), "error": self.error() if rc else None,
                              "r2_bits": m.view(np.uint32).ravel().tolist()}
        d.free()

    def ctx(self):
        """what a context of the device library itself took from STORM_HIP_VARIANT / _SEG_ROWS / _CHUNKS_PER_ITEM, and one
        small popcount-eligible pass on it"""
        ctx = self.sb.HipContext(0)
        o = {k: ctx.get_option(k) for k in ("variant", "seg_rows", "chunks_per_item")}
        m = ctx.matrix_from_host(self.x["diag"])
        o["total"] = m.pairw()
        o["variant_used"] = ctx.get_option("variant_used")
        o["launch"] = {k: int(v) for k, v in ctx.last_launch_info().items()}
        m.close()
        ctx.close()
        o["device_count"] = int(self.lib.storm_hip_device_count())
        self.out["ctx"] = o


def main(argv):
    wanted = [a for a in argv if a in SECTIONS] or list(SECTIONS)
    b = _Battery()
    for name in SECTIONS:
        if name in wanted:
            getattr(b, name)()
    b.lib.STORM_hip_shutdown()
    sys.stdout.flush()
    print(json.dumps(b.out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
