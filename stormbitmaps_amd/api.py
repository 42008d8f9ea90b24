"""Python mirror of the storm.h interface (same names, argument meaning and error behaviour as
the reference's C API) plus thin handles over the device-level C-ABI of include/storm_hip.h.

Everything here calls into libstorm_hip.so; no arithmetic happens in Python.
Reference lines cited are /root/reference/storm.h and storm.c of mklarqvist/StormBitmaps.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import StormHipError, check

ALL_PAIRS_FAILED = (1 << 64) - 1  # (uint64_t)-1, storm.c:878,898,1150,1176


def _u32(values) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(values, dtype=np.uint32))


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


MEASURES = {"jaccard": 0, "cosine": 1, "ld_d": 2, "ld_r2": 3}  # STORM_SIM_* (storm.h)


def _similarity(lib, what: str, rc: int) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} -> {rc}: {lib.STORM_hip_error().decode()}")


OPS = {"and": 0, "or": 1, "xor": 2}


class _LagForms:
    """The lag-layout calls of a storm.h container (extension; `_LAG` = the C prefix, STORM_contig_ or STORM_): the pairs
    within max_lag rows of each other, pair (i, j) at [i, j - i - 1] of an [n_rows, L] matrix, L = min(max_lag, n_rows - 1)."""

    def _lag_width(self, max_lag: int) -> int:
        return min(max_lag, max(self.n_rows - 1, 0))

    def pairw_lag_matrix(self, max_lag: int, op: str = "and") -> np.ndarray:
        """[n_rows, L] uint32: entry (i, d) = popcount(row_i OP row_{i+1+d}); 0 where i + 1 + d >= n_rows."""
        n, w = self.n_rows, self._lag_width(max_lag)
        out = np.zeros((n, w), dtype=np.uint32)
        name = self._LAG + "pairw_lag_matrix"
        _similarity(self._lib, name, int(getattr(self._lib, name)(self._h, OPS[op], max_lag,
                                                                  _ptr(out) if out.size else _ptr(np.zeros(1, np.uint32)), n, w)))
        return out

    def pairw_lag_matrix_device(self, d_out: int, out_rows: int, out_ld: int, max_lag: int, op: str = "and") -> None:
        """The same left in device memory at address d_out (out_rows x out_ld uint32; nothing outside the layout is written)."""
        name = self._LAG + "pairw_lag_matrix_device"
        _similarity(self._lib, name, int(getattr(self._lib, name)(self._h, OPS[op], max_lag, C.c_void_p(d_out), out_rows, out_ld)))

    def pairw_lag_similarity(self, max_lag: int, measure: str = "jaccard", n_bits: int = 0) -> np.ndarray:
        """[n_rows, L] float32: entry (i, d) = the measure of rows i and i + 1 + d (as pairw_similarity); 0 in the corner."""
        n, w = self.n_rows, self._lag_width(max_lag)
        out = np.zeros((n, w), dtype=np.float32)
        name = self._LAG + "pairw_lag_similarity"
        _similarity(self._lib, name, int(getattr(self._lib, name)(self._h, MEASURES[measure], n_bits, max_lag,
                                                                  _ptr(out) if out.size else _ptr(np.zeros(1, np.float32)), n, w)))
        return out

    def pairw_lag_similarity_device(self, d_out: int, out_rows: int, out_ld: int, max_lag: int, measure: str = "jaccard",
                                    n_bits: int = 0) -> None:
        """The same left in device memory at address d_out (out_rows x out_ld float32)."""
        name = self._LAG + "pairw_lag_similarity_device"
        _similarity(self._lib, name, int(getattr(self._lib, name)(self._h, MEASURES[measure], n_bits, max_lag, C.c_void_p(d_out),
                                                                  out_rows, out_ld)))


SCORES = dict(MEASURES, count=4)  # what the top-k calls rank by: a measure, or STORM_TOPK_COUNT (the AND count itself)


def _topk_out(n: int, k: int, score: str):
    """(idx, val) of n rows: val float32 for a measure, uint32 for the count (at least one entry, so that both have an address)"""
    return (np.zeros((n, k), dtype=np.uint32), np.zeros((n, k), dtype=np.uint32 if score == "count" else np.float32))


class _TopkForms:
    """The top-k calls of a storm.h container (extension; `_LAG` = the C prefix): for each row its k most similar rows,
    selected on the device. idx[i, t] is the row that ranks t-th for row i (value descending, then row index ascending),
    val[i, t] its value; fewer than k candidates: idx 0xFFFFFFFF with val NaN (0 under score "count")."""

    def pairw_topk(self, k: int, score: str = "jaccard", n_bits: int = 0, panel_rows: int = 0):
        """(idx [n_rows, k] uint32, val [n_rows, k] float32, or uint32 for score "count"): row i against every other row."""
        n = self.n_rows
        idx, val = _topk_out(n, k, score)
        name = self._LAG + "pairw_topk"
        spare = np.zeros(1, np.uint32)
        _similarity(self._lib, name, int(getattr(self._lib, name)(self._h, SCORES[score], n_bits, k, panel_rows,
                                                                  _ptr(idx) if idx.size else _ptr(spare),
                                                                  _ptr(val) if val.size else _ptr(spare), n, k)))
        return idx, val

    def pairw_topk_device(self, d_idx: int, d_val: int, out_rows: int, out_ld: int, k: int, score: str = "jaccard",
                          n_bits: int = 0, panel_rows: int = 0) -> None:
        """The same left in device memory at addresses d_idx / d_val (out_rows x out_ld 32-bit words each; columns [k, out_ld)
        are not touched)."""
        name = self._LAG + "pairw_topk_device"
        _similarity(self._lib, name, int(getattr(self._lib, name)(self._h, SCORES[score], n_bits, k, panel_rows, C.c_void_p(d_idx),
                                                                  C.c_void_p(d_val), out_rows, out_ld)))


def _all_pairs(value: int, what: str) -> int:
    if value == ALL_PAIRS_FAILED:
        lib = _lib.load()
        msg = lib.STORM_hip_error()
        raise StormHipError(f"{what}: device path failed: {msg.decode() if msg else '?'}")
    return int(value)


# ------------------------------------------------------------------------------------------
# storm.h containers
# ------------------------------------------------------------------------------------------
class StormContig(_LagForms, _TopkForms):
    """STORM_contiguous_t (storm.h:188-200, :235-242): dense row-major bitmap matrix."""
    _LAG = "STORM_contig_"

    def __init__(self, vector_length: int):
        self._lib = _lib.load()
        self._h = self._lib.STORM_contig_new(vector_length)  # storm.c:1001
        if not self._h:
            raise MemoryError("STORM_contig_new")
        self.vector_length = vector_length

    def add(self, values) -> int:
        """STORM_contig_add (storm.c:1031): sorted positions of one row; returns n_values,
        0 for an empty row (no row appended)."""
        v = _u32(values)
        return int(self._lib.STORM_contig_add(self._h, _ptr(v) if v.size else _ptr(np.zeros(1, np.uint32)),
                                              v.size))

    def add_synthetic(self, n_rows: int, draws: int, seed: int = 42, row0: int = 0) -> int:
        """Rows of the deterministic benchmark matrix (include/storm_synth.h), added in C."""
        return int(self._lib.storm_synth_fill_contig(self._h, self.vector_length, row0, n_rows,
                                                     draws, seed))

    def clear(self) -> int:
        return int(self._lib.STORM_contig_clear(self._h))  # storm.c:1139

    def pairw_intersect_cardinality(self) -> int:
        return _all_pairs(self._lib.STORM_contig_pairw_intersect_cardinality(self._h),
                          "STORM_contig_pairw_intersect_cardinality")  # storm.c:1149

    def pairw_intersect_cardinality_blocked(self, bsize: int = 0) -> int:
        return _all_pairs(
            self._lib.STORM_contig_pairw_intersect_cardinality_blocked(self._h, bsize),
            "STORM_contig_pairw_intersect_cardinality_blocked")  # storm.c:1175

    @property
    def n_rows(self) -> int:
        """Rows the handle holds (STORM_contig_n_rows; an empty add appends none, storm.c:1034)."""
        return int(self._lib.STORM_contig_n_rows(self._h))

    def pairw_matrix(self, op: str = "and") -> np.ndarray:
        """STORM_contig_pairw_matrix (extension): [n_rows, n_rows] uint32 per-pair counts, i < j.
        The buffer is sized from the handle's own row count and its extent is passed down, so a
        miscount cannot overrun it (the C entry point returns -4 instead)."""
        n = self.n_rows
        out = np.zeros((n, n), dtype=np.uint32)
        rc = int(self._lib.STORM_contig_pairw_matrix(self._h, {"and": 0, "or": 1, "xor": 2}[op],
                                                     _ptr(out), n, n))
        if rc != 0:
            raise RuntimeError(f"STORM_contig_pairw_matrix -> {rc}: "
                               f"{self._lib.STORM_hip_error().decode()}")
        return out

    def pairw_matrix_device(self, d_out: int, out_rows: int, out_ld: int, op: str = "and") -> None:
        """STORM_contig_pairw_matrix_device (extension): the same triangle left in device memory at address d_out."""
        rc = int(self._lib.STORM_contig_pairw_matrix_device(self._h, {"and": 0, "or": 1, "xor": 2}[op], C.c_void_p(d_out),
                                                            out_rows, out_ld))
        if rc != 0:
            raise RuntimeError(f"STORM_contig_pairw_matrix_device -> {rc}: {self._lib.STORM_hip_error().decode()}")

    def pairw_similarity(self, measure: str = "jaccard", n_bits: int = 0) -> np.ndarray:
        """STORM_contig_pairw_similarity (extension): [n_rows, n_rows] float32, entry (i, j), i < j = the measure ("jaccard",
        "cosine", "ld_d", "ld_r2") of rows i and j, finished on the device; 0 for i >= j. n_bits: the universe size of the
        LD measures, 0 = vector_length."""
        n = self.n_rows
        out = np.zeros((n, n), dtype=np.float32)
        _similarity(self._lib, "STORM_contig_pairw_similarity",
                    int(self._lib.STORM_contig_pairw_similarity(self._h, MEASURES[measure], n_bits,
                                                                _ptr(out) if out.size else _ptr(np.zeros(1, np.float32)), n, n)))
        return out

    def pairw_similarity_device(self, d_out: int, out_rows: int, out_ld: int, measure: str = "jaccard", n_bits: int = 0) -> None:
        """STORM_contig_pairw_similarity_device (extension): the same triangle left in device memory at address d_out
        (out_rows x out_ld float32; entries i >= j are not converted)."""
        _similarity(self._lib, "STORM_contig_pairw_similarity_device",
                    int(self._lib.STORM_contig_pairw_similarity_device(self._h, MEASURES[measure], n_bits, C.c_void_p(d_out),
                                                                       out_rows, out_ld)))

    def hip_invalidate(self) -> None:
        """STORM_contig_hip_invalidate: forget the device copy after an in-place edit of the
        handle's public buffers (storm.h extension)."""
        self._lib.STORM_contig_hip_invalidate(self._h)

    def pairw_intersect_cardinality_list(self) -> int:
        return int(self._lib.STORM_contig_pairw_intersect_cardinality_list(self._h))  # :1243

    def pairw_intersect_cardinality_blocked_list(self, bsize: int = 0) -> int:
        return int(self._lib.STORM_contig_pairw_intersect_cardinality_blocked_list(self._h,
                                                                                  bsize))  # :1265

    def free(self) -> None:
        if self._h:
            self._lib.STORM_contig_free(self._h)  # storm.c:1020
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


DOSAGE_MEASURES = {"r2": 0, "r": 1}  # STORM_DOSAGE_* (storm.h)
DOSAGE_SCORES = dict(DOSAGE_MEASURES, dot=2)  # what the dosage top-k calls rank by: a measure, or STORM_DOSAGE_TOPK_DOT
LDSCORE_STATS = {"r2": 0, "r2_adj": 1}  # STORM_LDSCORE_* (storm.h)


def _device_window(device, n: int):
    """(address, rows, leading dimension) of a 2-D torch tensor of 4-byte entries in device memory that receives an n x n
    result (rows contiguous; the leading dimension is the tensor's row stride)"""
    if device.dim() != 2 or device.element_size() != 4 or device.stride(1) != 1 or not device.is_cuda:
        raise ValueError("device=: a 2-D tensor of 32-bit entries in device memory with contiguous rows")
    if device.shape[0] < n or device.shape[1] < n:
        raise ValueError(f"device=: a tensor of {tuple(device.shape)} cannot hold {n} x {n} entries")
    return C.c_void_p(device.data_ptr()), int(device.shape[0]), int(device.stride(0))


def _device_vector(t, message: str, entry_bytes: int = 4) -> None:
    """ValueError(message) unless t is None or a 1-D contiguous torch tensor of entry_bytes-byte entries in device memory"""
    if t is not None and (t.dim() != 1 or t.element_size() != entry_bytes or t.stride(0) != 1 or not t.is_cuda):
        raise ValueError(message)


def _window_args(n: int, max_lag: Optional[int], pos, max_dist: Optional[float]):
    """(max_lag, pos, max_dist) of a windowed band call as the C call takes them: max_lag None is 0 ("what the windows
    need"), pos is n float64 coordinates or NULL, and comes with max_dist"""
    p = None
    if pos is not None:
        p = np.ascontiguousarray(pos, dtype=np.float64)
        if p.shape != (n,):
            raise ValueError("pos: one coordinate per row")
        if max_dist is None:
            raise ValueError("pos needs max_dist")
    p_ptr = None if p is None else _ptr(p if p.size else np.zeros(1))   # (no rows: still "positions given")
    return 0 if max_lag is None else int(max_lag), p_ptr, 0.0 if max_dist is None else float(max_dist)


class StormDosage:
    """STORM_dosage_t (storm.h, extension): rows of n_samples 2-bit dosages (0 / 1 / 2 copies of an allele per sample; 3 is an
    ordinary value), their per-pair dot products and genotype correlations (PLINK --r / --r2) on the device. In
    row_missing, pairw_nobs, pairw_corr_complete, their lag forms, square_nobs and square_corr(complete=True) — and only there —
    the value 3 means "missing"."""

    def __init__(self, n_samples: int):
        self._lib = _lib.load()
        self._h = self._lib.STORM_dosage_new(n_samples) if 0 <= n_samples < (1 << 64) else None
        if not self._h:
            raise ValueError(f"STORM_dosage_new({n_samples}): 1 .. 2^24 samples")
        self.n_samples = n_samples
        self.n_words = (n_samples + 31) // 32

    def _check(self, what: str, rc: int) -> None:
        if rc != 0:
            raise RuntimeError(f"{what} -> {rc}: {self._lib.STORM_hip_error().decode()}")

    def add(self, values) -> None:
        """STORM_dosage_add: one row, one value 0 .. 3 per sample."""
        v = np.ascontiguousarray(np.asarray(values, dtype=np.uint8))
        self._check("STORM_dosage_add", int(self._lib.STORM_dosage_add(self._h, _ptr(v) if v.size else _ptr(np.zeros(1, np.uint8)),
                                                                       v.size)))

    def add_packed(self, words) -> None:
        """STORM_dosage_add_packed: rows already packed, [n_rows, n_words] uint64 (32 values per word, tail bits zero)."""
        w = np.ascontiguousarray(np.asarray(words, dtype=np.uint64))
        if w.ndim == 1:
            w = w.reshape(1, -1)
        if w.ndim != 2 or w.shape[1] != self.n_words:
            raise ValueError(f"add_packed: rows of {self.n_words} words expected, got an array of {w.shape}")
        self._check("STORM_dosage_add_packed", int(self._lib.STORM_dosage_add_packed(self._h, _ptr(w), w.shape[0])))

    def clear(self) -> None:
        self._check("STORM_dosage_clear", int(self._lib.STORM_dosage_clear(self._h)))

    @property
    def n_rows(self) -> int:
        return int(self._lib.STORM_dosage_n_rows(self._h))

    def row_sums(self):
        """(sum v, sum v^2) of every row, [n_rows] uint32 each, computed on the device."""
        n = self.n_rows
        s, q = np.zeros(max(n, 1), dtype=np.uint32), np.zeros(max(n, 1), dtype=np.uint32)
        self._check("STORM_dosage_row_sums", int(self._lib.STORM_dosage_row_sums(self._h, _ptr(s), _ptr(q))))
        return s[:n], q[:n]

    def pairw_dot(self, device=None):
        """STORM_dosage_pairw_dot: [n_rows, n_rows] uint32, entry (i, j), i < j = sum_s v_i[s] v_j[s]; 0 for i >= j.
        device=: a 2-D torch tensor of 32-bit entries in device memory that receives the triangle instead
        (STORM_dosage_pairw_dot_device: entries i >= j stay as they were); returns None then."""
        n = self.n_rows
        if device is not None:
            ptr, rows, ld = _device_window(device, n)
            self._check("STORM_dosage_pairw_dot_device", int(self._lib.STORM_dosage_pairw_dot_device(self._h, ptr, rows, ld)))
            return None
        out = np.zeros((n, n), dtype=np.uint32)
        self._check("STORM_dosage_pairw_dot",
                    int(self._lib.STORM_dosage_pairw_dot(self._h, _ptr(out) if out.size else _ptr(np.zeros(1, np.uint32)), n, n)))
        return out

    def pairw_corr(self, measure: str = "r2", device=None):
        """STORM_dosage_pairw_corr: [n_rows, n_rows] float32, entry (i, j), i < j = the Pearson correlation ("r") of the two
        dosage vectors or its square ("r2"), finished on the device; NaN against a constant row; 0 for i >= j.
        device=: as pairw_dot (STORM_dosage_pairw_corr_device)."""
        n = self.n_rows
        if device is not None:
            ptr, rows, ld = _device_window(device, n)
            self._check("STORM_dosage_pairw_corr_device",
                        int(self._lib.STORM_dosage_pairw_corr_device(self._h, DOSAGE_MEASURES[measure], ptr, rows, ld)))
            return None
        out = np.zeros((n, n), dtype=np.float32)
        self._check("STORM_dosage_pairw_corr",
                    int(self._lib.STORM_dosage_pairw_corr(self._h, DOSAGE_MEASURES[measure],
                                                          _ptr(out) if out.size else _ptr(np.zeros(1, np.float32)), n, n)))
        return out

    def square_dot(self, other: "StormDosage", device=None):
        """STORM_dosage_square_dot: [n_rows, other.n_rows] uint32, entry (i, j) = sum_s v_i[s] w_j[s] for every row of this
        container against every row of `other` (the same number of samples; 3 is an ordinary value).
        device=: a 2-D torch tensor of 32-bit entries in device memory that receives the rectangle instead
        (STORM_dosage_square_dot_device); returns None then."""
        return self._square("STORM_dosage_square_dot", np.uint32, other, device)

    def _square(self, name: str, dtype, other: "StormDosage", device, *args):
        """one statistic of the rectangle with `other` (args: what the C call takes between the handles and the output)"""
        na, nb = self.n_rows, other.n_rows
        if device is not None:
            if device.dim() != 2 or device.element_size() != 4 or device.stride(1) != 1 or not device.is_cuda:
                raise ValueError("device=: a 2-D tensor of 32-bit entries in device memory with contiguous rows")
            if device.shape[0] < na or device.shape[1] < nb:
                raise ValueError(f"device=: a tensor of {tuple(device.shape)} cannot hold {na} x {nb} entries")
            self._check(name + "_device", int(getattr(self._lib, name + "_device")(self._h, other._h, *args, C.c_void_p(device.data_ptr()),
                                                                                   int(device.shape[0]), int(device.stride(0)))))
            return None
        out = np.zeros((na, nb), dtype=dtype)
        self._check(name, int(getattr(self._lib, name)(self._h, other._h, *args, _ptr(out) if out.size else _ptr(np.zeros(1, dtype)),
                                                       na, nb)))
        return out

    def square_corr(self, other: "StormDosage", measure: str = "r2", complete: bool = False, device=None):
        """STORM_dosage_square_corr[_complete]: [n_rows, other.n_rows] float32, entry (i, j) = the Pearson correlation ("r") or
        its square ("r2") of row i of this container and row j of `other` (the same number of samples) — a list of index
        variants against a panel — with pairw_corr's bits for the two rows; NaN against a constant row. complete=True: over the
        samples both rows have (value 3 = missing), pairw_corr_complete's bits. device=: as square_dot
        (STORM_dosage_square_corr[_complete]_device); every entry of the rectangle is written in both forms."""
        return self._square("STORM_dosage_square_corr_complete" if complete else "STORM_dosage_square_corr", np.float32, other, device,
                            DOSAGE_MEASURES[measure])

    def square_nobs(self, other: "StormDosage", device=None):
        """STORM_dosage_square_nobs: [n_rows, other.n_rows] uint32, entry (i, j) = the samples that neither row i of this
        container nor row j of `other` is missing (value 3) at. device=: as square_dot (STORM_dosage_square_nobs_device)."""
        return self._square("STORM_dosage_square_nobs", np.uint32, other, device)

    def _topk(self, name: str, handles, n: int, k: int, score: str, complete: bool, panel_rows: int, device):
        """one of the STORM_dosage_*_topk calls: (idx, val) of [n, k] as numpy arrays, or with device= (a torch device) as
        torch tensors there — idx int32 (the padding 0xFFFFFFFF reads -1), val float32, or int32 for score "dot" """
        name += "_complete" if complete else ""
        if device is not None:
            import torch
            idx = torch.empty((max(n, 1), k), dtype=torch.int32, device=device)
            val = torch.empty((max(n, 1), k), dtype=torch.int32 if score == "dot" else torch.float32, device=device)
            if not idx.is_cuda:
                raise ValueError("device=: a torch device with device memory")
            torch.cuda.synchronize(idx.device)   # (the allocator's stream is not the library's)
            self._check(name + "_device", int(getattr(self._lib, name + "_device")(
                *handles, DOSAGE_SCORES[score], k, panel_rows, C.c_void_p(idx.data_ptr()), C.c_void_p(val.data_ptr()), n, k)))
            return idx[:n], val[:n]
        idx = np.zeros((n, k), dtype=np.uint32)
        val = np.zeros((n, k), dtype=np.uint32 if score == "dot" else np.float32)
        spare = np.zeros(1, np.uint32)
        self._check(name, int(getattr(self._lib, name)(*handles, DOSAGE_SCORES[score], k, panel_rows,
                                                       _ptr(idx) if idx.size else _ptr(spare),
                                                       _ptr(val) if val.size else _ptr(spare), n, k)))
        return idx, val

    def pairw_topk(self, k: int, score: str = "r2", complete: bool = False, panel_rows: int = 0, device=None):
        """STORM_dosage_pairw_topk[_complete]: (idx [n_rows, k] uint32, val [n_rows, k] float32, or uint32 for score "dot"):
        for each row its k best OTHER rows by "r2", "r" (the signed value; rank by |r| with "r2") or "dot" (the dot product;
        not with complete=True), selected on the device: value descending, then row index ascending, pairw_corr's bits;
        fewer than k candidates (NaN entries are none): idx 0xFFFFFFFF with val NaN (0 for "dot"). complete=True: over the
        samples both rows have (value 3 = missing), pairw_corr_complete's bits. panel_rows: rows whose sums are on the
        device at a time (0: chosen by the library; else a multiple of 256). device=: a torch device; both results stay
        there as torch tensors (idx int32: the padding reads -1; val float32, or int32 for "dot")."""
        return self._topk("STORM_dosage_pairw_topk", (self._h,), self.n_rows, k, score, complete, panel_rows, device)

    def square_topk(self, other: "StormDosage", k: int, score: str = "r2", complete: bool = False, panel_rows: int = 0, device=None):
        """STORM_dosage_square_topk[_complete]: (idx, val) of [n_rows, k]: for each row of this container its k best rows of
        `other` (the same number of samples; other may be self, and a row lists itself then), square_corr's bits. Everything
        else as pairw_topk."""
        return self._topk("STORM_dosage_square_topk", (self._h, other._h), self.n_rows, k, score, complete, panel_rows, device)

    def row_missing(self):
        """STORM_dosage_row_missing: the samples of every row that are missing (value 3), [n_rows] uint32, counted on the
        device."""
        n = self.n_rows
        miss = np.zeros(max(n, 1), dtype=np.uint32)
        self._check("STORM_dosage_row_missing", int(self._lib.STORM_dosage_row_missing(self._h, _ptr(miss))))
        return miss[:n]

    def pairw_nobs(self, device=None):
        """STORM_dosage_pairw_nobs: [n_rows, n_rows] uint32, entry (i, j), i < j = the samples neither row is missing
        (value 3) at; 0 for i >= j. device=: as pairw_dot (STORM_dosage_pairw_nobs_device)."""
        n = self.n_rows
        if device is not None:
            ptr, rows, ld = _device_window(device, n)
            self._check("STORM_dosage_pairw_nobs_device", int(self._lib.STORM_dosage_pairw_nobs_device(self._h, ptr, rows, ld)))
            return None
        out = np.zeros((n, n), dtype=np.uint32)
        self._check("STORM_dosage_pairw_nobs",
                    int(self._lib.STORM_dosage_pairw_nobs(self._h, _ptr(out) if out.size else _ptr(np.zeros(1, np.uint32)), n, n)))
        return out

    def pairw_corr_complete(self, measure: str = "r2", device=None):
        """STORM_dosage_pairw_corr_complete: pairw_corr over the samples BOTH rows of a pair have (value 3 = missing): [n_rows,
        n_rows] float32; NaN where the pair shares fewer than two samples or a row is constant on the shared ones; 0 for
        i >= j. Rows without a 3 give pairw_corr's bits. device=: as pairw_dot (STORM_dosage_pairw_corr_complete_device)."""
        n = self.n_rows
        if device is not None:
            ptr, rows, ld = _device_window(device, n)
            self._check("STORM_dosage_pairw_corr_complete_device",
                        int(self._lib.STORM_dosage_pairw_corr_complete_device(self._h, DOSAGE_MEASURES[measure], ptr, rows, ld)))
            return None
        out = np.zeros((n, n), dtype=np.float32)
        self._check("STORM_dosage_pairw_corr_complete",
                    int(self._lib.STORM_dosage_pairw_corr_complete(self._h, DOSAGE_MEASURES[measure],
                                                                   _ptr(out) if out.size else _ptr(np.zeros(1, np.float32)), n, n)))
        return out

    # ---- the pairs within max_lag rows of each other: pair (i, j) at [i, j - i - 1] of an [n_rows, L] matrix ----
    def _pairw_lag(self, name: str, dtype, max_lag: int, device, *args):
        n, w = self.n_rows, min(max_lag, max(self.n_rows - 1, 0))
        if device is not None:
            if device.dim() != 2 or device.element_size() != 4 or device.stride(1) != 1 or not device.is_cuda:
                raise ValueError("device=: a 2-D tensor of 32-bit entries in device memory with contiguous rows")
            self._check(name + "_device", int(getattr(self._lib, name + "_device")(self._h, *args, max_lag, C.c_void_p(device.data_ptr()),
                                                                                   int(device.shape[0]), int(device.stride(0)))))
            return None
        out = np.zeros((n, w), dtype=dtype)
        self._check(name, int(getattr(self._lib, name)(self._h, *args, max_lag, _ptr(out) if out.size else _ptr(np.zeros(1, dtype)),
                                                       n, w)))
        return out

    def pairw_lag_dot(self, max_lag: int, device=None):
        """STORM_dosage_pairw_lag_dot: [n_rows, L] uint32, L = min(max_lag, n_rows - 1): entry (i, d) = the dot product of rows i
        and i + 1 + d, 0 where i + 1 + d >= n_rows. device=: a 2-D torch tensor of 32-bit entries in device memory (at least
        n_rows x L) that receives the layout instead (everything outside it stays as it was); returns None then."""
        return self._pairw_lag("STORM_dosage_pairw_lag_dot", np.uint32, max_lag, device)

    def pairw_lag_corr(self, max_lag: int, measure: str = "r2", device=None):
        """STORM_dosage_pairw_lag_corr: [n_rows, L] float32, pairw_corr's value (the same bits) of rows i and i + 1 + d."""
        return self._pairw_lag("STORM_dosage_pairw_lag_corr", np.float32, max_lag, device, DOSAGE_MEASURES[measure])

    def pairw_lag_nobs(self, max_lag: int, device=None):
        """STORM_dosage_pairw_lag_nobs: [n_rows, L] uint32, the samples neither of rows i and i + 1 + d is missing (3) at."""
        return self._pairw_lag("STORM_dosage_pairw_lag_nobs", np.uint32, max_lag, device)

    def pairw_lag_corr_complete(self, max_lag: int, measure: str = "r2", device=None):
        """STORM_dosage_pairw_lag_corr_complete: [n_rows, L] float32, pairw_corr_complete's value (the same bits) of rows i and
        i + 1 + d (value 3 = missing); memory and work are O(n_rows x L)."""
        return self._pairw_lag("STORM_dosage_pairw_lag_corr_complete", np.float32, max_lag, device, DOSAGE_MEASURES[measure])

    def lag_ldscore(self, max_lag: int, stat: str = "r2", complete: bool = False, device=None):
        """STORM_dosage_lag_ldscore[_complete]: (score [n_rows] float32, n_pairs [n_rows] uint32): for every row the sum, reduced
        on the device, of r2 ("r2") or of r2 - (1 - r2) / (N - 2) ("r2_adj") over the rows within max_lag on both sides of it,
        and the number of pairs summed (a NaN pair is not; under "r2_adj" neither is one with N < 3). complete=True: r2 over the
        samples both rows have (value 3 = missing), N = their number. The row itself is not included: LDSC's l is 1 + score.
        device=: (score, n_pairs) — two 1-D torch tensors of 32-bit entries in device memory, at least n_rows long (n_pairs
        may be None) — receive elements [0, n_rows) instead (complete on return); returns None then."""
        n = self.n_rows
        name = "STORM_dosage_lag_ldscore_complete" if complete else "STORM_dosage_lag_ldscore"
        code = LDSCORE_STATS[stat]
        if device is not None:
            d_score, d_pairs = device
            for t in (d_score, d_pairs):
                _device_vector(t, "device=: 1-D contiguous tensors of 32-bit entries in device memory")
            length = int(d_score.shape[0]) if d_pairs is None else min(int(d_score.shape[0]), int(d_pairs.shape[0]))
            self._check(name + "_device",
                        int(getattr(self._lib, name + "_device")(self._h, code, max_lag, C.c_void_p(d_score.data_ptr()),
                                                                 None if d_pairs is None else C.c_void_p(d_pairs.data_ptr()),
                                                                 length)))
            return None
        score, pairs = np.zeros(max(n, 1), dtype=np.float32), np.zeros(max(n, 1), dtype=np.uint32)
        self._check(name, int(getattr(self._lib, name)(self._h, code, max_lag, _ptr(score), _ptr(pairs), n)))
        return score[:n], pairs[:n]

    def lag_ldscore_annot(self, annot, max_lag: Optional[int] = None, stat: str = "r2", complete: bool = False, pos=None,
                          max_dist: Optional[float] = None, device=None):
        """STORM_dosage_lag_ldscore_annot[_complete]: (score [n_rows, C] float32, n_pairs [n_rows] uint32): stratified LD scores,
        score[i, c] = the sum over row i's window of annot[j, c] times lag_ldscore's term of the pair (i, j), reduced on the
        device. annot: [n_rows, C] float32, finite. The window: pos=None — the max_lag rows on each side; pos (n_rows
        non-decreasing coordinates) and max_dist — the rows within that distance, computed at the lag the windows need
        (max_lag=None) or refused when they need more than max_lag. The row itself is not included: LDSC's l is annot + score.
        device=: (score, n_pairs) — a 2-D torch float32 tensor of at least n_rows rows and C columns with unit column stride
        and a 1-D tensor of 32-bit entries (or None), in device memory, and annot a torch tensor there too — receive the
        results instead (complete on return); returns None then."""
        n = self.n_rows
        name = "STORM_dosage_lag_ldscore_annot_complete" if complete else "STORM_dosage_lag_ldscore_annot"
        code = LDSCORE_STATS[stat]
        lag, p_ptr, dist = _window_args(n, max_lag, pos, max_dist)
        if device is not None:
            d_score, d_pairs = device
            for t in (annot, d_score):
                if t.dim() != 2 or t.element_size() != 4 or not t.is_floating_point() or t.stride(1) != 1 or not t.is_cuda:
                    raise ValueError("device=: annot and score are 2-D float32 tensors with unit column stride in device memory")
            _device_vector(d_pairs, "device=: n_pairs is a 1-D contiguous tensor of 32-bit entries in device memory")
            if int(annot.shape[0]) < n or int(d_score.shape[1]) < int(annot.shape[1]):
                raise ValueError("device=: annot has a row per row of the container, score a column per column of annot")
            rows = int(d_score.shape[0]) if d_pairs is None else min(int(d_score.shape[0]), int(d_pairs.shape[0]))
            self._check(name + "_device",
                        int(getattr(self._lib, name + "_device")(self._h, code, lag, p_ptr, dist, C.c_void_p(annot.data_ptr()),
                                                                 int(annot.shape[1]), int(annot.stride(0)),
                                                                 C.c_void_p(d_score.data_ptr()), int(d_score.stride(0)),
                                                                 None if d_pairs is None else C.c_void_p(d_pairs.data_ptr()), rows)))
            return None
        a = np.ascontiguousarray(annot, dtype=np.float32)
        if a.ndim != 2 or a.shape[0] != n:
            raise ValueError("annot: [n_rows, C]")
        c = int(a.shape[1])
        score, pairs = np.zeros((max(n, 1), max(c, 1)), dtype=np.float32), np.zeros(max(n, 1), dtype=np.uint32)
        spare = np.zeros(1, dtype=np.float32)
        self._check(name, int(getattr(self._lib, name)(self._h, code, lag, p_ptr, dist, _ptr(a) if a.size else _ptr(spare), c, max(c, 1),
                                                       _ptr(score), max(c, 1), _ptr(pairs), n)))
        return score[:n, :c], pairs[:n]

    def lag_prune(self, min_r2: float, max_lag: Optional[int] = None, pos=None, max_dist: Optional[float] = None, priority=None,
                  complete: bool = False, owner: bool = False, device=None):
        """STORM_dosage_lag_prune[_complete]: keep [n_rows] uint8, or (keep, owner [n_rows] uint32) with owner=True: greedy LD
        pruning / clumping resolved on the device. Rows i < j are adjacent when they lie within max_lag rows (and, with pos and
        max_dist, within that distance: computed at the lag the windows need when max_lag is None, refused when they need
        more than max_lag) and their r2 — pairw_lag_corr's float, complete=True: pairw_lag_corr_complete's — is > min_r2. The
        rows are walked by priority ([n_rows] floats, higher first, ties to the lower row; None: row order; NaN refused) and
        a row is kept exactly when no kept row is adjacent to it; owner[i] is i for a kept row, else the kept neighbour that
        came first. A row without an edge — a constant row too — is kept. Not PLINK's --indep-pairwise.
        device=: (keep, owner) — 1-D contiguous torch tensors in device memory, uint8 and 32-bit entries (owner may be
        None), at least n_rows long — receive elements [0, n_rows) instead (complete on return); returns None then."""
        n = self.n_rows
        name = "STORM_dosage_lag_prune_complete" if complete else "STORM_dosage_lag_prune"
        lag, p_ptr, dist = _window_args(n, max_lag, pos, max_dist)
        pr = None
        if priority is not None:
            pr = np.ascontiguousarray(priority, dtype=np.float32)
            if pr.shape != (n,):
                raise ValueError("priority: one number per row")
        pr_ptr = None if pr is None else _ptr(pr if pr.size else np.zeros(1, np.float32))
        if device is not None:
            d_keep, d_owner = device
            _device_vector(d_keep, "device=: keep is a 1-D contiguous tensor of 8-bit entries in device memory", 1)
            _device_vector(d_owner, "device=: owner is a 1-D contiguous tensor of 32-bit entries in device memory")
            length = int(d_keep.shape[0]) if d_owner is None else min(int(d_keep.shape[0]), int(d_owner.shape[0]))
            self._check(name + "_device",
                        int(getattr(self._lib, name + "_device")(self._h, float(min_r2), lag, p_ptr, dist, pr_ptr,
                                                                 C.c_void_p(d_keep.data_ptr()),
                                                                 None if d_owner is None else C.c_void_p(d_owner.data_ptr()), length)))
            return None
        keep, own = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint32)
        self._check(name, int(getattr(self._lib, name)(self._h, float(min_r2), lag, p_ptr, dist, pr_ptr, _ptr(keep),
                                                       _ptr(own) if owner else None, n)))
        return (keep[:n], own[:n]) if owner else keep[:n]

    def lag_corr_sparse(self, min_r2: float, max_lag: Optional[int] = None, pos=None, max_dist: Optional[float] = None,
                        complete: bool = False, capacity: Optional[int] = None, device=None):
        """STORM_dosage_lag_corr_sparse[_complete]: (row_start [n_rows + 1] uint64, col uint32, val float32): the pairs i < j
        within max_lag rows (and, with pos and max_dist, within that distance, as lag_prune) whose r2 — pairw_lag_corr's
        float, complete=True: pairw_lag_corr_complete's — is > min_r2, compacted on the device: row i's pairs are
        col[row_start[i]:row_start[i + 1]], ascending, val their r2 (the same bits), row_start[-1] the total. Strict: a pair
        exactly at min_r2 is not listed (PLINK's filter is >=), a NaN never; a negative min_r2 lists every pair that is a number.
        capacity=None makes the count-only call and then the exact fill, which COSTS THE BAND TWICE; given a capacity, one
        call is made and a RuntimeError names the total when the capacity is too small.
        device=: (row_start, col, val) — 1-D contiguous torch tensors in device memory of 64-bit, 32-bit and float32 entries,
        row_start at least n_rows + 1 long, col and val of one length, the capacity (both None: the offsets alone) — receive
        the list instead: only the first len(col) pairs are written, row_start always holds the true offsets, and the caller
        compares row_start[n_rows] with len(col). Complete on return with pos, queued on the container's stream without;
        returns None."""
        n = self.n_rows
        name = "STORM_dosage_lag_corr_sparse_complete" if complete else "STORM_dosage_lag_corr_sparse"
        lag, p_ptr, dist = _window_args(n, max_lag, pos, max_dist)
        if device is not None:
            d_rows, d_col, d_val = device
            _device_vector(d_rows, "device=: row_start is a 1-D contiguous tensor of 64-bit entries in device memory", 8)
            for t in (d_col, d_val):
                _device_vector(t, "device=: col and val are 1-D contiguous tensors of 32-bit entries in device memory")
            if d_rows is None or (d_col is None) != (d_val is None) or (d_col is not None and d_col.shape[0] != d_val.shape[0]):
                raise ValueError("device=: row_start, and col and val of one length or both None")
            self._check(name + "_device",
                        int(getattr(self._lib, name + "_device")(self._h, float(min_r2), lag, p_ptr, dist, C.c_void_p(d_rows.data_ptr()),
                                                                 int(d_rows.shape[0]),
                                                                 None if d_col is None else C.c_void_p(d_col.data_ptr()),
                                                                 None if d_val is None else C.c_void_p(d_val.data_ptr()),
                                                                 0 if d_col is None else int(d_col.shape[0]))))
            return None
        rows = np.zeros(n + 1, dtype=np.uint64)
        total = C.c_uint64(0)
        if capacity is None:
            self._check(name, int(getattr(self._lib, name)(self._h, float(min_r2), lag, p_ptr, dist, _ptr(rows), n + 1, None, None, 0,
                                                           C.byref(total))))
            capacity = int(total.value)
        capacity = int(capacity)
        col, val = np.zeros(max(capacity, 1), dtype=np.uint32), np.zeros(max(capacity, 1), dtype=np.float32)
        rc = int(getattr(self._lib, name)(self._h, float(min_r2), lag, p_ptr, dist, _ptr(rows), n + 1, _ptr(col), _ptr(val), capacity,
                                          C.byref(total)))
        if rc == -4 and int(total.value) > capacity:
            raise RuntimeError(f"{name}: {int(total.value)} pairs are listed, capacity is {capacity}")
        self._check(name, rc)
        return rows, col[:int(total.value)], val[:int(total.value)]

    def ldscore_window_lag(self, pos, max_dist: float) -> int:
        """STORM_ldscore_window_lag: the lag the windows of these coordinates need under max_dist (host only)."""
        p = np.ascontiguousarray(pos, dtype=np.float64)
        out = C.c_uint64(0)
        self._check("STORM_ldscore_window_lag",
                    int(self._lib.STORM_ldscore_window_lag(C.c_void_p(p.ctypes.data if p.size else 0), int(p.size), float(max_dist),
                                                           C.byref(out))))
        return int(out.value)

    def free(self) -> None:
        if self._h:
            self._lib.STORM_dosage_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Storm(_LagForms, _TopkForms):
    """STORM_t (storm.h:175-178, :225-232): rows of 65536-bit blocks, list or bitmap kind."""
    _LAG = "STORM_"

    def __init__(self):
        self._lib = _lib.load()
        self._h = self._lib.STORM_new()  # storm.c:827
        if not self._h:
            raise MemoryError("STORM_new")

    def add(self, values) -> int:
        v = _u32(values)
        return int(self._lib.STORM_add(self._h, _ptr(v) if v.size else _ptr(np.zeros(1, np.uint32)),
                                       v.size))  # storm.c:844

    def add_synthetic(self, n_bits: int, n_rows: int, draws: int, seed: int = 42,
                      row0: int = 0) -> int:
        return int(self._lib.storm_synth_fill_storm(self._h, n_bits, row0, n_rows, draws, seed))

    def clear(self) -> int:
        return int(self._lib.STORM_clear(self._h))  # storm.c:868

    @property
    def n_rows(self) -> int:
        """Rows added so far (STORM_n_rows)."""
        return int(self._lib.STORM_n_rows(self._h))

    def pairw_matrix(self, op: str = "and") -> np.ndarray:
        """STORM_pairw_matrix (extension): [n_rows, n_rows] uint32, entry (i, j), i < j = what
        STORM_bitmap_cont_intersect_cardinality gives for rows i and j (storm.c:790-814); "or" / "xor": the union /
        symmetric-difference counts."""
        n = self.n_rows
        out = np.zeros((n, n), dtype=np.uint32)
        rc = int(self._lib.STORM_pairw_matrix(self._h, {"and": 0, "or": 1, "xor": 2}[op], _ptr(out), n, n))
        if rc != 0:
            raise RuntimeError(f"STORM_pairw_matrix -> {rc}: {self._lib.STORM_hip_error().decode()}")
        return out

    def pairw_matrix_device(self, d_out: int, out_rows: int, out_ld: int, op: str = "and") -> None:
        """STORM_pairw_matrix_device (extension): the same triangle left in device memory at address d_out."""
        rc = int(self._lib.STORM_pairw_matrix_device(self._h, {"and": 0, "or": 1, "xor": 2}[op], C.c_void_p(d_out),
                                                     out_rows, out_ld))
        if rc != 0:
            raise RuntimeError(f"STORM_pairw_matrix_device -> {rc}: {self._lib.STORM_hip_error().decode()}")

    def intersect_cardinality_square(self, other: "Storm") -> int:
        """STORM_intersect_cardinality_square (declared by the reference, storm.h:231): the sum over every row i of self
        and j of other of STORM_bitmap_cont_intersect_cardinality(row_i, row_j)."""
        return _all_pairs(self._lib.STORM_intersect_cardinality_square(self._h, other._h),
                          "STORM_intersect_cardinality_square")

    def square_matrix(self, other: "Storm", op: str = "and") -> np.ndarray:
        """STORM_square_matrix (extension): [self.n_rows, other.n_rows] uint32, every entry (i, j) = popcount(row_i OP
        other_j)."""
        na, nb = self.n_rows, other.n_rows
        out = np.zeros((na, nb), dtype=np.uint32)
        rc = int(self._lib.STORM_square_matrix(self._h, other._h, {"and": 0, "or": 1, "xor": 2}[op],
                                               _ptr(out) if out.size else _ptr(np.zeros(1, np.uint32)), na, nb))
        if rc != 0:
            raise RuntimeError(f"STORM_square_matrix -> {rc}: {self._lib.STORM_hip_error().decode()}")
        return out

    def square_matrix_device(self, other: "Storm", d_out: int, out_rows: int, out_ld: int, op: str = "and") -> None:
        """STORM_square_matrix_device (extension): the same rectangle left in device memory at address d_out."""
        rc = int(self._lib.STORM_square_matrix_device(self._h, other._h, {"and": 0, "or": 1, "xor": 2}[op],
                                                      C.c_void_p(d_out), out_rows, out_ld))
        if rc != 0:
            raise RuntimeError(f"STORM_square_matrix_device -> {rc}: {self._lib.STORM_hip_error().decode()}")

    def pairw_similarity(self, measure: str = "jaccard", n_bits: int = 0) -> np.ndarray:
        """STORM_pairw_similarity (extension): [n_rows, n_rows] float32, entry (i, j), i < j = the measure ("jaccard",
        "cosine", "ld_d", "ld_r2") of rows i and j, finished on the device; 0 for i >= j. The LD measures need n_bits, the
        size of the universe (a STORM_t declares none)."""
        n = self.n_rows
        out = np.zeros((n, n), dtype=np.float32)
        _similarity(self._lib, "STORM_pairw_similarity",
                    int(self._lib.STORM_pairw_similarity(self._h, MEASURES[measure], n_bits,
                                                         _ptr(out) if out.size else _ptr(np.zeros(1, np.float32)), n, n)))
        return out

    def pairw_similarity_device(self, d_out: int, out_rows: int, out_ld: int, measure: str = "jaccard", n_bits: int = 0) -> None:
        """STORM_pairw_similarity_device (extension): the same triangle left in device memory at address d_out."""
        _similarity(self._lib, "STORM_pairw_similarity_device",
                    int(self._lib.STORM_pairw_similarity_device(self._h, MEASURES[measure], n_bits, C.c_void_p(d_out),
                                                                out_rows, out_ld)))

    def square_similarity(self, other: "Storm", measure: str = "jaccard", n_bits: int = 0) -> np.ndarray:
        """STORM_square_similarity (extension): [self.n_rows, other.n_rows] float32, every entry (i, j) = the measure of
        row i of self and row j of other."""
        na, nb = self.n_rows, other.n_rows
        out = np.zeros((na, nb), dtype=np.float32)
        _similarity(self._lib, "STORM_square_similarity",
                    int(self._lib.STORM_square_similarity(self._h, other._h, MEASURES[measure], n_bits,
                                                          _ptr(out) if out.size else _ptr(np.zeros(1, np.float32)), na, nb)))
        return out

    def square_similarity_device(self, other: "Storm", d_out: int, out_rows: int, out_ld: int, measure: str = "jaccard",
                                 n_bits: int = 0) -> None:
        """STORM_square_similarity_device (extension): the same rectangle left in device memory at address d_out."""
        _similarity(self._lib, "STORM_square_similarity_device",
                    int(self._lib.STORM_square_similarity_device(self._h, other._h, MEASURES[measure], n_bits,
                                                                 C.c_void_p(d_out), out_rows, out_ld)))

    def square_topk(self, other: "Storm", k: int, score: str = "jaccard", n_bits: int = 0, panel_rows: int = 0):
        """STORM_square_topk (extension): (idx, val) of [self.n_rows, k]: for each row of self its k most similar rows of
        other (see pairw_topk)."""
        na = self.n_rows
        idx, val = _topk_out(na, k, score)
        spare = np.zeros(1, np.uint32)
        _similarity(self._lib, "STORM_square_topk",
                    int(self._lib.STORM_square_topk(self._h, other._h, SCORES[score], n_bits, k, panel_rows,
                                                    _ptr(idx) if idx.size else _ptr(spare),
                                                    _ptr(val) if val.size else _ptr(spare), na, k)))
        return idx, val

    def square_topk_device(self, other: "Storm", d_idx: int, d_val: int, out_rows: int, out_ld: int, k: int,
                           score: str = "jaccard", n_bits: int = 0, panel_rows: int = 0) -> None:
        """STORM_square_topk_device (extension): the same left in device memory at addresses d_idx / d_val."""
        _similarity(self._lib, "STORM_square_topk_device",
                    int(self._lib.STORM_square_topk_device(self._h, other._h, SCORES[score], n_bits, k, panel_rows,
                                                           C.c_void_p(d_idx), C.c_void_p(d_val), out_rows, out_ld)))

    def serialized_size(self) -> int:
        return int(self._lib.STORM_serialized_size(self._h))  # storm.c:963

    def hip_invalidate(self) -> None:
        """STORM_hip_invalidate (storm.h extension)."""
        self._lib.STORM_hip_invalidate(self._h)

    def serialize(self) -> np.ndarray:
        """STORM_serialize: exactly STORM_serialized_size(h) bytes (uint8 array)."""
        n = self.serialized_size()
        buf = np.zeros(n + (n & 1), dtype=np.uint8)
        got = int(self._lib.STORM_serialize(self._h, _ptr(buf), n))
        if got != n:
            raise RuntimeError(f"STORM_serialize wrote {got} of {n} bytes")
        return buf[:n]

    @classmethod
    def deserialize(cls, data) -> "Storm":
        """STORM_deserialize; ValueError on a malformed stream."""
        buf = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8))
        self = cls.__new__(cls)
        self._lib = _lib.load()
        self._h = self._lib.STORM_deserialize(_ptr(buf), buf.size)
        if not self._h:
            raise ValueError("STORM_deserialize: malformed stream")
        return self

    @staticmethod
    def serialized_pairw_intersect_cardinality(data) -> int:
        """All-pairs total of a serialized container, arena built on the device from the bytes."""
        buf = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8))
        lib = _lib.load()
        return _all_pairs(lib.STORM_serialized_pairw_intersect_cardinality(_ptr(buf), buf.size),
                          "STORM_serialized_pairw_intersect_cardinality")

    def pairw_intersect_cardinality(self) -> int:
        return _all_pairs(self._lib.STORM_pairw_intersect_cardinality(self._h),
                          "STORM_pairw_intersect_cardinality")  # storm.c:877

    def pairw_intersect_cardinality_blocked(self, bsize: int = 0) -> int:
        return _all_pairs(self._lib.STORM_pairw_intersect_cardinality_blocked(self._h, bsize),
                          "STORM_pairw_intersect_cardinality_blocked")  # storm.c:897

    def free(self) -> None:
        if self._h:
            self._lib.STORM_free(self._h)  # storm.c:836
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def wrapper_diag(vals: np.ndarray) -> int:
    """STORM_wrapper_diag (storm.c:132): all pairs of the rows of a host uint64 matrix."""
    lib = _lib.load()
    v = np.ascontiguousarray(vals, dtype=np.uint64)
    return _all_pairs(lib.STORM_wrapper_diag(v.shape[0], _ptr(v), v.shape[1], None),
                      "STORM_wrapper_diag")


def wrapper_diag_blocked(vals: np.ndarray, block_size: int = 0) -> int:
    """STORM_wrapper_diag_blocked (storm.c:222)."""
    lib = _lib.load()
    v = np.ascontiguousarray(vals, dtype=np.uint64)
    return _all_pairs(
        lib.STORM_wrapper_diag_blocked(v.shape[0], _ptr(v), v.shape[1], None, block_size),
        "STORM_wrapper_diag_blocked")


def wrapper_square(vals1: np.ndarray, vals2: np.ndarray) -> int:
    """STORM_wrapper_square (storm.c:153): every row of vals1 against every row of vals2."""
    lib = _lib.load()
    a = np.ascontiguousarray(vals1, dtype=np.uint64)
    b = np.ascontiguousarray(vals2, dtype=np.uint64)
    if a.shape[1] != b.shape[1]:
        raise ValueError("row widths differ")
    return _all_pairs(lib.STORM_wrapper_square(a.shape[0], _ptr(a), b.shape[0], _ptr(b),
                                               a.shape[1], None), "STORM_wrapper_square")


# ------------------------------------------------------------------------------------------
# device-level handles (include/storm_hip.h)
# ------------------------------------------------------------------------------------------
class HipContext:
    """storm_hip_ctx_t: one MI355X + stream + workspace."""

    def __init__(self, device: int = 0, stream: int = 0):
        self._lib = _lib.load()
        h = C.c_void_p()
        check(self._lib.storm_hip_ctx_create(device, C.c_void_p(stream), C.byref(h)),
              "storm_hip_ctx_create")
        self._h = h
        self.device = device

    def set_stream(self, stream: int) -> None:
        check(self._lib.storm_hip_ctx_set_stream(self._h, C.c_void_p(stream)),
              "storm_hip_ctx_set_stream")

    def synchronize(self) -> None:
        check(self._lib.storm_hip_ctx_synchronize(self._h), "storm_hip_ctx_synchronize")

    def set_option(self, key: str, value: int) -> None:
        check(self._lib.storm_hip_ctx_set_option(self._h, key.encode(), value),
              f"storm_hip_ctx_set_option({key})")

    def get_option(self, key: str) -> int:
        return int(self._lib.storm_hip_ctx_get_option(self._h, key.encode()))

    def kernel_time(self):
        """(summed ms, launches) of the dominant kernel since the last call; needs the
        "time_kernels" option (storm_hip.h)."""
        ms, n = C.c_double(0), C.c_uint64(0)
        check(self._lib.storm_hip_kernel_time(self._h, C.byref(ms), C.byref(n)),
              "storm_hip_kernel_time")
        return float(ms.value), int(n.value)

    def last_launch_info(self) -> dict:
        out = (C.c_uint64 * 4)()
        check(self._lib.storm_hip_last_launch_info(self._h, C.byref(out)),
              "storm_hip_last_launch_info")
        return {"items": out[0], "chunks_per_item": out[1], "word_pairs_executed": out[2],
                "segments": out[3]}

    def last_pass_report(self) -> dict:
        """What the last all-pairs pass ran (storm_hip.h: storm_hip_last_pass_report)."""
        out = (C.c_uint64 * 4)()
        check(self._lib.storm_hip_last_pass_report(self._h, out), "storm_hip_last_pass_report")
        names = {1: "pairw_dense_kernel", 2: "pairw_fp4_kernel", 4: "strip16_fp4_kernel", 8: "bitstream_kernel",
                 16: "strip16_bits_kernel", 32: "probe_lists_kernel", 512: "finish_tiles_kernel"}
        return {"kernels": [n for b, n in names.items() if out[0] & b], "dense_word_pairs": int(out[1]),
                "probe_lookups": int(out[2]), "rows_per_lookup": int(out[3])}

    def lag_band_sums_device(self, d_vals: int, ld: int, n_rows: int, max_lag: int, d_score: int, d_n_pairs: Optional[int] = None,
                             stat: str = "r2", n_const: int = 0, d_nobs: Optional[int] = None, nobs_row_pitch: int = 0,
                             nobs_col_stride: int = 1) -> None:
        """storm_hip_lag_band_sums_device: per-row sums over both sides of a float band in the lag layout at d_vals (n_rows rows
        of pitch ld, device memory) into d_score / d_n_pairs (n_rows entries each, device memory); N of "r2_adj" is n_const
        or the uint32 at d_nobs[i * nobs_row_pitch + d * nobs_col_stride]. The C call returns with its work
        queued: order later work on the context's stream or call `synchronize()`."""
        check(self._lib.storm_hip_lag_band_sums_device(self._h, C.c_void_p(d_vals), ld, n_rows, max_lag, LDSCORE_STATS[stat], n_const,
                                                       None if d_nobs is None else C.c_void_p(d_nobs), nobs_row_pitch,
                                                       nobs_col_stride, C.c_void_p(d_score),
                                                       None if d_n_pairs is None else C.c_void_p(d_n_pairs)),
              "storm_hip_lag_band_sums_device")

    def lag_band_annot_sums_device(self, d_vals: int, ld: int, n_rows: int, max_lag: int, d_annot: int, annot_ld: int, n_annot: int,
                                   d_score: int, score_ld: int, d_n_pairs: Optional[int] = None, stat: str = "r2", n_const: int = 0,
                                   d_nobs: Optional[int] = None, nobs_row_pitch: int = 0, nobs_col_stride: int = 1,
                                   d_lo: Optional[int] = None, d_hi: Optional[int] = None) -> None:
        """storm_hip_lag_band_annot_sums_device: the band at d_vals times the n_rows x n_annot annotations at d_annot, within
        the windows [d_lo[i], d_hi[i]] (uint32, both or neither: the whole lag), into d_score (pitch score_ld) and d_n_pairs;
        everything in device memory. The C call returns with its work
        queued: order later work on the context's stream or call `synchronize()`."""
        opt = lambda p: None if p is None else C.c_void_p(p)
        check(self._lib.storm_hip_lag_band_annot_sums_device(self._h, C.c_void_p(d_vals), ld, n_rows, max_lag, LDSCORE_STATS[stat],
                                                             n_const, opt(d_nobs), nobs_row_pitch, nobs_col_stride, opt(d_lo),
                                                             opt(d_hi), C.c_void_p(d_annot), annot_ld, n_annot, C.c_void_p(d_score),
                                                             score_ld, opt(d_n_pairs)),
              "storm_hip_lag_band_annot_sums_device")

    def lag_band_prune_device(self, d_vals: int, ld: int, n_rows: int, max_lag: int, min_r2: float, d_keep: int,
                              d_owner: Optional[int] = None, lo: Optional[np.ndarray] = None, hi: Optional[np.ndarray] = None,
                              order: Optional[np.ndarray] = None) -> None:
        """storm_hip_lag_band_prune_device: greedy pruning / clumping over a float band in the lag layout at d_vals (n_rows rows
        of pitch ld, device memory): rows i < j within max_lag, with j <= hi[i] and i >= lo[j] (host uint32 arrays, both or
        neither) and an entry > min_r2 are adjacent; walked in `order` (a host permutation; None: row order), a row is kept
        when no kept row is adjacent to it. d_keep (n_rows uint8) and d_owner (n_rows uint32, may be None) are device memory.
        The C call returns with its work queued and the host arrays still to be read; this wrapper owns their copies and
        waits."""
        u32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint32)
        lo, hi, order = u32(lo), u32(hi), u32(order)
        opt = lambda a: None if a is None else _ptr(a if a.size else np.zeros(1, np.uint32))
        check(self._lib.storm_hip_lag_band_prune_device(self._h, C.c_void_p(d_vals), ld, n_rows, max_lag, float(min_r2), opt(lo),
                                                        opt(hi), opt(order), C.c_void_p(d_keep),
                                                        None if d_owner is None else C.c_void_p(d_owner)),
              "storm_hip_lag_band_prune_device")
        self.synchronize()   # (lo / hi / order are this call's own copies: they must outlive the upload)

    def lag_band_sparse_device(self, d_vals: int, ld: int, n_rows: int, max_lag: int, min_r2: float, d_row_start: int,
                               d_col: Optional[int] = None, d_val: Optional[int] = None, capacity: int = 0,
                               lo: Optional[np.ndarray] = None, hi: Optional[np.ndarray] = None, wait: bool = True) -> None:
        """storm_hip_lag_band_sparse_device: the pairs of a float band in the lag layout at d_vals (n_rows rows of pitch ld,
        device memory) that lag_band_prune_device calls adjacent, as a CSR list in device memory: d_row_start (n_rows + 1
        uint64: the true offsets, the total last), d_col / d_val (uint32 j ascending / the band's float; both None with
        capacity 0: the offsets alone). Only the first `capacity` pairs are written. lo / hi: host uint32 arrays, both or
        neither. The C call returns with its work queued and the host arrays still to be read; this wrapper owns their copies
        and waits (wait=False, without lo / hi only: queued on the context's stream)."""
        u32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint32)
        lo, hi = u32(lo), u32(hi)
        opt = lambda a: None if a is None else _ptr(a if a.size else np.zeros(1, np.uint32))
        dev = lambda p: None if p is None else C.c_void_p(p)
        check(self._lib.storm_hip_lag_band_sparse_device(self._h, dev(d_vals), ld, n_rows, max_lag, float(min_r2), opt(lo), opt(hi),
                                                         dev(d_row_start), dev(d_col), dev(d_val), capacity),
              "storm_hip_lag_band_sparse_device")
        if wait or lo is not None or hi is not None:
            self.synchronize()   # (lo / hi are this call's own copies: they must outlive the upload)

    def matrix(self, n_rows: int, n_words: int) -> "HipMatrix":
        return HipMatrix(self, n_rows, n_words)

    def matrix_from_host(self, vals: np.ndarray) -> "HipMatrix":
        v = np.ascontiguousarray(vals, dtype=np.uint64)
        m = HipMatrix(self, v.shape[0], v.shape[1])
        m.upload(v)
        return m

    def close(self) -> None:
        if self._h:
            self._lib.storm_hip_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipMatrix:
    """storm_hip_matrix_t: dense uint64 bitmap rows resident in HBM (padded layout)."""

    def __init__(self, ctx: HipContext, n_rows: int, n_words: int):
        self.ctx = ctx
        self._lib = ctx._lib
        h = C.c_void_p()
        check(self._lib.storm_hip_matrix_create(ctx._h, n_rows, n_words, C.byref(h)),
              "storm_hip_matrix_create")
        self._h = h
        self.n_rows, self.n_words = n_rows, n_words

    # -- data movement
    def upload(self, vals: np.ndarray, row0: int = 0) -> None:
        v = np.ascontiguousarray(vals, dtype=np.uint64)
        check(self._lib.storm_hip_matrix_upload(self.ctx._h, self._h, row0, v.shape[0], _ptr(v),
                                                v.shape[1]), "storm_hip_matrix_upload")

    def import_device(self, data_ptr: int, n_rows: int, stride_words: int, row0: int = 0) -> None:
        check(self._lib.storm_hip_matrix_import(self.ctx._h, self._h, row0, n_rows,
                                                C.c_void_p(data_ptr), stride_words),
              "storm_hip_matrix_import")

    def download(self, row0: int = 0, n_rows: Optional[int] = None) -> np.ndarray:
        n = self.n_rows - row0 if n_rows is None else n_rows
        out = np.zeros((n, self.n_words), dtype=np.uint64)
        check(self._lib.storm_hip_matrix_download(self.ctx._h, self._h, row0, n, _ptr(out),
                                                  self.n_words), "storm_hip_matrix_download")
        return out

    def set_rows_from_positions(self, rows: Sequence[Iterable[int]], row0: int = 0) -> None:
        """storm_hip_matrix_set_rows_from_positions: SETS the listed bits of rows [row0, row0 + len(rows)) (the bit-setting loop
        of STORM_contig_add on the device); bits a row already has stay set — clear or upload first to replace a row."""
        arrs = [_u32(r) for r in rows]
        offs = np.zeros(len(arrs) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([a.size for a in arrs], dtype=np.uint64)
        pos = np.concatenate(arrs) if arrs and offs[-1] else np.zeros(1, dtype=np.uint32)
        check(self._lib.storm_hip_matrix_set_rows_from_positions(
            self.ctx._h, self._h, row0, len(arrs), _ptr(offs), _ptr(pos)),
            "storm_hip_matrix_set_rows_from_positions")

    def fill_synthetic(self, n_bits: int, draws: int, seed: int = 42) -> None:
        check(self._lib.storm_hip_matrix_fill_synthetic(self.ctx._h, self._h, n_bits, draws,
                                                        seed), "storm_hip_matrix_fill_synthetic")

    def clear(self) -> None:
        check(self._lib.storm_hip_matrix_clear(self.ctx._h, self._h), "storm_hip_matrix_clear")

    def resize(self, n_rows: int) -> None:
        """storm_hip_matrix_resize: change the logical row count. Rows dropped by a shrink are cleared, rows gained are
        zero until uploaded; growing beyond the allocation reallocates and keeps the rows."""
        check(self._lib.storm_hip_matrix_resize(self.ctx._h, self._h, n_rows), "storm_hip_matrix_resize")
        self.n_rows = n_rows

    @property
    def device_ptr(self) -> int:
        return int(self._lib.storm_hip_matrix_device_ptr(self._h) or 0)

    @property
    def stride_words(self) -> int:
        return int(self._lib.storm_hip_matrix_stride_words(self._h))

    # -- the hot path
    def pairw(self, shard_rank: int = 0, shard_count: int = 1) -> int:
        out = C.c_uint64()
        check(self._lib.storm_hip_pairw_dense(self.ctx._h, self._h, shard_rank, shard_count,
                                              C.byref(out)), "storm_hip_pairw_dense")
        return int(out.value)

    def pairw_launch(self, d_total_ptr: int, shard_rank: int = 0, shard_count: int = 1) -> None:
        """Asynchronous on the context's stream; d_total_ptr = device pointer to one uint64."""
        check(self._lib.storm_hip_pairw_dense_launch(self.ctx._h, self._h, shard_rank,
                                                     shard_count, C.c_void_p(d_total_ptr)),
              "storm_hip_pairw_dense_launch")

    def pairw_upload(self, host_rows: np.ndarray) -> int:
        """storm_hip_pairw_dense_upload: `host_rows` ([n_rows, >= n_words] uint64; a wider array's surplus words are not
        read) replace all rows of the matrix while the pass multiplies the panels that have landed; the all-pairs total."""
        v = np.ascontiguousarray(host_rows, dtype=np.uint64)
        if v.ndim != 2 or v.shape[0] != self.n_rows:
            raise ValueError(f"pairw_upload: {v.shape} is not [{self.n_rows}, >= {self.n_words}]")
        out = C.c_uint64()
        check(self._lib.storm_hip_pairw_dense_upload(self.ctx._h, self._h, _ptr(v), v.shape[1], C.byref(out)),
              "storm_hip_pairw_dense_upload")
        return int(out.value)

    def square(self, other: "HipMatrix") -> int:
        out = C.c_uint64()
        check(self._lib.storm_hip_square_dense(self.ctx._h, self._h, other._h, C.byref(out)),
              "storm_hip_square_dense")
        return int(out.value)

    def tile_counts(self, i0: int, i1: int, j0: int, j1: int) -> np.ndarray:
        out = np.zeros((i1 - i0, j1 - j0), dtype=np.uint32)
        check(self._lib.storm_hip_tile_counts(self.ctx._h, self._h, i0, i1, j0, j1, _ptr(out)),
              "storm_hip_tile_counts")
        return out

    OPS = {"and": 0, "or": 1, "xor": 2}

    def pairw_matrix(self, op: str = "and") -> np.ndarray:
        """[n_rows, n_rows] uint32, entry (i, j) = popcount(row_i OP row_j) for i < j, else 0."""
        out = np.zeros((self.n_rows, self.n_rows), dtype=np.uint32)
        check(self._lib.storm_hip_pairw_matrix(self.ctx._h, self._h, self.OPS[op], _ptr(out)),
              "storm_hip_pairw_matrix")
        return out

    def pairw_matrix_device(self, d_out: int, ld: int, op: str = "and") -> None:
        """Same, into a device buffer (address `d_out`, n_rows x ld uint32); synchronous."""
        check(self._lib.storm_hip_pairw_matrix_device(self.ctx._h, self._h, self.OPS[op],
                                                      C.c_void_p(d_out), ld),
              "storm_hip_pairw_matrix_device")

    def square_matrix(self, other: "HipMatrix", op: str = "and") -> np.ndarray:
        """[self.n_rows, other.n_rows] uint32: popcount(row_i(self) OP row_j(other)) for all i, j."""
        out = np.zeros((self.n_rows, other.n_rows), dtype=np.uint32)
        check(self._lib.storm_hip_square_matrix(self.ctx._h, self._h, other._h, self.OPS[op], _ptr(out)),
              "storm_hip_square_matrix")
        return out

    def pairw_matrix_band_device(self, d_out: int, ld: int, row0: int, n_band_rows: int,
                                 op: str = "and") -> None:
        """Rows [row0, row0 + n_band_rows) of the triangle into a device buffer (n_band_rows x ld)."""
        check(self._lib.storm_hip_pairw_matrix_band_device(self.ctx._h, self._h, self.OPS[op], row0,
                                                           n_band_rows, C.c_void_p(d_out), ld),
              "storm_hip_pairw_matrix_band_device")

    def _lag_width(self, max_lag: int) -> int:
        return min(max_lag, max(self.n_rows - 1, 0))

    def pairw_lag_matrix(self, max_lag: int, op: str = "and") -> np.ndarray:
        """[n_rows, L] uint32, L = min(max_lag, n_rows - 1): entry (i, d) = popcount(row_i OP row_{i+1+d}), 0 where
        i + 1 + d >= n_rows (the lag layout of storm_hip.h)."""
        w = self._lag_width(max_lag)
        out = np.zeros((self.n_rows, w), dtype=np.uint32)
        check(self._lib.storm_hip_pairw_lag_matrix(self.ctx._h, self._h, self.OPS[op], max_lag,
                                                   _ptr(out) if out.size else _ptr(np.zeros(1, np.uint32)), w),
              "storm_hip_pairw_lag_matrix")
        return out

    def pairw_lag_matrix_device(self, d_out: int, ld: int, max_lag: int, op: str = "and", row0: int = 0,
                                n_band_rows: Optional[int] = None) -> None:
        """Same, rows [row0, row0 + n_band_rows) (None: all) into a device buffer (n_band_rows x ld uint32); synchronous."""
        check(self._lib.storm_hip_pairw_lag_matrix_device(self.ctx._h, self._h, self.OPS[op], max_lag, row0,
                                                          (1 << 64) - 1 if n_band_rows is None else n_band_rows,
                                                          C.c_void_p(d_out), ld),
              "storm_hip_pairw_lag_matrix_device")

    def pairw_lag_similarity(self, max_lag: int, measure: str = "jaccard", n_bits: int = 1) -> np.ndarray:
        """[n_rows, L] float32: the measure of rows i and i + 1 + d, +0.0 in the corner."""
        w = self._lag_width(max_lag)
        out = np.zeros((self.n_rows, w), dtype=np.float32)
        check(self._lib.storm_hip_pairw_lag_similarity(self.ctx._h, self._h, MEASURES[measure], n_bits, max_lag,
                                                       _ptr(out) if out.size else _ptr(np.zeros(1, np.float32)), w),
              "storm_hip_pairw_lag_similarity")
        return out

    def pairw_lag_similarity_device(self, d_out: int, ld: int, max_lag: int, measure: str = "jaccard", n_bits: int = 1) -> None:
        """Same, into a device buffer (n_rows x ld float32); complete on return."""
        check(self._lib.storm_hip_pairw_lag_similarity_device(self.ctx._h, self._h, MEASURES[measure], n_bits, max_lag,
                                                              C.c_void_p(d_out), ld),
              "storm_hip_pairw_lag_similarity_device")

    def similarity_finish_lag_device(self, d_io: int, ld: int, max_lag: int, d_counts: int, measure: str = "jaccard",
                                     n_bits: int = 1, row0: int = 0, n_band_rows: Optional[int] = None) -> None:
        """The finish pass alone over a count matrix in the lag layout at d_io (d_counts: n_rows uint32 set-bit counts on the
        device); asynchronous on the context's stream."""
        check(self._lib.storm_hip_similarity_finish_lag_device(self.ctx._h, C.c_void_p(d_io), ld, self.n_rows, row0,
                                                               (1 << 64) - 1 if n_band_rows is None else n_band_rows, max_lag,
                                                               C.c_void_p(d_counts), MEASURES[measure], n_bits),
              "storm_hip_similarity_finish_lag_device")

    # ---- a matrix whose rows hold 2-bit dosages (32 values per word), in the lag layout (storm_hip.h) ----
    def _lag_dosage_host(self, name: str, dtype, max_lag: int, *args) -> np.ndarray:
        w = self._lag_width(max_lag)
        out = np.zeros((self.n_rows, w), dtype=dtype)
        check(getattr(self._lib, name)(self.ctx._h, self._h, *args, max_lag, _ptr(out) if out.size else _ptr(np.zeros(1, dtype)), w),
              name)
        return out

    def pairw_lag_dosage_matrix(self, max_lag: int) -> np.ndarray:
        """[n_rows, L] uint32: entry (i, d) = sum_s v_i[s] v_{i+1+d}[s] of the rows' 2-bit values, 0 in the corner."""
        return self._lag_dosage_host("storm_hip_pairw_lag_dosage_matrix", np.uint32, max_lag)

    def pairw_lag_dosage_matrix_device(self, d_out: int, ld: int, max_lag: int, row0: int = 0,
                                       n_band_rows: Optional[int] = None) -> None:
        """Same, rows [row0, row0 + n_band_rows) (None: all) into a device buffer (n_band_rows x ld uint32); synchronous."""
        check(self._lib.storm_hip_pairw_lag_dosage_matrix_device(self.ctx._h, self._h, max_lag, row0,
                                                                 (1 << 64) - 1 if n_band_rows is None else n_band_rows,
                                                                 C.c_void_p(d_out), ld),
              "storm_hip_pairw_lag_dosage_matrix_device")

    def pairw_lag_dosage_corr(self, max_lag: int, n_samples: int, measure: str = "r2") -> np.ndarray:
        """[n_rows, L] float32: the genotype correlation ("r") of rows i and i + 1 + d or its square ("r2"), +0.0 in the corner."""
        return self._lag_dosage_host("storm_hip_pairw_lag_dosage_corr", np.float32, max_lag, DOSAGE_MEASURES[measure], n_samples)

    def pairw_lag_dosage_corr_device(self, d_out: int, ld: int, max_lag: int, n_samples: int, measure: str = "r2") -> None:
        """Same, into a device buffer (n_rows x ld float32); complete on return."""
        check(self._lib.storm_hip_pairw_lag_dosage_corr_device(self.ctx._h, self._h, DOSAGE_MEASURES[measure], n_samples, max_lag,
                                                               C.c_void_p(d_out), ld),
              "storm_hip_pairw_lag_dosage_corr_device")

    def dosage_finish_lag_device(self, d_io: int, ld: int, max_lag: int, d_sum: int, d_sum_sq: int, n_samples: int,
                                 measure: str = "r2", row0: int = 0, n_band_rows: Optional[int] = None) -> None:
        """The finish pass alone over a matrix of dot products in the lag layout at d_io (d_sum, d_sum_sq: n_rows uint32 each
        on the device); asynchronous on the context's stream."""
        check(self._lib.storm_hip_dosage_finish_lag_device(self.ctx._h, C.c_void_p(d_io), ld, self.n_rows, row0,
                                                           (1 << 64) - 1 if n_band_rows is None else n_band_rows, max_lag,
                                                           C.c_void_p(d_sum), C.c_void_p(d_sum_sq), DOSAGE_MEASURES[measure],
                                                           n_samples),
              "storm_hip_dosage_finish_lag_device")

    def pairw_lag_dosage_nobs(self, max_lag: int, n_samples: int) -> np.ndarray:
        """[n_rows, L] uint32: the samples neither of rows i and i + 1 + d is missing (value 3) at, 0 in the corner."""
        return self._lag_dosage_host("storm_hip_pairw_lag_dosage_nobs", np.uint32, max_lag, n_samples)

    def pairw_lag_dosage_nobs_device(self, d_out: int, ld: int, max_lag: int, n_samples: int) -> None:
        check(self._lib.storm_hip_pairw_lag_dosage_nobs_device(self.ctx._h, self._h, n_samples, max_lag, C.c_void_p(d_out), ld),
              "storm_hip_pairw_lag_dosage_nobs_device")

    def pairw_lag_dosage_corr_complete(self, max_lag: int, n_samples: int, measure: str = "r2") -> np.ndarray:
        """[n_rows, L] float32: pairw_lag_dosage_corr over the samples both rows have (value 3 = missing)."""
        return self._lag_dosage_host("storm_hip_pairw_lag_dosage_corr_complete", np.float32, max_lag, DOSAGE_MEASURES[measure],
                                     n_samples)

    def pairw_lag_dosage_corr_complete_device(self, d_out: int, ld: int, max_lag: int, n_samples: int, measure: str = "r2") -> None:
        check(self._lib.storm_hip_pairw_lag_dosage_corr_complete_device(self.ctx._h, self._h, DOSAGE_MEASURES[measure], n_samples,
                                                                        max_lag, C.c_void_p(d_out), ld),
              "storm_hip_pairw_lag_dosage_corr_complete_device")

    # ---- LD scores: per-row sums over both sides of a band in the lag layout (storm_hip.h) ----
    def lag_dosage_ldscore(self, max_lag: int, n_samples: int, stat: str = "r2", complete: bool = False):
        """(score [n_rows] float32, n_pairs [n_rows] uint32): the sums of r2 ("r2") or its small-sample correction ("r2_adj")
        over the rows within max_lag on both sides of every row; complete=True: over the samples both rows have."""
        name = "storm_hip_lag_dosage_ldscore_complete" if complete else "storm_hip_lag_dosage_ldscore"
        n = self.n_rows
        score, pairs = np.zeros(max(n, 1), dtype=np.float32), np.zeros(max(n, 1), dtype=np.uint32)
        check(getattr(self._lib, name)(self.ctx._h, self._h, LDSCORE_STATS[stat], n_samples, max_lag, _ptr(score), _ptr(pairs)), name)
        return score[:n], pairs[:n]

    def lag_dosage_ldscore_device(self, d_score: int, d_n_pairs: Optional[int], max_lag: int, n_samples: int, stat: str = "r2",
                                  complete: bool = False) -> None:
        """Same, into device buffers of n_rows entries each (d_n_pairs may be None). The C call returns with its work
        queued: order later work on the context's stream or call `synchronize()`."""
        name = "storm_hip_lag_dosage_ldscore_complete_device" if complete else "storm_hip_lag_dosage_ldscore_device"
        check(getattr(self._lib, name)(self.ctx._h, self._h, LDSCORE_STATS[stat], n_samples, max_lag, C.c_void_p(d_score),
                                       None if d_n_pairs is None else C.c_void_p(d_n_pairs)), name)

    def lag_dosage_ldscore_annot(self, annot: np.ndarray, max_lag: int, n_samples: int, stat: str = "r2", complete: bool = False,
                                 lo: Optional[np.ndarray] = None, hi: Optional[np.ndarray] = None):
        """(score [n_rows, C] float32, n_pairs [n_rows] uint32): the stratified sums — annot[j, c] times the pair's term over
        the rows j within max_lag of every row and inside its window [lo[i], hi[i]] (uint32 arrays, both or neither)."""
        name = "storm_hip_lag_dosage_ldscore_annot_complete" if complete else "storm_hip_lag_dosage_ldscore_annot"
        n = self.n_rows
        a = np.ascontiguousarray(annot, dtype=np.float32)
        c = int(a.shape[1])
        lo = None if lo is None else np.ascontiguousarray(lo, dtype=np.uint32)
        hi = None if hi is None else np.ascontiguousarray(hi, dtype=np.uint32)
        score, pairs = np.zeros((max(n, 1), max(c, 1)), dtype=np.float32), np.zeros(max(n, 1), dtype=np.uint32)
        check(getattr(self._lib, name)(self.ctx._h, self._h, LDSCORE_STATS[stat], n_samples, max_lag,
                                       None if lo is None else _ptr(lo), None if hi is None else _ptr(hi), _ptr(a), max(c, 1), c,
                                       _ptr(score), max(c, 1), _ptr(pairs)), name)
        return score[:n, :c], pairs[:n]

    def lag_dosage_ldscore_annot_device(self, d_annot: int, annot_ld: int, n_annot: int, d_score: int, score_ld: int,
                                        d_n_pairs: Optional[int], max_lag: int, n_samples: int, stat: str = "r2",
                                        complete: bool = False, lo: Optional[np.ndarray] = None, hi: Optional[np.ndarray] = None) -> None:
        """Same, from annotations and into buffers in device memory (d_n_pairs may be None); lo / hi stay host arrays. The C
        call returns with its work queued and lo / hi still to be read; this wrapper owns their copies and waits."""
        name = "storm_hip_lag_dosage_ldscore_annot_complete_device" if complete else "storm_hip_lag_dosage_ldscore_annot_device"
        lo = None if lo is None else np.ascontiguousarray(lo, dtype=np.uint32)
        hi = None if hi is None else np.ascontiguousarray(hi, dtype=np.uint32)
        check(getattr(self._lib, name)(self.ctx._h, self._h, LDSCORE_STATS[stat], n_samples, max_lag,
                                       None if lo is None else _ptr(lo), None if hi is None else _ptr(hi), C.c_void_p(d_annot),
                                       annot_ld, n_annot, C.c_void_p(d_score), score_ld,
                                       None if d_n_pairs is None else C.c_void_p(d_n_pairs)), name)
        self.ctx.synchronize()   # (lo / hi are this call's own copies: they must outlive the upload)

    def lag_dosage_prune(self, min_r2: float, max_lag: int, n_samples: int, complete: bool = False, owner: bool = False,
                         lo: Optional[np.ndarray] = None, hi: Optional[np.ndarray] = None, order: Optional[np.ndarray] = None):
        """storm_hip_lag_dosage_prune[_complete]: keep [n_rows] uint8, or (keep, owner [n_rows] uint32): greedy pruning /
        clumping over the rows' r2 within max_lag (and within [lo, hi], host uint32 arrays, both or neither), walked in
        `order` (a host permutation; None: row order)."""
        name = "storm_hip_lag_dosage_prune_complete" if complete else "storm_hip_lag_dosage_prune"
        n = self.n_rows
        u32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint32)
        lo, hi, order = u32(lo), u32(hi), u32(order)
        keep, own = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(n, 1), dtype=np.uint32)
        check(getattr(self._lib, name)(self.ctx._h, self._h, n_samples, max_lag, float(min_r2), _ptr(lo), _ptr(hi), _ptr(order),
                                       _ptr(keep), _ptr(own) if owner else None), name)
        return (keep[:n], own[:n]) if owner else keep[:n]

    def lag_dosage_prune_device(self, d_keep: int, d_owner: Optional[int], min_r2: float, max_lag: int, n_samples: int,
                                complete: bool = False, lo: Optional[np.ndarray] = None, hi: Optional[np.ndarray] = None,
                                order: Optional[np.ndarray] = None) -> None:
        """Same, into buffers in device memory (d_owner may be None); lo / hi / order stay host arrays. The C call returns with
        its work queued and the host arrays still to be read; this wrapper owns their copies and waits."""
        name = "storm_hip_lag_dosage_prune_complete_device" if complete else "storm_hip_lag_dosage_prune_device"
        u32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint32)
        lo, hi, order = u32(lo), u32(hi), u32(order)
        check(getattr(self._lib, name)(self.ctx._h, self._h, n_samples, max_lag, float(min_r2), _ptr(lo), _ptr(hi), _ptr(order),
                                       C.c_void_p(d_keep), None if d_owner is None else C.c_void_p(d_owner)), name)
        self.ctx.synchronize()   # (lo / hi / order are this call's own copies: they must outlive the upload)

    def lag_dosage_corr_sparse(self, min_r2: float, max_lag: int, n_samples: int, complete: bool = False,
                               capacity: Optional[int] = None, lo: Optional[np.ndarray] = None, hi: Optional[np.ndarray] = None):
        """storm_hip_lag_dosage_corr_sparse[_complete]: (row_start [n_rows + 1] uint64, col uint32, val float32): the pairs
        within max_lag (and within [lo, hi], host uint32 arrays, both or neither) whose r2 is > min_r2, CSR over the forward
        pairs. capacity=None: the count-only call, then the exact fill (the band twice); else one call, and a RuntimeError
        naming the total where the capacity is too small."""
        name = "storm_hip_lag_dosage_corr_sparse_complete" if complete else "storm_hip_lag_dosage_corr_sparse"
        n = self.n_rows
        u32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint32)
        lo, hi = u32(lo), u32(hi)
        rows, total = np.zeros(n + 1, dtype=np.uint64), C.c_uint64(0)
        call = lambda c, v, cap: getattr(self._lib, name)(self.ctx._h, self._h, n_samples, max_lag, float(min_r2), _ptr(lo), _ptr(hi),
                                                          _ptr(rows), c, v, cap, C.byref(total))
        if capacity is None:
            check(call(None, None, 0), name)
            capacity = int(total.value)
        col, val = np.zeros(max(capacity, 1), dtype=np.uint32), np.zeros(max(capacity, 1), dtype=np.float32)
        check(call(_ptr(col), _ptr(val), int(capacity)), name)
        return rows, col[:int(total.value)], val[:int(total.value)]

    def lag_dosage_corr_sparse_device(self, d_row_start: int, d_col: Optional[int], d_val: Optional[int], capacity: int, min_r2: float,
                                      max_lag: int, n_samples: int, complete: bool = False, lo: Optional[np.ndarray] = None,
                                      hi: Optional[np.ndarray] = None, wait: bool = True) -> None:
        """Same, into buffers in device memory (d_col / d_val None with capacity 0: the offsets alone); only the first
        `capacity` pairs are written. lo / hi stay host arrays. The C call returns with its work queued and the host arrays
        still to be read; this wrapper owns their copies and waits (wait=False, without lo / hi only: queued on the
        context's stream)."""
        name = "storm_hip_lag_dosage_corr_sparse_complete_device" if complete else "storm_hip_lag_dosage_corr_sparse_device"
        u32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.uint32)
        lo, hi = u32(lo), u32(hi)
        dev = lambda p: None if p is None else C.c_void_p(p)
        check(getattr(self._lib, name)(self.ctx._h, self._h, n_samples, max_lag, float(min_r2), _ptr(lo), _ptr(hi), dev(d_row_start),
                                       dev(d_col), dev(d_val), capacity), name)
        if wait or lo is not None or hi is not None:
            self.ctx.synchronize()   # (lo / hi are this call's own copies: they must outlive the upload)

    def pairw_topk(self, k: int, score: str = "jaccard", n_bits: int = 1, panel_rows: int = 0):
        """(idx [n_rows, k] uint32, val [n_rows, k] float32, or uint32 for score "count"): for each row its k best other rows,
        value descending, then row index ascending; fewer than k candidates: idx 0xFFFFFFFF with val NaN (0 for "count")."""
        idx, val = _topk_out(self.n_rows, k, score)
        spare = np.zeros(1, np.uint32)
        check(self._lib.storm_hip_pairw_topk(self.ctx._h, self._h, SCORES[score], n_bits, k, panel_rows,
                                             _ptr(idx) if idx.size else _ptr(spare), _ptr(val) if val.size else _ptr(spare), k),
              "storm_hip_pairw_topk")
        return idx, val

    def pairw_topk_device(self, d_idx: int, d_val: int, ld_k: int, k: int, score: str = "jaccard", n_bits: int = 1,
                          panel_rows: int = 0) -> None:
        """Same, into device buffers (n_rows x ld_k 32-bit words each; columns [k, ld_k) are not touched); complete on return."""
        check(self._lib.storm_hip_pairw_topk_device(self.ctx._h, self._h, SCORES[score], n_bits, k, panel_rows, C.c_void_p(d_idx),
                                                    C.c_void_p(d_val), ld_k),
              "storm_hip_pairw_topk_device")

    def cross_topk(self, other: "HipMatrix", k: int, score: str = "jaccard", n_bits: int = 1, panel_rows: int = 0):
        """(idx, val) of [n_rows, k]: for each row of self its k best rows of other (equal row widths)."""
        idx, val = _topk_out(self.n_rows, k, score)
        spare = np.zeros(1, np.uint32)
        check(self._lib.storm_hip_cross_dense_topk(self.ctx._h, self._h, other._h, SCORES[score], n_bits, k, panel_rows,
                                                   _ptr(idx) if idx.size else _ptr(spare),
                                                   _ptr(val) if val.size else _ptr(spare), k),
              "storm_hip_cross_dense_topk")
        return idx, val

    def topk_rows_device(self, d_counts_matrix: int, ld: int, n_rows: int, n_cols: int, d_counts_rows: int, d_counts_cols: int,
                         d_idx: int, d_val: int, ld_k: int, k: int, score: str = "jaccard", n_bits: int = 1,
                         skip0: Optional[int] = None) -> None:
        """The selection alone over a complete count matrix of the caller's in device memory (storm_hip_topk_rows_device; the
        matrix only lends its context); asynchronous on the context's stream. skip0: row r never lists column skip0 + r."""
        check(self._lib.storm_hip_topk_rows_device(self.ctx._h, C.c_void_p(d_counts_matrix), ld, n_rows, n_cols,
                                                   C.c_void_p(d_counts_rows), C.c_void_p(d_counts_cols),
                                                   (1 << 64) - 1 if skip0 is None else skip0, SCORES[score], n_bits, k,
                                                   C.c_void_p(d_idx), C.c_void_p(d_val), ld_k),
              "storm_hip_topk_rows_device")

    def pairw_dosage_topk(self, n_samples: int, k: int, score: str = "r2", complete: bool = False, panel_rows: int = 0):
        """storm_hip_pairw_dosage_topk[_complete] on a dosage matrix: (idx [n_rows, k] uint32, val [n_rows, k] float32, or
        uint32 for score "dot"): for each row its k best other rows by r^2, r or the dot product."""
        name = "storm_hip_pairw_dosage_topk" + ("_complete" if complete else "")
        idx, val = _topk_out(self.n_rows, k, "count" if score == "dot" else score)
        spare = np.zeros(1, np.uint32)
        check(getattr(self._lib, name)(self.ctx._h, self._h, DOSAGE_SCORES[score], n_samples, k, panel_rows,
                                       _ptr(idx) if idx.size else _ptr(spare), _ptr(val) if val.size else _ptr(spare), k), name)
        return idx, val

    def cross_dosage_topk(self, other: "HipMatrix", n_samples: int, k: int, score: str = "r2", complete: bool = False,
                          panel_rows: int = 0):
        """storm_hip_square_dosage_topk[_complete]: (idx, val) of [n_rows, k]: for each row of self its k best rows of other."""
        name = "storm_hip_square_dosage_topk" + ("_complete" if complete else "")
        idx, val = _topk_out(self.n_rows, k, "count" if score == "dot" else score)
        spare = np.zeros(1, np.uint32)
        check(getattr(self._lib, name)(self.ctx._h, self._h, other._h, DOSAGE_SCORES[score], n_samples, k, panel_rows,
                                       _ptr(idx) if idx.size else _ptr(spare), _ptr(val) if val.size else _ptr(spare), k), name)
        return idx, val

    def dosage_topk_rows_device(self, d_dots: int, ld: int, n_rows: int, n_cols: int, d_sum_rows: int, d_sq_rows: int,
                                d_sum_cols: int, d_sq_cols: int, n_samples: int, d_idx: int, d_val: int, ld_k: int, k: int,
                                score: str = "r2", skip0: Optional[int] = None) -> None:
        """The selection alone over a complete panel of dot products of the caller's in device memory
        (storm_hip_dosage_topk_rows_device; the matrix only lends its context); asynchronous on the context's stream."""
        check(self._lib.storm_hip_dosage_topk_rows_device(self.ctx._h, C.c_void_p(d_dots), ld, n_rows, n_cols, C.c_void_p(d_sum_rows),
                                                          C.c_void_p(d_sq_rows), C.c_void_p(d_sum_cols), C.c_void_p(d_sq_cols),
                                                          n_samples, (1 << 64) - 1 if skip0 is None else skip0,
                                                          DOSAGE_SCORES[score], k, C.c_void_p(d_idx), C.c_void_p(d_val), ld_k),
              "storm_hip_dosage_topk_rows_device")

    def row_counts(self) -> np.ndarray:
        out = np.zeros(self.n_rows, dtype=np.uint32)
        check(self._lib.storm_hip_row_counts(self.ctx._h, self._h, _ptr(out)),
              "storm_hip_row_counts")
        return out

    def pairw_op(self, op: str) -> int:
        """sum_{i<j} popcount(row_i OP row_j), OP in and / or / xor."""
        total = C.c_uint64(0)
        check(self._lib.storm_hip_pairw_dense_op(self.ctx._h, self._h, self.OPS[op],
                                                 C.byref(total)), "storm_hip_pairw_dense_op")
        return int(total.value)

    def column_identity(self) -> int:
        out = C.c_uint64()
        check(self._lib.storm_hip_column_identity(self.ctx._h, self._h, C.byref(out)),
              "storm_hip_column_identity")
        return int(out.value)

    def close(self) -> None:
        if self._h:
            self._lib.storm_hip_matrix_destroy(self.ctx._h, self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
