"""The reference of the sparse pair list tests: from a float band in the lag layout, the CSR list of the forward pairs whose
entry exceeds a threshold — row by row in plain numpy, written from the definition in storm.h (STORM_dosage_lag_corr_sparse)
and not from the kernels: no masks, no scan."""
import numpy as np


def sparse_list(band, n, max_lag, min_r2, lo=None, hi=None):
    """(row_start [n + 1] uint64, col uint32, val float32): pair (i, j = i + 1 + d) is listed when d < L = min(max_lag, n - 1),
    j < n, with windows j <= hi[i] and i >= lo[j], and band[i, d] > min_r2 as float32 (a NaN never is). col ascends within a
    row; val is band's own float."""
    band = np.asarray(band, dtype=np.float32)
    row_start = np.zeros(n + 1, dtype=np.uint64)
    cols, vals = [], []
    L = min(max_lag, n - 1) if n >= 2 else 0
    t = np.float32(min_r2)
    total = 0
    for i in range(n):
        width = min(L, n - 1 - i)
        j = i + 1 + np.arange(width, dtype=np.int64)
        entry = band[i, :width]
        with np.errstate(invalid="ignore"):
            listed = entry > t
        if lo is not None:
            listed &= (j <= int(hi[i])) & (i >= np.asarray(lo, dtype=np.int64)[j])
        cols.append(j[listed].astype(np.uint32))
        vals.append(entry[listed])
        total += int(listed.sum())
        row_start[i + 1] = total
    col = np.concatenate(cols) if cols else np.zeros(0, np.uint32)
    val = np.concatenate(vals) if vals else np.zeros(0, np.float32)
    return row_start, col.astype(np.uint32), val.astype(np.float32)


def symmetrised(row_start, col, n):
    """nb[i] = sorted rows adjacent to i in the list taken both ways round"""
    nb = [[] for _ in range(n)]
    for i in range(n):
        for j in col[int(row_start[i]):int(row_start[i + 1])]:
            nb[i].append(int(j))
            nb[int(j)].append(i)
    return [sorted(x) for x in nb]
