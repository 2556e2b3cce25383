"""The definition of the sparse adjacency (include/selection_hip.h section 2n) in numpy: what the device must produce, bit for bit."""
import numpy as np


def key(values):
    """key(J) of csrc/kernel_topk.cuh: a uint64 whose unsigned order is the IEEE total order of the float64 values"""
    bits = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    return np.where(bits >> np.uint64(63) != 0, ~bits, bits ^ np.uint64(1 << 63))


def csr(i, k, values, n_rows, symmetric, min_value=-np.inf):
    """(row_ptr int64 [n_rows + 1], col int32 [nnz], val float64 [nnz]) of the records {i, k, values}"""
    i, k, v = np.asarray(i, dtype=np.int64), np.asarray(k, dtype=np.int64), np.asarray(values, dtype=np.float64)
    take = v >= min_value                                                   # (a NaN value is never an entry)
    i, k, v = i[take], k[take], v[take]
    if symmetric:
        off = i != k
        i, k, v = np.concatenate([i, k[off]]), np.concatenate([k, i[off]]), np.concatenate([v, v[off]])
    order = np.lexsort((~key(v), k, i))                                     # row, column, key descending
    i, k, v = i[order], k[order], v[order]
    first = np.ones(len(i), dtype=bool)
    first[1:] = (i[1:] != i[:-1]) | (k[1:] != k[:-1])
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(i[first], minlength=n_rows))]).astype(np.int64)
    return row_ptr, k[first].astype(np.int32), v[first]
