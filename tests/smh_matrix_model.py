"""The numpy model of the SuperMinHash matrix measures (include/selection_hip.h section 2f, SELHIP_MEASURE_SMH_MATCHES / _SMH_JACCARD) and
the planted bucket sets their tests use.  The cell of rows a and b is the number of positions at which the two u64 rows are equal; the
Jaccard measure is that count / m in float64."""
import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)            # every bucket of an empty sketch


def match_counts(A, B, chunk=64):
    """int64 [len(A), len(B)]: (A[:, None, :] == B[None, :, :]).sum(-1), in chunks of rows of A"""
    A, B = np.asarray(A, dtype=np.uint64), np.asarray(B, dtype=np.uint64)
    assert A.ndim == 2 and B.ndim == 2 and A.shape[1] == B.shape[1]
    out = np.empty((A.shape[0], B.shape[0]), dtype=np.int64)
    for a in range(0, A.shape[0], chunk):
        out[a:a + chunk] = (A[a:a + chunk, None, :] == B[None, :, :]).sum(-1)
    return out


def expected(A, B, measure="smh_matches", dtype=np.float64):
    """the matrix a call must return: the counts, or counts / m in float64, then cast to dtype"""
    c = match_counts(A, B).astype(np.float64)
    if measure == "smh_jaccard":
        c = c / np.float64(A.shape[1])
    else:
        assert measure == "smh_matches"
    return c.astype(dtype)


def random_rows(n, m, seed):
    """n rows of m buckets (high dword = the bucket index, as the sketches have it, low dword random) in which every row shares a
    random subset of its buckets with one common base row -- the subset's share drawn per row from 0 .. 1, so that the counts of the
    pairs spread over 0 .. m"""
    rng = np.random.default_rng(seed)
    hi = np.arange(m, dtype=np.uint64) << np.uint64(32)
    base = hi | rng.integers(0, 1 << 32, size=m, dtype=np.uint64)
    rows = hi[None, :] | rng.integers(0, 1 << 32, size=(n, m), dtype=np.uint64)
    share = rng.random(n)
    share[: min(n, 2)] = (1.0, 0.0)[: min(n, 2)]                 # one row equal to the base, one that shares nothing
    keep = rng.random((n, m)) < share[:, None]
    return np.where(keep, base[None, :], rows)


def planted_single(m, seed):
    """m + 1 rows: row j + 1 equals row 0 in bucket j ALONE -- row 0 of the matrix is all ones off the diagonal"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(1, 1 << 62, size=(m + 1, m), dtype=np.uint64)
    rows[1:] += (rows[1:] == rows[0][None, :]).astype(np.uint64)        # (no accidental equality with row 0)
    idx = np.arange(m)
    rows[idx + 1, idx] = rows[0, idx]
    return rows


def planted_all_but_one(m, seed):
    """m + 1 rows: row j + 1 equals row 0 everywhere EXCEPT bucket j -- row 0 of the matrix is m - 1 off the diagonal"""
    rng = np.random.default_rng(seed)
    base = rng.integers(1, 1 << 62, size=m, dtype=np.uint64)
    rows = np.tile(base, (m + 1, 1))
    idx = np.arange(m)
    rows[idx + 1, idx] = base ^ np.uint64(1)
    return rows


def half_equal(n, m, seed):
    """n rows of which row 0 is a base; odd rows differ from the base ONLY in the upper dword of every second bucket, even rows ONLY in
    the lower dword of every third bucket: each such bucket must count as unequal"""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 1 << 63, size=m, dtype=np.uint64)
    rows = np.tile(base, (n, 1))
    for g in range(1, n):
        if g & 1:
            rows[g, (g // 2) % 2::2] ^= np.uint64(g << 32)
        else:
            rows[g, (g // 2) % 3::3] ^= np.uint64(g)
    return rows
