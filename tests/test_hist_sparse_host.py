"""The counting rule of stage 2a's sparse lists ("hist_sparse", csrc/kernel_hllbs.cuh), restated in numpy on random rows: the values
below the set's threshold T from the dense decode, every value >= T from the two rows' sorted lists (the query row's histogram, then each
entry of the candidate row: not in the query list -> +1 at b; in it with b > a -> +1 at b, -1 at a) give the union histogram of
max(a, b) exactly.  No GPU."""
import numpy as np
import pytest

CAP = 128


def threshold(rows):
    """the smallest multiple of 4 (>= 4) at which every row holds at most CAP registers >= it; 28 = none up to 24"""
    for t in range(4, 28, 4):
        if int((rows >= t).sum(axis=1).max()) <= CAP:
            return t
    return 28


def sparse_list(row, t):
    idx = np.nonzero(row >= t)[0]
    return idx, row[idx].astype(np.int64)


def union_hist_sparse(a, b, t):
    m = np.maximum(a, b)
    hist = np.bincount(m[m < t], minlength=64)[:64].astype(np.int64)    # the dense groups [0, t / 4)
    ia, va = sparse_list(a, t)
    ib, vb = sparse_list(b, t)
    bins = np.bincount(va, minlength=64).astype(np.int64)               # hA
    pos = {int(r): k for k, r in enumerate(ia)}                         # the image of A: membership and rank
    for r, v in zip(ib, vb):
        k = pos.get(int(r))
        if k is None:
            bins[v] += 1
        elif v > va[k]:
            bins[v] += 1
            bins[va[k]] -= 1
    return hist + bins


def rows_like_sketches(rng, n, shift):
    """HLL-14-like registers: 1 + a geometric count of leading zeros, shifted by log2(cardinality / 2^14)"""
    return np.minimum(63, rng.geometric(0.5, size=(n, 16384)) + shift).astype(np.uint8)


@pytest.mark.parametrize("shift", [0, 2, 4, 8])
def test_sparse_rule_equals_union_histogram(shift):
    rng = np.random.default_rng(0x5EA5E + shift)
    rows = rows_like_sketches(rng, 8, shift)
    # similar pairs share most high registers: row 1 is row 0 with a few registers raised or lowered
    rows[1] = rows[0]
    sel = rng.choice(16384, 200, replace=False)
    rows[1, sel] = np.clip(rows[1, sel].astype(int) + rng.integers(-3, 4, 200), 0, 63)
    t = threshold(rows)
    assert 4 <= t <= 24
    for i in range(rows.shape[0]):
        for k in range(rows.shape[0]):
            want = np.bincount(np.maximum(rows[i], rows[k]), minlength=64)
            assert np.array_equal(union_hist_sparse(rows[i], rows[k], t), want), (shift, t, i, k)


def test_threshold_moves_at_the_cap():
    rng = np.random.default_rng(7)
    rows = np.minimum(rng.geometric(0.5, size=(3, 16384)) + 1, 10).astype(np.uint8)   # nothing >= 12
    rows[0, :CAP] = 12
    assert threshold(rows) == 12
    rows[0, CAP] = 13
    assert threshold(rows) == 16
    rows[1, :CAP + 1] = 30
    assert threshold(rows) == 28                                       # above 24: the set keeps the full decode
