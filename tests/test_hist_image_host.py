"""The clamped image of stage 2a ("hist_image", csrc/kernel_hllbs.cuh) restated in numpy: a genome's registers as four planes of
a' = min(a, 15) -- plane b < 4 of the image = p[b] | p[4] | p[5] of its six bit planes.  The union histogram of a pair is then
(the values below the set's sparse threshold T, decoded from the bit-serial maximum of the two IMAGE rows) + (every value >= T, from the
two rows' sparse lists of the full registers), and for T in {4, 8, 12} that is the byte-wise histogram of max(a, b) exactly.  For T = 16 it
is not: a 15 and a 16 both read 15 in the image, and 15 is below 16 -- which is why the image stops at 12.  No GPU."""
import numpy as np
import pytest

import bitplane_model as bm


def planes_of(row):
    """[6][16384] bits of a register row (values modulo 64)"""
    row = np.asarray(row, dtype=np.int64) & 63
    return np.stack([(row >> b) & 1 for b in range(6)])


def image_of(row):
    """the four planes of the clamped image, from the six planes alone (what hll_sparse_list_kernel writes)"""
    p = planes_of(row)
    return np.stack([p[b] | p[4] | p[5] for b in range(4)])


def bitserial_max(xa, yb):
    """bs_decode's maximum over NB planes: g = the borrow of b - a from the LSB (a > b), M_b = g ? A_b : B_b; the value per register"""
    g = np.zeros_like(xa[0])
    for a, b in zip(xa, yb):
        g = (a & ~b & 1) | (~(a ^ b) & 1 & g)
    m = [np.where(g == 1, a, b) for a, b in zip(xa, yb)]
    return sum(mb << b for b, mb in enumerate(m))


def sparse_part(a, b, t):
    """the counts of the values >= t from the two rows' lists: the query row's histogram, then each candidate entry (not in the query
    list: +1 at b; in it with b > a: +1 at b, -1 at a) -- bs_sparse_row / bs_sparse_entry"""
    a, b = np.asarray(a, dtype=np.int64) & 63, np.asarray(b, dtype=np.int64) & 63
    bins = np.bincount(a[a >= t], minlength=64).astype(np.int64)
    for r in np.nonzero(b >= t)[0]:
        if a[r] < t:
            bins[b[r]] += 1
        elif b[r] > a[r]:
            bins[b[r]] += 1
            bins[a[r]] -= 1
    return bins


def union_hist_image(a, b, t):
    m = bitserial_max(image_of(a), image_of(b))
    dense = np.bincount(m[m < t], minlength=64)[:64].astype(np.int64)
    return dense + sparse_part(a, b, t)


def random_rows(seed, shift):
    rng = np.random.default_rng([0x1A6E, seed])
    rows = np.minimum(63, rng.geometric(0.5, size=(6, 16384)) + shift).astype(np.uint8)
    rows[1] = rows[0]                                                   # a similar pair: a few registers raised or lowered
    sel = rng.choice(16384, 300, replace=False)
    rows[1, sel] = np.clip(rows[1, sel].astype(int) + rng.integers(-4, 5, 300), 0, 63)
    return rows


def adversarial_rows():
    """every value 0..63 against every value 0..63 (rows 0 and 1: 4 096 registers), and rows that sit on the clamp's boundaries"""
    a, b = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    rows = np.zeros((6, 16384), dtype=np.uint8)
    rows[0, :4096], rows[1, :4096] = a.ravel(), b.ravel()
    edge = np.array([11, 12, 15, 16, 17, 31, 32, 63])
    rows[2, :8], rows[3, 4:12] = edge, edge                             # alone in either row, and both at the same registers (4..7: unequal values)
    rows[4, :] = 15
    rows[5, :] = 16
    return rows


def test_image_is_the_clamp():
    for rows in (random_rows(0, 6), adversarial_rows()):
        for row in rows:
            img = image_of(row)
            assert np.array_equal(sum(img[b] << b for b in range(4)), np.minimum(row.astype(np.int64) & 63, 15))
    low = np.random.default_rng(3).integers(0, 16, 16384).astype(np.uint8)       # a four-plane row: the image is its planes
    assert np.array_equal(image_of(low), planes_of(low)[:4])


@pytest.mark.parametrize("t", [4, 8, 12])
@pytest.mark.parametrize("kind", ["random0", "random2", "random9", "adversarial"])
def test_image_plus_lists_equals_union_histogram(kind, t):
    rows = adversarial_rows() if kind == "adversarial" else random_rows(t, int(kind[6:]))
    for i in range(rows.shape[0]):
        for k in range(rows.shape[0]):
            got, want = union_hist_image(rows[i], rows[k], t), bm.union_hist(rows[i], rows[k])
            assert np.array_equal(got, want), (kind, t, i, k, np.nonzero(got != want)[0])


def test_sixteen_is_excluded():
    """T = 16: a register at 15 beside one at 16 -- the list takes the 16, and the image counts the clamped maximum 15 < T once more"""
    a, b = np.zeros(16384, dtype=np.uint8), np.zeros(16384, dtype=np.uint8)
    a[7], b[7] = 15, 16
    want = bm.union_hist(a, b)
    got = union_hist_image(a, b, 16)
    assert not np.array_equal(got, want)
    assert got[15] == want[15] + 1 and got[16] == want[16] == 1
    for t in (4, 8, 12):
        assert np.array_equal(union_hist_image(a, b, t), want)
