"""Stage 2a on the clamped image ("hist_image", csrc/kernel_hllbs.cuh): where a set's sparse threshold T is 4, 8 or 12 the all-pairs
bit-plane kernel reads four planes of min(register, 15) per row (8 KiB) instead of the set's five or six, and takes every value >= T from
the lists as before.  Every case runs the public pass on one context three ways -- the default (image), "hist_image" = 0 (the six-plane
rows) and "hist_sparse" = 0 (every value from the planes) -- and compares pairs, J bit for bit and the counters with each other and
with the oracle: registers on the clamp's boundaries (11, 12, 15, 16, 17, 31, 32, 63) in the query row, the candidate row and both, at
bit 0 and bit 31 of the first and the last dword of a plane; T = 4, 8, 12 and 16 (off); four-, five- and six-plane sets; the dense walk,
runs of 1 and 4; database replacements on a live context; two passes of one context."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import cuda_selection_criteria_amd as pkg  # noqa: E402
from cuda_selection_criteria_amd import MODE_SMH, Selector  # noqa: E402

import bitplane_model as bm  # noqa: E402
import test_hist_sparse_gpu as hs  # noqa: E402  (its forged rows: adversarial_rows)

M = 64
TAU = 0.05
EDGE = (11, 12, 15, 16, 17, 31, 32, 63)
# register 4 ((8 o + jj) 64 + lane) + s is bit 8 s + jj of plane dword 64 o + lane (hll_bitslice_kernel): bit 0 and bit 31 of the
# first and the last dword of a plane
CORNERS = [4 * ((8 * o + jj) * 64 + lane) + s for o, lane in ((0, 0), (7, 63)) for jj, s in ((0, 0), (7, 3))]


def boundary_rows(extra=0):
    """8 genomes that hold one EDGE value each at the four CORNERS (any two of them: both rows at the same registers, unequal values),
    one that holds them all at other registers, and 8 plain genomes of smaller and larger cardinality (so that ranked, the planted rows
    are query rows of some pairs and candidate rows of others).  Nothing else reaches 12: T = 12.  extra: registers >= 12 added to
    genome 8 on top of its 7 (122 -> 129 of them: T = 16)"""
    rng = np.random.default_rng(0x1A6E)
    base = np.minimum(rng.geometric(0.5, 16384) + 1, 11)                # ~256 registers >= 8, none >= 12
    rows = np.tile(base, (17, 1)).astype(np.int64)
    free = np.setdiff1d(np.arange(16384), CORNERS)
    for g in range(17):                                                 # similar genomes
        sel = rng.choice(free, 300, replace=False)
        rows[g, sel] = np.clip(rows[g, sel] + rng.integers(-2, 3, sel.size), 0, 11)
    for g, v in enumerate(EDGE):
        rows[g, CORNERS] = v
    other = rng.choice(free, 8 + extra, replace=False)
    rows[8, other[:8]] = EDGE
    rows[8, other[8:]] = rng.integers(12, 16, extra)
    for g in range(9, 13):                                              # smaller sketches
        rows[g, rng.choice(free, 1500, replace=False)] = 0
    for g in range(13, 17):                                             # larger ones
        sel = rng.choice(free, 1500, replace=False)
        rows[g, sel] = np.minimum(rows[g, sel] + 2, 11)
    return rows.astype(np.uint8)


def t8_rows():
    """the tiny recipe four values up: every register >= 4, only the planted ones (<= 128 per genome) reach 8"""
    return (hs.adversarial_rows("tiny") + 4).astype(np.uint8)


def five_plane_rows(n):
    rows = hs.adversarial_rows("plain", n=n, seed=0xAD5E + n)
    rows[1, 5], rows[n - 1, 9000] = 17, 31
    return rows


SETS = {
    "boundary": lambda: boundary_rows(),
    "boundary129": lambda: boundary_rows(122),
    "t4": lambda: hs.adversarial_rows("tiny"),
    "t8": t8_rows,
    "four_planes": lambda: hs.adversarial_rows("plain"),
    "six_planes": lambda: hs.adversarial_rows("six_planes"),
    "five_planes_24": lambda: five_plane_rows(24),
    "five_planes_40": lambda: five_plane_rows(40),
}


@functools.lru_cache(maxsize=None)
def case(oracle, name):
    """(hll ranked, aux, cards, the oracle's records, its stats) of a set, computed once"""
    hll, cards, perm = bm.rank_set(oracle, SETS[name]())
    aux = bm.aux_equal(hll.shape[0], M)                                 # every pair reaches stage 2
    r, b = pkg.banding(M, 0.5)
    want, st = oracle.select(hll, aux, cards, TAU, r, b, use_cb=False)
    n = hll.shape[0]
    assert n <= 48 and st["survivors"] == n * (n - 1) // 2 and len(want) > 0
    for a in (hll, aux, cards, want):
        a.setflags(write=False)
    return hll, aux, cards, want, st, perm


def one_pass(sel):
    r, b = pkg.banding(M, 0.5)
    got = sel.run(TAU, MODE_SMH, r, b)
    s = sel.stats()
    return got, (s["evaluated"], s["survivors"], s["selected"], s["candidates"]), sel.get_param("hist_image"), sel.get_param("hist_sparse_t")


def check_three_ways(sel, want, st, image_want, t_want):
    """the pass with the defaults, with "hist_image" = 0 and with "hist_sparse" = 0 (settings restored): each equal to the oracle"""
    runs = []
    for image, sparse in ((-1, 1), (0, 1), (-1, 0)):
        sel.set_param("hist_image", image)
        sel.set_param("hist_sparse", sparse)
        runs.append(one_pass(sel))
    sel.set_param("hist_image", -1)
    sel.set_param("hist_sparse", -1)
    assert [(u, t) for _, _, u, t in runs] == [(image_want, t_want), (0, t_want), (0, 0)], [(u, t) for _, _, u, t in runs]
    for got, stats, _, _ in runs:
        assert got.shape[0] == want.shape[0] and np.array_equal(got["i"], want["i"]) and np.array_equal(got["k"], want["k"])
        assert np.array_equal(got["jaccard"].view(np.uint64), want["jacc"].view(np.uint64))
        assert stats == runs[0][1] and stats[:2] == (st["evaluated"], st["survivors"])
    return runs[0][0]


def test_boundary_registers(oracle):
    hll, aux, cards, want, st, perm = case(oracle, "boundary")
    assert bm.khi(hll) == 64 and int((hll >= 12).sum(axis=1).max()) <= 128
    rank = np.argsort(perm)                                             # rank of every genome of boundary_rows
    assert rank[9:].min() < rank[:9].min() and rank[:9].max() < rank[9:].max()
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        check_three_ways(sel, want, st, 1, 12)


def test_one_register_more_switches_the_image_off(oracle):
    hll, aux, cards, want, st, _ = case(oracle, "boundary129")
    assert int((hll >= 12).sum(axis=1).max()) == 129
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        sel.set_param("hist_image", 1)                                  # forced: still only where it is exact
        got, _, used, t = one_pass(sel)
        assert (used, t) == (0, 16)
        assert np.array_equal(got["jaccard"].view(np.uint64), want["jacc"].view(np.uint64))
        check_three_ways(sel, want, st, 0, 16)


@pytest.mark.parametrize("name,t,planes", [("t4", 4, 4), ("t8", 8, 4), ("four_planes", 12, 4), ("five_planes_24", 12, 5), ("six_planes", 12, 6)])
def test_thresholds_and_plane_counts(oracle, name, t, planes):
    hll, aux, cards, want, st, _ = case(oracle, name)
    assert bm.planes(bm.khi(hll)) == planes and bm.sparse_t(hll, bm.khi(hll)) == t
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        check_three_ways(sel, want, st, 1, t)                           # (four planes: the image holds the planes' own bits)


@pytest.mark.parametrize("name", ["boundary", "six_planes"])
def test_walk_shapes(oracle, name):
    hll, aux, cards, want, st, _ = case(oracle, name)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        for degree, run in ((32, 0), (32, 1), (32, 4), (0, 0), (-1, 4)):   # the short list on one round of waves; the slice walk; no dense walk
            sel.set_param("hist_dense_degree", degree)
            sel.set_param("hist_run", run)
            for group in (True, False):
                sel.set_stage2_grouping(group)
                check_three_ways(sel, want, st, 1, 12)


def test_database_replacement(oracle):
    with Selector(0) as sel:
        for name, used, t in (("five_planes_24", 1, 12), ("boundary129", 0, 16), ("five_planes_40", 1, 12), ("t4", 1, 4)):
            hll, aux, cards, want, st, _ = case(oracle, name)
            sel.upload(hll, aux, cards)
            check_three_ways(sel, want, st, used, t)


def test_two_passes_identical_bytes(oracle):
    hll, aux, cards, want, _, _ = case(oracle, "six_planes")
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        first, s1, u1, _ = one_pass(sel)
        second, s2, u2, _ = one_pass(sel)
        assert u1 == u2 == 1 and s1 == s2 and first.tobytes() == second.tobytes() and len(first) == len(want)


def test_hist_image_param():
    with Selector(0) as sel:
        with pytest.raises(pkg.SelhipError):
            sel.set_param("hist_image", 2)
        assert sel.get_param("hist_image") == 0                         # no pass yet
