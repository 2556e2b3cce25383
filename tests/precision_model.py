"""Sketch sets at every main-sketch precision p_hll in 4..20, in plain numpy -- nothing here comes from the library under test.

A context whose sketches have p_hll != 14 builds no bit planes: stage 2 of its passes reads the byte rows through hll_union_hist_kernel
(csrc/kernel_hll.cuh), which has three bodies -- the unrolled one of 2^14 registers, one of 16-byte loads for 2^p >= 1024 (2^p / 1024
iterations) and a scalar one below that, down to 16 registers for the 64 lanes of a wave.  The generator makes VALID sketches of the
reference's precision-generic hll_t (hll.h: register = hash >> (64 - p); value = leading zeros of the other q = 64 - p bits, plus 1, at
most q + 1) and asserts it: no test feeds a register above q + 1.

PASS_PS with N, M, TAU and RB are what the pass tests of test_hll_precision_gpu.py run; test_hll_precision_host.py checks on the oracle
alone that these sets give every stage of a pass something to do at every one of those precisions."""
import functools

import numpy as np

from oracle_py import Oracle

ALL_PS = tuple(range(4, 21))
# 16, 64 and 512 registers (scalar body: fewer registers than lanes, as many, more), 1, 8, 32 and 1024 iterations of the 16-byte body
PASS_PS = (4, 6, 9, 10, 13, 15, 20)
N, M, TAU, RB = 48, 64, 0.5, (2, 32)
SEED = 137                              # (chosen so that every condition of test_hll_precision_host.py holds at every precision)
ITEMS_PER_REGISTER = 8
MAX_ITEMS = 200_000                     # per genome: keeps p = 20 under a second

_ORACLE = None


def oracle():
    global _ORACLE
    if _ORACLE is None:
        _ORACLE = Oracle()
    return _ORACLE


def bit_length(x):
    """exact bit length of every uint64 of x (0 for 0)"""
    x = np.array(x, dtype=np.uint64)
    out = np.zeros(x.shape, dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        hi = x >> np.uint64(s)
        big = hi != 0
        out += np.where(big, s, 0)
        x = np.where(big, hi, x)
    return out + (x != 0)


def registers(hashes, p):
    """the 2^p registers of an HLL sketch of precision p that holds these 64-bit hashes"""
    q = 64 - p
    hashes = np.asarray(hashes, dtype=np.uint64)
    idx = (hashes >> np.uint64(q)).astype(np.int64)
    rest = hashes & np.uint64((1 << q) - 1)
    rank = np.minimum(q - bit_length(rest) + 1, q + 1).astype(np.uint8)
    row = np.zeros(1 << p, dtype=np.uint8)
    np.maximum.at(row, idx, rank)
    assert int(row.max(initial=0)) <= q + 1
    return row


def genomes(p, n, m, seed):
    """(hash sets, SuperMinHash rows [n, m] u64) of n genomes in clusters of 2 to 6: a member keeps a share of the cluster's core
    hashes and core buckets -- 84 to 98 % (seven in ten members: near neighbours, J above 0.5 among themselves) or 50 to 78 % -- and fills
    up with hashes and buckets of its own; the clusters' sizes spread over a factor of 16, so the CB bound cuts pairs of different
    clusters"""
    rng = np.random.default_rng([seed, p, n, m])
    top = min(ITEMS_PER_REGISTER << p, MAX_ITEMS)
    sets, rows = [], []
    while len(sets) < n:
        size = min(int(rng.integers(2, 7)), n - len(sets))
        items = max(8, int(top * 2.0 ** rng.uniform(-4.0, 0.0)))
        core = rng.integers(0, 1 << 64, size=items, dtype=np.uint64)
        core_row = rng.integers(1, 1 << 62, size=m, dtype=np.uint64)
        for _ in range(size):
            share = rng.uniform(0.84, 0.98) if rng.random() < 0.7 else rng.uniform(0.5, 0.78)
            keep = rng.random(items) < share
            own = rng.integers(0, 1 << 64, size=int(items - keep.sum()), dtype=np.uint64)
            sets.append(np.concatenate([core[keep], own]))
            rows.append(np.where(rng.random(m) < share, core_row, rng.integers(1, 1 << 62, size=m, dtype=np.uint64)))
    return sets, np.stack(rows)


def rank_order(hll, p, fma=1):
    """(cards, perm): the oracle's report() of every row under flavour fma, and the order of the reference's std::sort on them"""
    orc = oracle()
    orc.set_fma(fma)
    try:
        cards = orc.cards(hll, p)
    finally:
        orc.set_fma(1)
    return cards, orc.std_sort_perm(cards)


def _frozen(*arrays):
    for a in arrays:
        a.flags.writeable = False
    return arrays


@functools.lru_cache(maxsize=None)
def sketch_set_aux(p, n, m, seed, p_aux=0, fma=1):
    """(hll u8 [n, 1 << p], aux u64 [n, m], cards f64 [n], aux_hll u8 [n, 1 << p_aux]) in ascending-card order; aux_hll are sketches of
    precision p_aux of the same genomes (p_aux = 0: an empty array).  Computed once per argument tuple, shared and read-only"""
    sets, aux = genomes(p, n, m, seed)
    hll = np.stack([registers(s, p) for s in sets])
    assert int(hll.max()) <= 64 - p + 1
    aux_hll = np.stack([registers(s, p_aux) for s in sets]) if p_aux else np.zeros((n, 0), dtype=np.uint8)
    cards, perm = rank_order(hll, p, fma)
    return _frozen(np.ascontiguousarray(hll[perm]), np.ascontiguousarray(aux[perm]), np.ascontiguousarray(cards[perm]),
                   np.ascontiguousarray(aux_hll[perm]))


def sketch_set(p, n, m, seed, fma=1):
    """(hll u8 [n, 1 << p], aux u64 [n, m], cards) in ascending-card order, the cards from Oracle.cards(hll, p)"""
    return sketch_set_aux(p, n, m, seed, 0, fma)[:3]


def pass_set(p, fma=1, p_aux=0):
    """the set the pass tests run at precision p: (hll, aux, cards, aux_hll)"""
    return sketch_set_aux(p, N, M, SEED, p_aux, fma)


def edge_rows(p, rng):
    """hand-made rows [5, 1 << p]: empty; saturated (every register q + 1: the estimate is +inf); one non-zero register; uniform over
    [0, q + 1] (at p = 4 that reaches bins up to 61); only the values q and q + 1"""
    q, nreg = 64 - p, 1 << p
    one = np.zeros(nreg, dtype=np.uint8)
    one[rng.integers(0, nreg)] = rng.integers(1, q + 2)
    rows = np.stack([np.zeros(nreg, dtype=np.uint8), np.full(nreg, q + 1, dtype=np.uint8), one,
                     rng.integers(0, q + 2, size=nreg).astype(np.uint8), rng.integers(q, q + 2, size=nreg).astype(np.uint8)])
    assert int(rows.max()) <= q + 1
    return rows


def union_hist(a, b):
    """the 64 bins of the register-wise maximum of two rows"""
    return np.bincount(np.maximum(a, b), minlength=64).astype(np.uint32)


def match_counts(aux):
    """[n, n] numbers of equal buckets of every pair of SuperMinHash rows"""
    return (aux[:, None, :] == aux[None, :, :]).sum(axis=2)


def pair_space(cards, tau, use_cb):
    """bool [n, n]: the pairs (i, k), i < k in rank order, an all-pairs pass evaluates: e_k != 0 and, with the CB bound,
    (double)e_i / (double)e_k >= (double)(float)tau on the truncated cardinalities"""
    e = np.asarray(cards, dtype=np.float64).astype(np.int64).astype(np.float64)
    n = len(e)
    E = np.triu(np.ones((n, n), dtype=bool), 1) & (e != 0)[None, :]
    if use_cb:
        with np.errstate(divide="ignore", invalid="ignore"):
            E &= (e[:, None] / e[None, :]) >= np.float64(np.float32(tau))
    return E


def smhc_threshold(orc, hll, aux, cards, p, tau, use_cb=False):
    """(c, all, kept) for the smh_c tests: `all` = the oracle's smh_a pass with bands of one bucket (a pair passes iff at least one
    bucket is equal: smh_c with c = 1), c = the median bucket count of its selected pairs, rounded up, and kept = the mask of the
    records whose count reaches c"""
    want, st = orc.select(hll, aux, cards, tau, 1, aux.shape[1], use_cb=use_cb, p=p)
    cnt = match_counts(aux)[want["i"], want["k"]]
    c = int(np.ceil(np.median(cnt))) if len(cnt) else 1
    return c, want, cnt >= c
