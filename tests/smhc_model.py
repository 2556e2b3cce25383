"""The model of criterion smh_c (SELHIP_CRIT_SMH_C, include/selection_hip.h): a pair of the pass's pair space E survives stage 1 iff at
least c_min of its m SuperMinHash buckets are equal, and the survivors go to the unchanged HLL-Jaccard test.

The expected records are the `none` ground truth every exhaustive test uses -- flat_oracle_select of test_exhaustive_host.py, the
oracle's own loop -- filtered by the numpy bucket count of smh_matrix_model.py on the rank-ordered rows.  Independent of numpy, the
oracle's smh_a IS the count test at both ends: select(..., n_rows=1, n_bands=m) is c_min = 1 (some band of one bucket equal) and
select(..., n_rows=m, n_bands=1) is c_min = m (the one band of all buckets equal): oracle_ends."""
import numpy as np

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import FP_FMA, PAIR_DTYPE, SYNTH_CONFIGS
from smh_matrix_model import match_counts
from test_exhaustive_host import flat_oracle_select

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)            # every bucket of an empty SuperMinHash row


def ranked(oracle, hll, aux, fp=FP_FMA):
    """(hll, aux, cards) in rank order under the oracle's report() of flavour fp"""
    if hll.shape[0] == 0:
        return hll, aux, np.zeros(0, dtype=np.float64)
    oracle.set_fma(fp)
    try:
        cards = oracle.cards(hll)
    finally:
        oracle.set_fma(1)
    perm = pkg.sort_by_card(cards)
    return hll[perm], aux[perm], cards[perm]


_POOL = {}


def hll_pool(n, spread=True):
    """n HLL rows of the synthetic generator (spread: cardinalities over a range wide enough for the CB bound to cut)"""
    key = "cfg2-spread" if spread else "cfg2"
    if key not in _POOL or _POOL[key].shape[0] < n:
        cfg = SYNTH_CONFIGS[key].scaled(max(n, 1030))
        _POOL[key] = pkg.synth_host(cfg)[0]
    return _POOL[key][:n].copy()


def pair_space(cards, tau, use_cb):
    """bool [n, n]: the pairs (i, k), i < k in rank order, an all-pairs pass evaluates -- e_k != 0 and, with the CB bound,
    (double)e_i / (double)e_k >= (double)(float)tau"""
    e = np.asarray(cards, dtype=np.float64).astype(np.int64).astype(np.uint64)
    n = len(e)
    E = np.triu(np.ones((n, n), dtype=bool), 1) & (e != 0)[None, :]
    if use_cb:
        with np.errstate(divide="ignore", invalid="ignore"):
            E &= (e.astype(np.float64)[:, None] / e.astype(np.float64)[None, :]) >= np.float64(np.float32(tau))
    return E


class Truth:
    """the ground truth of one (sketch set, tau, mode, FP flavour): computed once, shared by every threshold tested on it"""

    def __init__(self, oracle, hll, aux, cards, tau, use_cb, fp=FP_FMA):
        self.none, self.st = flat_oracle_select(oracle, hll, cards, tau, use_cb, fp)
        self.counts = match_counts(aux, aux)
        self.E = pair_space(cards, tau, use_cb)
        assert int(self.E.sum()) == self.st["evaluated"]
        self.n, self.m = aux.shape

    def expected(self, c_min, rows=None, cand_begin=0):
        """(records, statistics) of the pass with this threshold over the rows [rows[0], rows[1]) and the candidates >= cand_begin"""
        keep = self.counts[self.none["i"], self.none["k"]] >= c_min
        E = self.E
        if rows is not None or cand_begin:
            rb, re = rows if rows is not None else (0, self.n)
            inside = np.zeros_like(E)
            inside[rb:re, cand_begin:] = True
            E = E & inside
            keep &= (self.none["i"] >= rb) & (self.none["i"] < re) & (self.none["k"] >= cand_begin)
        surv = int((E & (self.counts >= c_min)).sum())
        rec = self.none[keep]
        return rec, {"evaluated": int(E.sum()), "survivors": surv, "selected": len(rec), "candidates": surv}


def oracle_ends(oracle, hll, aux, cards, tau, use_cb, fp=FP_FMA):
    """{1: (records, statistics), m: (records, statistics)} straight from the oracle's smh_a, without numpy"""
    m = aux.shape[1]
    out = {}
    oracle.set_fma(fp)
    try:
        for c_min, (r, b) in ((1, (1, m)), (m, (m, 1))):
            pairs, st = oracle.select(hll, aux, cards, tau, r, b, use_cb=use_cb, criterion=0)
            rec = np.zeros(len(pairs), dtype=PAIR_DTYPE)
            rec["i"], rec["k"], rec["jaccard"] = pairs["i"], pairs["k"], pairs["jacc"]
            out[c_min] = (rec, {"evaluated": st["evaluated"], "survivors": st["survivors"], "selected": len(rec), "candidates": st["survivors"]})
    finally:
        oracle.set_fma(1)
    return out


def tuples(rec):
    """the records as (i, k, J bits) tuples, compared with =="""
    return list(zip(rec["i"].tolist(), rec["k"].tolist(), rec["jaccard"].view(np.uint64).tolist()))


def spread_positions(m, c):
    """c bucket positions spread evenly over [0, m): every 128-bucket chunk and every lane region gets its share"""
    return (np.arange(c, dtype=np.int64) * m) // max(c, 1)


def planted_groups(n, m, seed, shares=None):
    """n rows of m random buckets in groups of seven: the first row of a group is its base, the others share exactly `c` buckets with it
    at spread positions, c running through `shares` (default 1, m/2 - 1, m/2, m/2 + 1, m - 1, m, clipped to [0, m]).  The survivors of
    every threshold in (0, m] are a proper non-empty subset of the pairs as soon as n >= 2"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(1, 1 << 62, size=(n, m), dtype=np.uint64)
    if shares is None:
        shares = [1, m // 2 - 1, m // 2, m // 2 + 1, m - 1, m]
    shares = [min(max(int(c), 0), m) for c in shares]
    for g in range(n):
        base, j = g - g % 7, g % 7
        if j:
            pos = spread_positions(m, shares[(j - 1) % len(shares)])
            pos = (pos + g) % m                       # (a different phase per row: every bucket position is used by some group)
            rows[g, pos] = rows[base, pos]
    return rows


def boundary_triple_rows(m, c_min, seed):
    """four rows: a base and three that share c_min - 1, c_min and c_min + 1 buckets with it, the equal buckets spread over all chunks"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(1, 1 << 62, size=(4, m), dtype=np.uint64)
    for j, c in enumerate((c_min - 1, c_min, c_min + 1)):
        pos = spread_positions(m, min(max(c, 0), m))
        rows[j + 1, pos] = rows[0, pos]
    return rows


def cross_none(oracle, Q, D, tau, use_cb, fp=FP_FMA):
    """the HLL side of a query pass's ground truth, independent of the bucket rows: (records of the exhaustive all-pairs pass over Q u D
    cut to its cross pairs, as (query rank, database rank, J) sorted by (i, k); bool [n_q, n_d] pair space of the query pass).
    Q, D: (hll, aux, cards) in rank order"""
    n_q = Q[0].shape[0]
    hll = np.concatenate([Q[0], D[0]])
    cards = np.concatenate([Q[2], D[2]])
    perm = pkg.sort_by_card(cards)
    pairs, _ = flat_oracle_select(oracle, hll[perm], cards[perm], tau, use_cb, fp)
    g1, g2 = perm[pairs["i"]], perm[pairs["k"]]
    cross = (g1 < n_q) != (g2 < n_q)
    out = np.zeros(int(cross.sum()), dtype=PAIR_DTYPE)
    out["i"] = np.where(g1 < n_q, g1, g2)[cross]
    out["k"] = np.where(g1 < n_q, g2, g1)[cross] - n_q
    out["jaccard"] = pairs["jaccard"][cross]
    e_q = Q[2].astype(np.int64).astype(np.uint64)[:, None]
    e_d = D[2].astype(np.int64).astype(np.uint64)[None, :]
    e_lo, e_hi = np.minimum(e_q, e_d), np.maximum(e_q, e_d)
    E = e_hi != 0
    if use_cb:
        with np.errstate(divide="ignore", invalid="ignore"):
            E &= (e_lo.astype(np.float64) / e_hi.astype(np.float64)) >= np.float64(np.float32(tau))
    return out[np.lexsort((out["k"], out["i"]))], E


def cross_expected(none, E, Q_aux, D_aux, c_min):
    """(records, statistics) of the query pass under smh_c: cross_none's records filtered by the bucket count of (query row, database row)"""
    counts = match_counts(Q_aux, D_aux)
    rec = none[counts[none["i"], none["k"]] >= c_min]
    surv = int((E & (counts >= c_min)).sum())
    return rec, {"evaluated": int(E.sum()), "survivors": surv, "selected": len(rec), "candidates": surv}
