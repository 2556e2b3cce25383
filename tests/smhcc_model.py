"""The model of criterion smh_c's per-pair threshold for a minimum containment gamma (include/selection_hip.h:
selhip_ctx_set_min_containment), in numpy float64 -- nothing here comes from the library under test.

    threshold(m, gamma, e_lo, e_hi) in [0, m + 1]:
        a = (double)e_lo, b = (double)e_hi
        a == 0                     -> m + 1
        num = (gamma * m) * a,  den = (a + b) - gamma * a        (numpy rounds every operation on its own)
        not den > 0                -> m + 1
        q = num / den;  q <= 0 -> 0,  q > m -> m + 1,  else ceil(q)

A pair of the pass's pair space survives stage 1 iff its bucket count c >= max(c_min if set else 0, threshold(m, gamma, min(e_i, e_k),
max(e_i, e_k))).  The expected records are the `none` ground truth under the pass's measure -- flat_oracle_select under J, the numpy
values of containment_model.py under max containment -- filtered by the count of smh_matrix_model.py against that threshold."""
import numpy as np

import containment_model as CM
import smhc_model as M
from smh_matrix_model import match_counts
from test_exhaustive_host import flat_oracle_select

from cuda_selection_criteria_amd import FP_FMA

G08 = float(np.float32(0.8))                        # (double)0.8f: what a float threshold of 0.8 is as a double


def threshold(m, gamma, e_lo, e_hi):
    """the rule above, broadcast over arrays; int64"""
    m_, g, a, b = np.broadcast_arrays(np.asarray(m, dtype=np.float64), np.asarray(gamma, dtype=np.float64),
                                      np.asarray(e_lo, dtype=np.uint64).astype(np.float64), np.asarray(e_hi, dtype=np.uint64).astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        num = (g * m_) * a
        den = (a + b) - g * a
        q = num / den
        none = (a == 0) | ~(den > 0) | (q > m_)
        t = np.where(none, m_ + 1, np.where(q <= 0, 0.0, np.ceil(np.where(none, 0.0, q))))
    return t.astype(np.int64)


def trunc_u64(cards):
    return np.asarray(cards, dtype=np.float64).astype(np.int64).astype(np.uint64)


def pair_thresholds(m, gamma, cards_r, cards_c):
    """int64 [n_r, n_c]: the threshold of every (row, column) pair"""
    e_r, e_c = trunc_u64(cards_r)[:, None], trunc_u64(cards_c)[None, :]
    return threshold(m, gamma, np.minimum(e_r, e_c), np.maximum(e_r, e_c))


def needed(m, gamma, c_min, cards_r, cards_c):
    """the count a pair needs: max(c_min or 0, its threshold)"""
    return np.maximum(pair_thresholds(m, gamma, cards_r, cards_c), int(c_min or 0))


class Truth:
    """the ground truth of one (sketch set, tau, mode, measure, FP flavour), computed once and shared by every (gamma, c_min) tested on it.
    measure "jaccard": the oracle's own exhaustive loop; "max_containment": containment_model's values on the oracle's unions (MODE_SMH)"""

    def __init__(self, oracle, hll, aux, cards, tau, use_cb, fp=FP_FMA, measure="jaccard"):
        self.n, self.m = aux.shape
        self.cards = cards
        self.counts = match_counts(aux, aux)
        self.E = M.pair_space(cards, tau, use_cb)
        if measure == "jaccard":
            self.none, st = flat_oracle_select(oracle, hll, cards, tau, use_cb, fp)
            assert int(self.E.sum()) == st["evaluated"]
        else:
            assert not use_cb
            V = CM.values(CM.union_matrix(oracle, hll, hll, fp, symmetric=True), cards, cards)["max_containment"]
            self.none = CM.select(V, self.E, tau)

    def expected(self, gamma, c_min=None, rows=None, cand_begin=0):
        """(records, statistics) of the pass over the rows [rows[0], rows[1]) and the candidates >= cand_begin"""
        need = needed(self.m, gamma, c_min, self.cards, self.cards) if gamma is not None else np.full((self.n, self.n), int(c_min))
        ok = self.counts >= need
        keep = ok[self.none["i"], self.none["k"]]
        E = self.E
        if rows is not None or cand_begin:
            rb, re = rows if rows is not None else (0, self.n)
            inside = np.zeros_like(E)
            inside[rb:re, cand_begin:] = True
            E = E & inside
            keep &= (self.none["i"] >= rb) & (self.none["i"] < re) & (self.none["k"] >= cand_begin)
        surv = int((E & ok).sum())
        rec = self.none[keep]
        return rec, {"evaluated": int(E.sum()), "survivors": surv, "selected": len(rec), "candidates": surv}


def cross_expected(none, E, Q, D, gamma, c_min=None):
    """(records, statistics) of the query pass: smhc_model.cross_none's records filtered by the count of (query row, database row)
    against the pair's needed count.  Q, D: (hll, aux, cards) in rank order"""
    counts = match_counts(Q[1], D[1])
    ok = counts >= needed(Q[1].shape[1], gamma, c_min, Q[2], D[2])
    rec = none[ok[none["i"], none["k"]]]
    surv = int((E & ok).sum())
    return rec, {"evaluated": int(E.sum()), "survivors": surv, "selected": len(rec), "candidates": surv}


def plant(aux, i, k, c, salt=0):
    """make rows i and k of aux share exactly c buckets, at positions spread over every 16-byte chunk of the row (rows of random
    buckets that share nothing before); row k is written"""
    m = aux.shape[1]
    pos = (M.spread_positions(m, c) + salt) % m
    aux[k, pos] = aux[i, pos]


def random_rows(n, m, seed):
    return np.random.default_rng(seed).integers(1, 1 << 62, size=(n, m), dtype=np.uint64)


def step_pairs(m, gamma, a_values, b_lo, b_hi):
    """(a, b) with threshold(a, b) > threshold(a, b + 1): the places where the threshold steps down between two neighbouring larger
    cardinalities, found by bisection on the (monotone) threshold; one per a"""
    out = []
    for a in a_values:
        lo, hi = int(b_lo), int(b_hi)
        t_lo, t_hi = int(threshold(m, gamma, a, lo)), int(threshold(m, gamma, a, hi))
        if t_lo == t_hi:
            continue
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if int(threshold(m, gamma, a, mid)) == t_lo:
                lo = mid
            else:
                hi = mid
        out.append((int(a), lo))
    return out
