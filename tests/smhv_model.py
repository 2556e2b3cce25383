"""The model of the passes under SELHIP_ESTIMATOR_SMH (include/selection_hip.h: selhip_ctx_set_estimator), in numpy
float64 -- nothing here comes from the library under test.

    value(measure, m, c, e1, e2):
        "jaccard"           (double)c / (double)m
        "max_containment"   a = (double)min(e1, e2), b = (double)max(e1, e2);  ((double)c * (a + b)) / (((double)m + (double)c) * a)
                            min(e1, e2) == 0 -> NaN                               (numpy rounds every operation on its own)

A pass selects a pair iff it lies in the pass's pair space E, its bucket count c (smh_matrix_model.match_counts) reaches the pass's
count threshold -- max(1, c_min if set, smhcc_model.threshold(...) if gamma is set) -- and value >= (double)(float)tau.  Its record is
{i, k, value}.  stats: evaluated = |E|, survivors = candidates = the pairs of E that pass the count test, selected = the records.
No HLL register takes part: the cardinalities are given."""
import numpy as np

import smhcc_model as CC
from smh_matrix_model import match_counts

from cuda_selection_criteria_amd import PAIR_DTYPE


def trunc_u64(cards):
    return np.asarray(cards, dtype=np.float64).astype(np.int64).astype(np.uint64)


def value(measure, m, c, e1, e2):
    """float64, broadcast over arrays"""
    m_, c_, e1, e2 = np.broadcast_arrays(np.asarray(m, dtype=np.int64).astype(np.float64), np.asarray(c, dtype=np.int64).astype(np.float64),
                                         np.asarray(e1, dtype=np.uint64), np.asarray(e2, dtype=np.uint64))
    if measure == "jaccard":
        return c_ / m_
    assert measure == "max_containment"
    a, b = np.minimum(e1, e2).astype(np.float64), np.maximum(e1, e2).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (c_ * (a + b)) / ((m_ + c_) * a)
    return np.where(a == 0, np.nan, v)


def needed(m, cards_r, cards_c, c_min=None, gamma=None):
    """int64 [n_r, n_c]: the count a pair needs under the estimator -- never below 1"""
    need = np.full((len(cards_r), len(cards_c)), max(1, int(c_min or 0)), dtype=np.int64)
    if gamma is not None:
        need = np.maximum(need, CC.pair_thresholds(m, gamma, cards_r, cards_c))
    return need


def space_all(cards, tau, use_cb):
    """bool [n, n]: the pair space of an all-pairs pass (smhc_model.pair_space, restated)"""
    e = trunc_u64(cards)
    n = len(e)
    E = np.triu(np.ones((n, n), dtype=bool), 1) & (e != 0)[None, :]
    if use_cb:
        with np.errstate(divide="ignore", invalid="ignore"):
            E &= (e.astype(np.float64)[:, None] / e.astype(np.float64)[None, :]) >= np.float64(np.float32(tau))
    return E


def space_cross(cards_q, cards_d, tau, use_cb):
    """bool [n_q, n_d]: the pair space of a query pass"""
    e_q, e_d = trunc_u64(cards_q)[:, None], trunc_u64(cards_d)[None, :]
    lo, hi = np.minimum(e_q, e_d), np.maximum(e_q, e_d)
    E = hi != 0
    if use_cb:
        with np.errstate(divide="ignore", invalid="ignore"):
            E = E & ((lo.astype(np.float64) / hi.astype(np.float64)) >= np.float64(np.float32(tau)))
    return E


def _records(E, ok, V, tau):
    with np.errstate(invalid="ignore"):
        sel = E & ok & (V >= np.float64(np.float32(tau)))
    i, k = np.nonzero(sel)
    rec = np.zeros(len(i), dtype=PAIR_DTYPE)
    rec["i"], rec["k"], rec["jaccard"] = i, k, V[i, k]
    surv = int((E & ok).sum())
    return rec, {"evaluated": int(E.sum()), "survivors": surv, "selected": len(rec), "candidates": surv}


def expected(aux, cards, tau, use_cb=False, measure="jaccard", c_min=None, gamma=None, rows=None, cand_begin=0, counts=None):
    """(records sorted by (i, k), statistics) of an all-pairs pass over the rows [rows[0], rows[1]) and the candidates >= cand_begin.  counts: match_counts(aux, aux) when the caller has it already"""
    n, m = aux.shape
    e = trunc_u64(cards)
    if counts is None:
        counts = match_counts(aux, aux)
    E = space_all(cards, tau, use_cb)
    if rows is not None or cand_begin:
        rb, re = rows if rows is not None else (0, n)
        inside = np.zeros_like(E)
        inside[rb:re, cand_begin:] = True
        E = E & inside
    V = value(measure, m, counts, e[:, None], e[None, :])
    return _records(E, counts >= needed(m, cards, cards, c_min, gamma), V, tau)


def expected_cross(Q_aux, Q_cards, D_aux, D_cards, tau, use_cb=False, measure="jaccard", c_min=None, gamma=None):
    """the same of a query pass: records {query rank, database rank, value}"""
    m = Q_aux.shape[1]
    counts = match_counts(Q_aux, D_aux)
    E = space_cross(Q_cards, D_cards, tau, use_cb)
    V = value(measure, m, counts, trunc_u64(Q_cards)[:, None], trunc_u64(D_cards)[None, :])
    return _records(E, counts >= needed(m, Q_cards, D_cards, c_min, gamma), V, tau)


def expected_list(aux, cards, pairs, tau, use_cb=False, measure="jaccard", c_min=None, gamma=None):
    """the same of a pair-list pass over the (valid) entries `pairs` [P, 2]: one record {min, max, value} per selected ENTRY, sorted by
    (i, k); the statistics count entries"""
    n, m = aux.shape
    e = trunc_u64(cards)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    x, y = pairs.min(axis=1), pairs.max(axis=1)
    E = e[y] != 0
    if use_cb:
        with np.errstate(divide="ignore", invalid="ignore"):
            E = E & ((e[x].astype(np.float64) / e[y].astype(np.float64)) >= np.float64(np.float32(tau)))
    counts = (aux[x] == aux[y]).sum(-1).astype(np.int64)
    need = np.full(len(x), max(1, int(c_min or 0)), dtype=np.int64)
    if gamma is not None:
        need = np.maximum(need, CC.threshold(m, gamma, np.minimum(e[x], e[y]), np.maximum(e[x], e[y])))
    V = value(measure, m, counts, e[x], e[y])
    ok = counts >= need
    with np.errstate(invalid="ignore"):
        sel = E & ok & (V >= np.float64(np.float32(tau)))
    rec = np.zeros(int(sel.sum()), dtype=PAIR_DTYPE)
    rec["i"], rec["k"], rec["jaccard"] = x[sel], y[sel], V[sel]
    rec = rec[np.lexsort((rec["k"], rec["i"]))]
    surv = int((E & ok).sum())
    return rec, {"evaluated": int(E.sum()), "survivors": surv, "selected": len(rec), "candidates": surv}


def spread_cards(n, lo=2000.0, ratio=60.0):
    """n ascending cardinalities from lo to lo * ratio, with a few exact ties"""
    c = lo * np.power(ratio, np.arange(n) / max(n - 1, 1))
    c = np.floor(c)
    c[1::7] = c[0::7][: len(c[1::7])]                 # equal neighbours
    return np.sort(c)
