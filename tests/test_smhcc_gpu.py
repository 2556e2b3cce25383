"""Criterion smh_c with its per-pair threshold for a minimum containment gamma (selhip_ctx_set_min_containment) on the GPU: a pair of
the pass's pair space survives stage 1 iff its equal buckets reach max(c_min, threshold(m, gamma, e_small, e_large)).  Expected records
and statistics come from tests/smhcc_model.py: the `none` ground truth under the pass's measure filtered by a numpy bucket count against
the numpy threshold.  Records are compared with == on (i, k, value bits), statistics with ==; tau = -1 makes every survivor with a
non-empty smaller genome a record."""
import gzip
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import containment_model as CM
import smhc_model as M
import smhcc_model as CC
from test_allpairs_topk_host import nbr_reference
from test_query_topk_host import topk_reference

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import (CRIT_NONE, CRIT_SMH_A, CRIT_SMH_C, FP_FMA, FP_STRICT, MODE_CB_SMH, MODE_SMH, PAIR_DTYPE, SelhipError,
                                         Selector)

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
FAST_M = (128, 256, 512, 1024)
GENERIC_M = (1, 3, 64, 100, 192)
G08 = CC.G08


def run_g(sel, gamma, c_min, tau, mode, rows=None):
    """one all-pairs pass under smh_c with the containment rule (c_min None: the selector's floor is left as it is -- never set in a
    fresh one); the band shape handed over is no factorisation of m: the criterion ignores it"""
    sel.set_criterion(CRIT_SMH_C)
    if c_min is not None:
        sel.set_min_matches(c_min)
    sel.set_min_containment(gamma)
    got = sel.run(tau, mode, 7, 3, rows=rows)
    return got, sel.stats()


def assert_pass(got, st, want, wst, what=""):
    assert M.tuples(got) == M.tuples(want), (what, len(got), len(want))
    assert st == wst, (what, st, wst)
    assert st["survivors"] == st["candidates"]


def assert_rule(sel, m, rule=1):
    assert sel.get_param("smhc_rule_used") == rule
    assert sel.get_param("smhc_path_used") == (1 if m in FAST_M else 0), m


def merged(parts):
    out = np.concatenate(parts) if parts else np.zeros(0, dtype=PAIR_DTYPE)
    return out[np.lexsort((out["k"], out["i"]))]


# ---- 1. shapes ---------------------------------------------------------------------------------------------------------------------
_TRUTH = {}


def shaped(oracle, n, m, tau=-1.0, use_cb=False, fp=FP_FMA, measure="jaccard", seed=0):
    """(hll, aux, cards, truth) of n pooled genomes (cardinalities spread over a wide range) with planted bucket groups; the HLL side of
    the truth is computed once per (n, tau, mode, flavour, measure) and shared"""
    hll, aux, cards = M.ranked(oracle, M.hll_pool(n), M.planted_groups(n, m, 1000 * m + n + seed), fp)
    key = (n, tau, use_cb, fp, measure)
    if key not in _TRUTH:
        _TRUTH[key] = CC.Truth(oracle, hll, np.zeros((n, 1), dtype=np.uint64), cards, tau, use_cb, fp, measure)
    t = CC.Truth.__new__(CC.Truth)
    t.none, t.E, t.cards = _TRUTH[key].none, _TRUTH[key].E, cards
    t.counts = M.match_counts(aux, aux)
    t.n, t.m = aux.shape
    return hll, aux, cards, t


@pytest.mark.parametrize("m", GENERIC_M + FAST_M)
def test_shapes(oracle, m):
    sizes = [1, 2, 3, 5, 25, 63, 64, 65, 129] + ([1030] if m == 128 else [])
    n_surv = 0
    with Selector(0) as sel, Selector(0) as floored:
        for n in sizes:
            hll, aux, cards, truth = shaped(oracle, n, m)
            sel.upload(hll, aux, cards)
            for gamma in (G08, 0.3):
                got, st = run_g(sel, gamma, None, -1.0, MODE_SMH)
                want, wst = truth.expected(gamma)
                print(f"m={m} n={n} gamma={gamma:.3f}: {st}")
                assert_pass(got, st, want, wst, what=(m, n, gamma))
                if n >= 2:
                    assert_rule(sel, m)
                if n >= 25 and m > 3 and gamma == G08:
                    assert 0 < wst["survivors"] < wst["evaluated"], (m, n, wst)          # a proper, non-empty subset
                n_surv += wst["survivors"]
            floored.upload(hll, aux, cards)
            c_min = max(1, m // 2)
            got, st = run_g(floored, 0.3, c_min, -1.0, MODE_SMH)
            assert_pass(got, st, *truth.expected(0.3, c_min), what=(m, n, "floor"))
    assert n_surv > 0
    # (n = 1030: the candidates cross a kChunk = 1024 boundary and the coarse thresholds of the two chunks' blocks differ)


@pytest.mark.parametrize("measure", ["jaccard", "max_containment"])
@pytest.mark.parametrize("fp", [FP_FMA, FP_STRICT])
def test_measures_and_flavours(oracle, measure, fp):
    n = 65
    with Selector(0, fp) as sel:
        sel.set_measure(measure)
        for m in (512, 100):
            hll, aux, cards, truth = shaped(oracle, n, m, fp=fp, measure=measure)
            sel.upload(hll, aux, cards)
            for gamma in (G08, 0.5):
                got, st = run_g(sel, gamma, None, -1.0, MODE_SMH)
                want, wst = truth.expected(gamma)
                assert_pass(got, st, want, wst, what=(measure, fp, m, gamma))
                assert len(want) > 0
            assert_rule(sel, m)


# ---- 2. the coarse test is a lower bound, the exact test decides -------------------------------------------------------------------
def doubling_cards(n, every, base=1000.0):
    """n ascending cardinalities that double every `every` ranks: a strong spread inside one chunk of candidates"""
    return base * np.power(2.0, np.arange(n) // every) + np.arange(n) % every


@pytest.mark.parametrize("m", [128, 512, 1024, 100])
def test_coarse_versus_exact(oracle, m):
    n, i = 160, 10
    cards = doubling_cards(n, 8)
    e = cards.astype(np.uint64)
    thr = CC.threshold(m, G08, e[i], e[i + 1:])                               # of (i, k), k = i + 1 ..: e_k >= e_i
    t_last = int(thr[-1])
    c = max(t_last, int(thr[0]) // 3)
    k_drop = i + 1 + int(np.nonzero(thr > c)[0].max())                       # the last candidate that still needs more than c
    k_keep = i + 1 + int(np.nonzero(thr <= c)[0].min())                      # the first one that does not
    assert k_drop > i and k_keep == k_drop + 1 < n
    assert t_last <= c < int(CC.threshold(m, G08, e[i], e[k_drop])) and int(CC.threshold(m, G08, e[i], e[k_keep])) <= c
    aux = CC.random_rows(n, m, 5 * m)
    CC.plant(aux, i, k_drop, c)
    CC.plant(aux, i, k_keep, c, salt=1)
    CC.plant(aux, i, i + 1, int(thr[0]), salt=2)                             # and one pair right on its (high) threshold
    hll = M.hll_pool(n)
    truth = CC.Truth(oracle, hll, aux, cards, -1.0, False)
    assert truth.counts[i, k_drop] == c and truth.counts[i, k_keep] == c
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        got, st = run_g(sel, G08, None, -1.0, MODE_SMH)
        want, wst = truth.expected(G08)
        assert_pass(got, st, want, wst, what=m)
        found = {(a, b) for a, b, _ in M.tuples(got)}
        assert (i, k_drop) not in found and (i, k_keep) in found and (i, i + 1) in found
        assert_rule(sel, m)
        # the same sketches as queries against themselves as the database: the cross pairs (x, y) with both orders of the cardinalities
        sel.upload_queries(hll[[i, k_drop, k_keep]], aux[[i, k_drop, k_keep]], cards[[i, k_drop, k_keep]])
        sel.set_criterion(CRIT_SMH_C)
        got = sel.run_queries(-1.0, MODE_SMH, 7, 3)
        found = {(int(a), int(b)) for a, b in zip(got["i"], got["k"])}
        assert (0, k_drop) not in found and (1, i) not in found and (0, k_keep) in found and (2, i) in found
        counts = M.match_counts(aux[[i, k_drop, k_keep]], aux)
        need = CC.needed(m, G08, None, cards[[i, k_drop, k_keep]], cards)
        assert found == {(int(a), int(b)) for a, b in zip(*np.nonzero(counts >= need))}


# ---- 3. boundary triples where the threshold steps ----------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [128, 256, 512, 1024, 100])
def test_boundary_triples(oracle, m):
    steps = [pr for a in (6500, 13000, 40000) for pr in CC.step_pairs(m, G08, [a], 2 * a, 40 * a)]      # (e_lo <= e_hi: b from 2 a on)
    assert len(steps) == 3
    pool = M.hll_pool(7)
    with Selector(0) as sel:
        for a, b in steps:
            t_b, t_b1 = int(CC.threshold(m, G08, a, b)), int(CC.threshold(m, G08, a, b + 1))
            assert t_b1 == t_b - 1 and 2 <= t_b1 and t_b + 1 <= m, (m, a, b, t_b)
            cards = np.array([a, b, b, b, b + 1, b + 1, b + 1], dtype=np.float64)
            shares = [t_b - 1, t_b, t_b + 1, t_b1 - 1, t_b1, t_b1 + 1]
            aux = CC.random_rows(7, m, m + a)
            for j, c in enumerate(shares):
                CC.plant(aux, 0, j + 1, c, salt=j)
            truth = CC.Truth(oracle, pool, aux, cards, -1.0, False)
            assert truth.counts[0, 1:].tolist() == shares
            sel.upload(pool, aux, cards)
            got, st = run_g(sel, G08, None, -1.0, MODE_SMH)
            assert_pass(got, st, *truth.expected(G08), what=(m, a, b))
            found = {(i, k) for i, k, _ in M.tuples(got)}
            assert [(0, j) in found for j in range(1, 7)] == [False, True, True, False, True, True], (m, a, b)
            # (shares[0] == shares[4]: the same count is dropped at b and kept at b + 1)


# ---- 4. the c_min floor, clearing ---------------------------------------------------------------------------------------------------
def test_c_min_floor_and_clear(oracle):
    n, m = 65, 256
    hll, aux, cards, truth = shaped(oracle, n, m)
    thr = CC.pair_thresholds(m, G08, cards, cards)[truth.E]
    lo, hi = int(thr.min()), int(thr.max())
    assert lo < hi <= m
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        seen = []
        for c_min in (1, max(1, lo - 1), (lo + hi) // 2, hi + 1, m):
            got, st = run_g(sel, G08, c_min, -1.0, MODE_SMH)
            assert_pass(got, st, *truth.expected(G08, c_min), what=c_min)
            seen.append(st["survivors"])
        assert seen[0] > seen[-1] and seen == sorted(seen, reverse=True)
        # gamma cleared: the fixed rule's records and kernel again
        for clear in (None, float("nan")):
            sel.set_min_containment(G08)
            sel.set_min_containment(clear)
            sel.set_min_matches(m // 2)
            got, st = sel.run(-1.0, MODE_SMH, 7, 3), sel.stats()
            assert_pass(got, st, *truth.expected(None, m // 2), what="cleared")
            assert_rule(sel, m, rule=0)
        for bad in (float("inf"), float("-inf")):
            with pytest.raises(SelhipError, match="min_containment"):
                sel.set_min_containment(bad)
        got, st = sel.run(-1.0, MODE_SMH, 7, 3), sel.stats()                  # the refused values left it cleared
        assert_pass(got, st, *truth.expected(None, m // 2), what="refused")


# ---- 5. empty rows, e = 0, equal cardinalities, gamma outside (0, 1] -----------------------------------------------------------------
@pytest.mark.parametrize("m", [256, 100])
def test_empty_and_degenerate(oracle, m):
    n = 30
    hll = M.hll_pool(n)
    aux = M.planted_groups(n, m, 5, shares=[1, m // 2, m - 1, m])
    aux[[3, 9, 20, 21, 22]] = M.EMPTY                          # empty SuperMinHash rows ...
    hll[[20, 21]] = 0                                          # ... two of them of genomes whose HLL sketch is empty too (e = 0)
    hll, aux, cards = M.ranked(oracle, hll, aux)
    assert np.all(cards[:2] == 0) and cards[2] > 0 and np.all(aux[:2] == M.EMPTY)
    truth = CC.Truth(oracle, hll, aux, cards, -1.0, False)
    cb = CC.Truth(oracle, hll, aux, cards, 0.2, True)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        for gamma in (G08, 0.3, 1.0):
            got, st = run_g(sel, gamma, None, -1.0, MODE_SMH)
            want, wst = truth.expected(gamma)
            assert_pass(got, st, want, wst, what=(m, gamma))
            assert not np.any(want["i"] < 2) and wst["survivors"] > 0        # a pair with an e = 0 rank never survives (threshold m + 1)
            got, st = run_g(sel, gamma, None, 0.2, MODE_CB_SMH)
            assert_pass(got, st, *cb.expected(gamma), what=("cb", m, gamma))
        # gamma <= 0: the threshold is 0 for every pair with a non-empty smaller genome -- all of the pair space but the e = 0 rows
        for gamma in (0.0, -1.0):
            got, st = run_g(sel, gamma, None, -1.0, MODE_SMH)
            want, wst = truth.expected(gamma)
            assert_pass(got, st, want, wst, what=(m, gamma))
            assert wst["survivors"] == (n - 2) * (n - 3) // 2 and wst["evaluated"] == wst["survivors"] + 2 * (n - 2)
    # equal cardinalities: the threshold is ceil(gamma m / (2 - gamma)) for every pair; gamma = 3 has den <= 0 there: nothing survives
    hll, aux, _ = M.ranked(oracle, M.hll_pool(n), M.planted_groups(n, m, 6, shares=[1, m // 2, m - 1, m]))
    cards = np.full(n, 13000.0)
    truth = CC.Truth(oracle, hll, aux, cards, -1.0, False)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        for gamma in (G08, 1.0, 3.0):
            got, st = run_g(sel, gamma, None, -1.0, MODE_SMH)
            want, wst = truth.expected(gamma)
            assert_pass(got, st, want, wst, what=("equal", m, gamma))
            assert (wst["survivors"] == 0) == (gamma == 3.0)


# ---- 6. CB windows, partitions, candidate begin, pipeline, overflow ------------------------------------------------------------------
def test_cb_windows_that_differ_inside_a_tile(oracle):
    n, m, tau = 300, 128, 0.9
    hll = M.hll_pool(n)
    hll[:3] = 0
    hll, aux, cards = M.ranked(oracle, hll, M.planted_groups(n, m, 77))
    e = cards.astype(np.int64).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        hi = np.array([np.max(np.nonzero((e == 0) | (e[i] / e >= np.float64(np.float32(tau))))[0]) for i in range(n)])
    assert any(len(set(hi[t:t + 12].tolist())) > 1 for t in range(0, n, 12))
    truth = CC.Truth(oracle, hll, aux, cards, tau, True)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        for gamma, c_min in ((G08, None), (0.95, None), (0.5, 100)):
            got, st = run_g(sel, gamma, c_min, tau, MODE_CB_SMH)
            want, wst = truth.expected(gamma, c_min)
            assert_pass(got, st, want, wst, what=(gamma, c_min))
            assert 0 < wst["survivors"] < wst["evaluated"]


@pytest.mark.parametrize("m", [256, 100])
def test_partitions_add_up(oracle, m):
    n, tau, gamma = 700, 0.3, 0.6
    hll, aux, cards, truth = shaped(oracle, n, m, tau, True)
    want, wst = truth.expected(gamma)
    assert 0 < len(want)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        parts, sts = [], []
        for rb, re in ((0, 1), (1, 130), (130, 130), (130, 699), (699, n)):
            got, st = run_g(sel, gamma, None, tau, MODE_CB_SMH, rows=(rb, re))
            assert_pass(got, st, *truth.expected(gamma, rows=(rb, re)), what=(rb, re))
            parts.append(got); sts.append(st)
        assert M.tuples(merged(parts)) == M.tuples(want)
        assert sum(s["survivors"] for s in sts) == wst["survivors"]
        parts, sts = [], []
        for part in range(3):
            sel.set_row_interleave(32, 3, part)
            got, st = run_g(sel, gamma, None, tau, MODE_CB_SMH)
            parts.append(got); sts.append(st)
        sel.set_row_interleave(32, 1, 0)
        assert M.tuples(merged(parts)) == M.tuples(want)
        assert sum(s["evaluated"] for s in sts) == wst["evaluated"] and sum(s["survivors"] for s in sts) == wst["survivors"]
        h = 333
        sel.set_candidate_begin(h)
        got, st = run_g(sel, gamma, None, tau, MODE_CB_SMH, rows=(0, h))
        sel.set_candidate_begin(0)
        assert_pass(got, st, *truth.expected(gamma, rows=(0, h), cand_begin=h), what="cand_begin")
        sel.set_pipeline(2)
        got, st = run_g(sel, gamma, None, tau, MODE_CB_SMH)
        assert sel.get_param("chunks") == 2
        assert_pass(got, st, want, wst, what="pipeline")


@pytest.mark.parametrize("m", [128, 100])
def test_survivor_list_overflow(oracle, m):
    n = 300
    aux = M.planted_groups(n, m, 9)
    aux[:, : m - m // 8] = aux[0, : m - m // 8]                # every pair shares seven eighths of its buckets: above every threshold
    hll, aux, cards = M.ranked(oracle, M.hll_pool(n), aux)
    truth = CC.Truth(oracle, hll, aux, cards, 0.3, False)
    want, wst = truth.expected(G08)
    assert wst["survivors"] == n * (n - 1) // 2
    with Selector(0) as sel:
        sel.set_param("init_cap", 1024)
        sel.upload(hll, aux, cards)
        got, st = run_g(sel, G08, None, 0.3, MODE_SMH)
        assert sel.last_attempts() > 1
        assert_pass(got, st, want, wst)


# ---- 7. query passes -----------------------------------------------------------------------------------------------------------------
_CROSS = {}


def query_case(oracle, n_q, n_d, m, tau, use_cb):
    pool = M.hll_pool(n_q + n_d)
    rows = M.planted_groups(n_q + n_d, m, 3 * m + n_q + n_d)
    pick = np.zeros(n_q + n_d, dtype=bool)
    pick[np.random.default_rng(n_q * 1000 + n_d).choice(n_q + n_d, n_q, replace=False)] = True
    Q, D = M.ranked(oracle, pool[pick], rows[pick]), M.ranked(oracle, pool[~pick], rows[~pick])
    key = (n_q, n_d, tau, use_cb)
    if key not in _CROSS:
        _CROSS[key] = M.cross_none(oracle, Q, D, tau, use_cb)
    return Q, D, _CROSS[key]


@pytest.mark.parametrize("n_q", [1, 5, 7])
def test_queries_equal_cross_pairs(oracle, n_q):
    n_rec, inside = 0, 0
    with Selector(0) as sel, Selector(0) as floored:
        for m in (128, 512, 100):
            for n_d in (1, 64, 65, 200):
                for mode in (MODE_CB_SMH, MODE_SMH):
                    tau = 0.3 if mode == MODE_CB_SMH else -1.0
                    Q, D, (none, E) = query_case(oracle, n_q, n_d, m, tau, mode == MODE_CB_SMH)
                    inside += int(np.count_nonzero((Q[2] > D[2][0]) & (Q[2] < D[2][-1])))      # queries whose threshold peaks inside the database
                    for s, gamma, c_min in ((sel, G08, None), (sel, 0.4, None), (floored, 0.4, max(1, m // 2))):
                        s.upload(D[0], D[1], D[2])
                        s.upload_queries(Q[0], Q[1], Q[2])
                        s.set_criterion(CRIT_SMH_C)
                        if c_min is not None:
                            s.set_min_matches(c_min)
                        s.set_min_containment(gamma)
                        got = s.run_queries(tau, mode, 7, 3)
                        want, wst = CC.cross_expected(none, E, Q, D, gamma, c_min)
                        assert_pass(got, s.stats(), want, wst, what=(n_q, n_d, m, mode, gamma, c_min))
                        assert_rule(s, m)
                        n_rec += len(want)
    assert n_rec > 0 and inside > 0


def test_queries_max_containment(oracle):
    n_q, n_d, m = 5, 64, 512
    Q, D, _ = query_case(oracle, n_q, n_d, m, -1.0, False)
    V = CM.values(CM.union_matrix(oracle, Q[0], D[0]), Q[2], D[2])["max_containment"]
    e_q, e_d = CM.trunc(Q[2])[:, None], CM.trunc(D[2])[None, :]
    E = np.maximum(e_q, e_d) != 0
    none = CM.select(V, E, -1.0)
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        sel.set_criterion(CRIT_SMH_C)
        sel.set_measure("max_containment")
        for gamma in (G08, 0.4):
            sel.set_min_containment(gamma)
            got = sel.run_queries(-1.0, MODE_SMH, 7, 3)
            want, wst = CC.cross_expected(none, E, Q, D, gamma)
            assert_pass(got, sel.stats(), want, wst, what=gamma)
            assert len(want) > 0


def test_top_ks(oracle):
    m = 128
    Q, D, (none, E) = query_case(oracle, 7, 200, m, -1.0, False)
    aux_d = D[1].copy()
    aux_d[:, : m - m // 8] = Q[1][0, : m - m // 8]             # every database row shares seven eighths of its buckets with query 0
    D2 = (D[0], aux_d, D[2])
    with Selector(0) as sel:
        sel.upload(*D2)
        sel.upload_queries(Q[0], Q[1], Q[2])
        sel.set_criterion(CRIT_SMH_C)
        sel.set_min_containment(G08)
        whole, _ = CC.cross_expected(none, E, Q, D2, G08)
        assert np.count_nonzero(whole["i"] == 0) == 200
        got = sel.run_queries(-1.0, MODE_SMH, 7, 3, top_k=3)
        assert M.tuples(got) == M.tuples(topk_reference(whole, 3))
        assert sel.stats()["selected"] == len(whole)
        sel.set_query_topk(0)
    n, m = 129, 256
    hll, aux, cards, truth = shaped(oracle, n, m)
    want, wst = truth.expected(0.4)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        sel.set_criterion(CRIT_SMH_C)
        sel.set_min_containment(0.4)
        got = sel.run(-1.0, MODE_SMH, 7, 3, top_k=2)
        assert M.tuples(got) == M.tuples(nbr_reference(want, 2)) and len(got) > 0
        assert sel.stats() == wst
        sel.set_allpairs_topk(0)


# ---- 8. pair lists ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [128, 1024, 100])
def test_pair_lists(oracle, m):
    n, tau = 129, 0.3
    hll, aux, cards, truth = shaped(oracle, n, m, tau, True)
    rng = np.random.default_rng(m)
    x = rng.integers(0, n, size=4000)
    y = rng.integers(0, n, size=4000)
    lst = np.stack([x, y], axis=1)[x != y].astype(np.int32)
    lst = np.concatenate([lst, lst[:300], lst[300:600, ::-1]])              # entries listed twice, in both orders
    lo, hi = lst.min(axis=1), lst.max(axis=1)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        sel.set_criterion(CRIT_SMH_C)
        for gamma, c_min in ((G08, None), (0.4, None), (0.4, max(1, m // 2))):
            all_pairs, _ = truth.expected(gamma, c_min)
            j_of = {(i, k): j for i, k, j in M.tuples(all_pairs)}
            want = sorted((int(a), int(b), j_of[(int(a), int(b))]) for a, b in zip(lo, hi) if (int(a), int(b)) in j_of)
            in_e = truth.E[lo, hi]
            need = CC.needed(m, gamma, c_min, cards, cards)
            surv = int(np.count_nonzero(in_e & (truth.counts[lo, hi] >= need[lo, hi])))
            if c_min is not None:
                sel.set_min_matches(c_min)
            sel.set_min_containment(gamma)
            got = sel.run_pairs(lst, tau, MODE_CB_SMH, 7, 3)
            assert M.tuples(got) == want, (m, gamma, c_min)
            assert sel.stats() == {"evaluated": int(in_e.sum()), "survivors": surv, "selected": len(want), "candidates": surv}
            assert len(want) > 0 and sel.get_param("smhc_rule_used") == 1
        for bad in ([[0, n]], [[-1, 2]], [[5, 5]]):
            with pytest.raises(SelhipError, match="invalid entries"):
                sel.run_pairs(np.array([[0, 1]] + bad, dtype=np.int32), tau, MODE_CB_SMH, 7, 3)


# ---- 9. isolation and refusals -------------------------------------------------------------------------------------------------------
def test_isolation_and_refusals(oracle):
    n, m, tau = 200, 256, 0.3
    hll, aux, cards, truth = shaped(oracle, n, m, tau, True)
    fixed = M.Truth(oracle, hll, aux, cards, tau, True)
    lst = np.array([[0, 1], [2, 3]], dtype=np.int32)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        sel.upload_queries(hll[:3], aux[:3], cards[:3])
        sel.set_criterion(CRIT_SMH_A)
        smh_before, smh_st = sel.run(tau, MODE_CB_SMH, 2, 128), sel.stats()
        sel.set_criterion(CRIT_NONE)
        none_before, none_st = sel.run(tau, MODE_CB_SMH, 1, 1), sel.stats()
        assert sel.get_param("smhc_rule_used") == -1
        sel.set_criterion(CRIT_SMH_C)
        runs = (lambda: sel.run(tau, MODE_CB_SMH, 1, 1), lambda: sel.run_queries(tau, MODE_CB_SMH, 1, 1), lambda: sel.run_pairs(lst, tau, MODE_CB_SMH, 1, 1))
        for run in runs:                                           # neither c_min nor gamma: refused, both setters named
            with pytest.raises(SelhipError, match="smh_c.*set_min_matches.*set_min_containment"):
                run()
        sel.set_min_containment(0.5)
        sel.set_min_containment(None)
        for run in runs:                                           # cleared is unset
            with pytest.raises(SelhipError, match="smh_c.*set_min_matches"):
                run()
        sel.set_min_containment(G08)
        sel.set_min_matches(m + 1)
        for run in runs:                                           # c_min > m is refused with gamma set too
            with pytest.raises(SelhipError, match="smh_c.*exceeds"):
                run()
        # the refusals claimed no counter set: the context is fully usable
        sel.set_criterion(CRIT_NONE)
        assert M.tuples(sel.run(tau, MODE_CB_SMH, 1, 1)) == M.tuples(none_before) and sel.stats() == none_st
        sel.set_min_matches(m // 2)
        got, st = run_g(sel, G08, None, tau, MODE_CB_SMH)
        assert_pass(got, st, *truth.expected(G08, m // 2), what="after refusals")
        # gamma is an option of smh_c alone: the other criteria and the fixed rule give their old records before and after
        sel.set_criterion(CRIT_SMH_A)
        assert M.tuples(sel.run(tau, MODE_CB_SMH, 2, 128)) == M.tuples(smh_before) and sel.stats() == smh_st
        sel.set_criterion(CRIT_NONE)
        assert M.tuples(sel.run(tau, MODE_CB_SMH, 1, 1)) == M.tuples(none_before) and sel.stats() == none_st
        sel.set_criterion(CRIT_SMH_C)
        sel.set_min_containment(None)
        for c_min in (1, m // 2, m):
            sel.set_min_matches(c_min)
            got, st = sel.run(tau, MODE_CB_SMH, 7, 3), sel.stats()
            assert_pass(got, st, *fixed.expected(c_min), what=("fixed", c_min))
            assert sel.get_param("smhc_rule_used") == 0
        # a pass pending: the setter answers SELHIP_E_STATE and changes nothing
        sel.run_async(tau, MODE_CB_SMH, 7, 3)
        with pytest.raises(SelhipError, match="pending") as err:
            sel.set_min_containment(0.1)
        assert err.value.code == -5                                 # SELHIP_E_STATE
        sel.finish()
        assert M.tuples(sel.fetch()) == M.tuples(fixed.expected(m)[0]) and sel.get_param("smhc_rule_used") == 0
        with pytest.raises(SelhipError):
            sel.set_criterion(6)


# ---- 10. the front ends on the influenza fixtures --------------------------------------------------------------------------------------
def selection(args, cwd=GOLDEN):
    out = subprocess.run([str(BIN / "selection")] + [str(a) for a in args], cwd=cwd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return out.stdout


@pytest.mark.parametrize("measure", ["jaccard", "max_containment"])
def test_front_ends_on_influenza(oracle, monkeypatch, tmp_path, measure):
    monkeypatch.chdir(GOLDEN)
    m, gamma = 512, 0.8
    ds = pkg.load_dataset("influenza_filelist.txt", m, 0, FP_FMA)
    truth = CC.Truth(oracle, ds.hll, ds.aux, ds.cards, -1.0, False, FP_FMA, measure)
    flags = ["-S", "max_containment"] if measure == "max_containment" else []
    kw = dict(mode=MODE_SMH, criterion="smh_c", measure=measure)
    base = ["-c", "smh_c", "-a", 8 * m, "-h", "-1", "-n"] + flags
    texts = {}
    for c_min in (None, 500):
        want, _ = truth.expected(gamma, c_min)
        text = pkg.format_lines(ds.names, want)
        extra = ["-C", c_min] if c_min else []
        assert selection(["-l", "influenza_filelist.txt", "-G", gamma] + extra + base) == text
        assert pkg.select_from_filelist("influenza_filelist.txt", -1.0, 8 * m, min_containment=gamma, min_matches=c_min, **kw) == text
        texts[c_min] = text
    union = texts[None]
    assert 0 < len(texts[500].splitlines()) < len(union.splitlines()) < 45
    # query passes: the cross pairs of the all-pairs output; pair lists: one run's output is the next run's list; the two top-ks
    names = [l.strip() for l in (GOLDEN / "influenza_filelist.txt").read_text().splitlines() if l.strip()]
    q_names, d_names = names[::3], [x for j, x in enumerate(names) if j % 3]
    (tmp_path / "q.txt").write_text("\n".join(q_names) + "\n")
    (tmp_path / "d.txt").write_text("\n".join(d_names) + "\n")
    q, d = str(tmp_path / "q.txt"), str(tmp_path / "d.txt")
    want = set()
    for line in union.splitlines():
        a, b, j = line.split(" ")
        if (a in q_names) != (b in q_names):
            want.add((a, b, j) if a in q_names else (b, a, j))
    got = selection(["-l", d, "-q", q, "-G", gamma] + base)
    assert {tuple(l.split(" ")) for l in got.splitlines()} == want and len(got.splitlines()) == len(want) > 0
    assert pkg.query_from_filelists(q, d, -1.0, 8 * m, min_containment=gamma, **kw) == got
    best = selection(["-l", d, "-q", q, "-k", 1, "-G", gamma] + base)
    assert best == pkg.query_from_filelists(q, d, -1.0, 8 * m, top_k=1, min_containment=gamma, **kw) and 0 < len(best.splitlines()) <= len(q_names)
    (tmp_path / "p.txt").write_text(selection(["-l", "influenza_filelist.txt", "-c", "none", "-h", "-1", "-n"] + flags))
    p = str(tmp_path / "p.txt")
    assert selection(["-l", "influenza_filelist.txt", "-p", p, "-G", gamma] + base) == union
    assert pkg.select_pairs_from_filelist("influenza_filelist.txt", p, -1.0, 8 * m, min_containment=gamma, **kw) == union
    nbr = selection(["-l", "influenza_filelist.txt", "-K", 1, "-G", gamma] + base)
    assert nbr == pkg.select_from_filelist("influenza_filelist.txt", -1.0, 8 * m, top_k=1, min_containment=gamma, **kw) and len(nbr.splitlines()) > 0


# ---- 11. real sequence: fragments of a genome inside the genome -------------------------------------------------------------------------
FRAGMENT_PARENTS = ("GCA_037915395.1_ASM3791539v1_genomic.fna.gz", "GCA_037919945.1_ASM3791994v1_genomic.fna.gz")


def test_fragments_of_real_genomes(tmp_path):
    """Two influenza A genomes (8 segments each) and, of each, a fragment file holding segments 1, 3, 5 and 7: J(fragment, parent) is
    about 0.53 -- far below any J threshold a prefilter tuned for J would be run at -- while the fragment lies in the parent whole.
    Margins, computed on the CPU from the reference's build_sketch files of these four inputs (m = 512; the GPU builder writes the same
    bits): equal buckets 274 and 267 against the thresholds 195 and 196 of gamma = 0.8 (sigma = sqrt(m J (1 - J)) = 11: 7.2 and 6.5
    sigma), below c_min = 410 = min_matches(512, 0.8) by 12 sigma; the HLL max containment of both pairs is 1.0000 against -h 0.8;
    smh_a's 64 bands of 8 rows hold no equal band for either pair."""
    work = tmp_path / "flu"
    work.mkdir()
    names, pairs = [], []
    for parent in FRAGMENT_PARENTS:
        src = GOLDEN / "influenza_fasta" / parent
        (work / parent).write_bytes(src.read_bytes())
        recs = [">" + r for r in gzip.open(src, "rt").read().split(">") if r.strip()]
        assert len(recs) == 8
        frag = parent.replace("_genomic", "_fragment")
        with gzip.open(work / frag, "wt") as f:
            f.write("".join(recs[0::2]))
        names += ["flu/" + parent, "flu/" + frag]
        pairs.append({"flu/" + parent, "flu/" + frag})
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    r = subprocess.run([str(BIN / "build_sketch"), "-l", "list.txt", "-t", "4", "-a", "4096", "-c", "smh_a"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    base = ["-l", "list.txt", "-n", "-S", "max_containment", "-h", "0.8", "-a", "4096"]

    def lines(args):
        return selection(base + args, cwd=tmp_path).splitlines()

    none = lines(["-c", "none"])
    contained = lines(["-c", "smh_c", "-G", "0.8"])
    fixed = lines(["-c", "smh_c", "-C", "410"])
    banded = lines(["-c", "smh_a"])
    print("none", none, "smh_c -G", contained, "smh_c -C", fixed, "smh_a", banded, sep="\n")

    def held(out):
        return [any({l.split(" ")[0], l.split(" ")[1]} == pr for l in out) for pr in pairs]

    assert held(none) == [True, True]
    assert held(contained) == [True, True] and set(contained) <= set(none)          # selected, with the records of the `none` pass
    for pr in pairs:
        (line,) = [l for l in contained if {l.split(" ")[0], l.split(" ")[1]} == pr]
        assert line in none and float(line.split(" ")[2]) >= 0.97                      # V = 1 +- 0.03 (HLL, p = 14)
    assert held(fixed) == [False, False] and held(banded) == [False, False]
