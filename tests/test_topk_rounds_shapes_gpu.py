"""The all-pairs top-k in row rounds (DESIGN.md sections 19, 41) at m = 32, 64 and m = 2048, 3072, whose rounds run the TOPK form of the
narrow / wide count kernel: list and statistics == the one-shot pass, nbr_reference of the numpy records and the same rounds under
"smhc_generic" = 1; the admitted count == the replay of topk_rounds_model.py; "smhc_kernel_used" names the kernel that ran."""
import functools

import pytest

import smhc_model as M
import smhv_model as V
import topk_rounds_model as R
from test_allpairs_topk_host import nbr_reference
from test_smhv_gpu import case, configure, tied_rows, zeros_hll
from test_topk_rounds_gpu import admitted, rounds_of

from cuda_selection_criteria_amd import MODE_SMH, TOPK_MAX, Selector

pytestmark = pytest.mark.gpu

KIND = {32: 2, 64: 2, 2048: 3, 3072: 3}                       # "smhc_kernel_used": 2 narrow (G = 4, 2), 3 wide (2 and 3 bucket chunks)
SHAPES = [(m, n) for m in sorted(KIND) for n in (2, 5, 66, 130, 257)] + [(2048, 1030)]


@functools.lru_cache(maxsize=None)
def tied(m, n):
    """(rows, cards, records of the one-shot pass, its statistics) under c_min = 1, tau = -1: every pair, ties on every level"""
    aux, cards = tied_rows(n, m, 3 * m + n), V.spread_cards(n)
    return (aux, cards) + V.expected(aux, cards, -1.0, False, "jaccard", c_min=1)


def in_rounds(sel, m, K, rows, tau=-1.0, generic=0):
    """(ranked list, statistics) of the pass in rounds, on the kernel of m or on the generic one"""
    sel.set_param("smhc_generic", generic)
    got = sel.run(tau, MODE_SMH, 7, 3, top_k=K, rounds=rows)
    sel.set_param("smhc_generic", 0)
    assert sel.get_param("smhc_kernel_used") == (0 if generic else KIND[m]) and sel.get_param("smhc_path_used") == 0, (m, K, rows, generic)
    return M.tuples(got), sel.stats()


@pytest.mark.parametrize("K", (1, 3, "n + 1"))
@pytest.mark.parametrize("m,n", SHAPES)
def test_shapes(m, n, K):
    K = min(n + 1, TOPK_MAX) if K == "n + 1" else K                  # (no cut; n = 1030: the largest K the library takes, five below a full list)
    aux, cards, S, wst = tied(m, n)
    with Selector(0) as sel:
        sel.upload(zeros_hll(n), aux, cards)
        configure(sel, c_min=1)
        sel.set_topk_rounds(0)
        whole = M.tuples(sel.run(-1.0, MODE_SMH, 7, 3, top_k=K))
        assert whole == M.tuples(nbr_reference(S, K)) and sel.stats() == wst
        for rows in (1, 5, 64, n + 7, "auto"):
            for generic in (0, 1):
                assert in_rounds(sel, m, K, rows, generic=generic) == (whole, wst), (rows, generic)
                assert sel.get_param("topk_rounds_used") == rounds_of(n, n, rows) and admitted(sel) <= len(S) == n * (n - 1) // 2


@pytest.mark.parametrize("m", [64, 2048])
def test_admitted_is_the_models(m):
    """the test a kernel that ignores thr fails: the narrow and the wide kernel append exactly the records the replay admits"""
    n = 257
    with Selector(0) as sel:
        for planted, (aux, cards) in ((True, case(n, m)), (False, tied(m, n)[:2])):
            sel.upload(zeros_hll(n), aux, cards)
            configure(sel, c_min=1)
            S, wst = V.expected(aux, cards, -1.0, False, "jaccard", c_min=1)
            for K, rows in ((1, 8), (1, 1), (3, 8), (2, 5)):
                ref, n_adm, per_round, _ = R.replay(S, n, K, rows)
                assert in_rounds(sel, m, K, rows) == (M.tuples(ref), wst), (planted, K, rows)
                assert admitted(sel) == n_adm and sel.get_param("topk_rounds_used") == len(per_round), (planted, K, rows)
                if planted and K == 1:                                  # (the model at K = 1: 628 and 509 of 692; at K = 2, 3 all of them)
                    assert 0 < n_adm < len(S) == wst["selected"], (K, rows)


@pytest.mark.parametrize("m", [32, 3072])
def test_rule_and_measure(m):
    """the -G rule with the maximum containment on cardinalities 1 : 100, and a fixed c_min > 1 with tau > -1, in rounds of 5 rows"""
    n, K = 130, 3
    with Selector(0) as sel:
        # (tied rows: every pair passes both rules and the rounds prune, 4 470 of 8 385 admitted; planted groups: the rules and tau cut)
        for aux in (tied_rows(n, m, 7 * m), M.planted_groups(n, m, 31 * m)):
            for cards, rule, measure, tau in ((V.spread_cards(n, ratio=100.0), dict(gamma=0.3, c_min=2), "max_containment", -1.0),
                                              (V.spread_cards(n), dict(c_min=max(2, m // 8)), "jaccard", 0.3)):
                sel.upload(zeros_hll(n), aux, cards)
                configure(sel, measure=measure, **rule)
                S, wst = V.expected(aux, cards, tau, False, measure, **rule)
                ref, n_adm, _, _ = R.replay(S, n, K, 5)
                assert M.tuples(ref) == M.tuples(nbr_reference(S, K)) and 0 < n_adm <= wst["selected"]
                for generic in (0, 1):
                    assert in_rounds(sel, m, K, 5, tau, generic) == (M.tuples(ref), wst), (rule, generic)
                    assert admitted(sel) == n_adm and sel.get_param("smhc_rule_used") == ("gamma" in rule)
