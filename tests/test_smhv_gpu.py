"""The smh_c passes under SELHIP_ESTIMATOR_SMH on the GPU (selhip_ctx_set_estimator): the count kernels emit the
records {i, k, V} themselves, V = smh_value(measure, m, c, e_i, e_k), and no HLL stage runs.  Expected records and statistics come from
tests/smhv_model.py -- numpy counts (smh_matrix_model), numpy thresholds (smhcc_model), the float64 expression of V -- never from the
library.  Records are compared with == on (i, k, value bits) sorted by (i, k), statistics with ==.  Unless a test is about them the
HLL rows uploaded are all zero and the cardinalities are given: nothing may depend on them."""
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import smhc_model as M
import smhcc_model as CC
import smhv_model as V
from test_allpairs_topk_host import nbr_reference
from test_query_topk_host import topk_reference

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import (CRIT_HLL_A, CRIT_NONE, CRIT_SMH_A, CRIT_SMH_C, MODE_CB_SMH, MODE_SMH, PAIR_DTYPE, SelhipError, Selector)

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
FAST_M = (128, 256, 512, 1024)
GENERIC_M = (64, 100)
SIZES = (1, 2, 3, 5, 13, 63, 64, 65, 129, 257)
G08 = CC.G08


def zeros_hll(n):
    return np.zeros((n, 1 << 14), dtype=np.uint8)


def case(n, m, seed=0):
    """(aux, cards) of n genomes in rank order: planted bucket groups, cardinalities spread over a factor 60 with ties"""
    return M.planted_groups(n, m, 1000 * m + n + seed), V.spread_cards(n)


def configure(sel, c_min=None, gamma=None, measure="jaccard", estimator="smh"):
    """(c_min is sticky and cannot be cleared: None sets 1, the floor of every pass under the estimator)"""
    sel.set_criterion(CRIT_SMH_C)
    sel.set_min_matches(1 if c_min is None else c_min)
    sel.set_min_containment(gamma)
    sel.set_measure(measure)
    sel.set_estimator(estimator)


def assert_pass(got, st, want, wst, what=""):
    assert M.tuples(got) == M.tuples(want), (what, len(got), len(want))
    assert st == wst, (what, st, wst)
    assert st["survivors"] == st["candidates"]


def merged(parts):
    out = np.concatenate(parts) if parts else np.zeros(0, dtype=PAIR_DTYPE)
    return out[np.lexsort((out["k"], out["i"]))]


# ---- 1. shapes: both kernel paths, tile / wave / block / chunk edges, both rules, both measures, the CB mode ---------------------------
@pytest.mark.parametrize("m", FAST_M + GENERIC_M)
def test_shapes(m):
    sizes = SIZES + ((1030,) if m == 128 else ())
    n_rec = 0
    with Selector(0) as sel:
        for n in sizes:
            aux, cards = case(n, m)
            counts = M.match_counts(aux, aux)
            sel.upload(zeros_hll(n), aux, cards)
            rules = [dict(c_min=1), dict(c_min=m // 2), dict(gamma=G08), dict(gamma=0.3, c_min=max(1, m // 8))]
            for rule in rules if n <= 257 else rules[1:3]:
                for measure, mode, tau in (("jaccard", MODE_SMH, 0.3), ("max_containment", MODE_SMH, 0.6), ("jaccard", MODE_CB_SMH, 0.3)):
                    configure(sel, measure=measure, **rule)
                    got, st = sel.run(tau, mode, 7, 3), sel.stats()
                    want, wst = V.expected(aux, cards, tau, mode == MODE_CB_SMH, measure, counts=counts, **rule)
                    assert_pass(got, st, want, wst, what=(m, n, rule, measure, mode))
                    n_rec += len(want)
                    if n >= 2:
                        assert sel.get_param("smhc_path_used") == (1 if m in FAST_M else 0)
                        assert sel.get_param("smhc_rule_used") == (1 if "gamma" in rule else 0)
            if n >= 63:
                want, wst = V.expected(aux, cards, 0.3, False, "jaccard", c_min=1, counts=counts)
                assert 0 < wst["selected"] < wst["survivors"] < wst["evaluated"], (m, n, wst)      # every test of the three bites
    assert n_rec > 0


# ---- 2. the tau boundary -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", FAST_M + GENERIC_M)
def test_tau_boundary_jaccard(m):
    with Selector(0) as sel:
        for tau in (0.25, 0.5, 0.75):
            c = int(tau * m)
            assert c == tau * m and float(np.float32(tau)) == tau
            aux = CC.random_rows(4, m, m + c)
            for j, share in enumerate((c - 1, c, c + 1)):
                CC.plant(aux, 0, j + 1, share, salt=j)
            cards = np.full(4, 10000.0)
            sel.upload(zeros_hll(4), aux, cards)
            configure(sel, c_min=1)
            got, st = sel.run(tau, MODE_SMH, 7, 3), sel.stats()
            want, wst = V.expected(aux, cards, tau, False, "jaccard", c_min=1)
            assert_pass(got, st, want, wst, what=(m, tau))
            assert [(0, k) in {(int(a), int(b)) for a, b in zip(got["i"], got["k"])} for k in (1, 2, 3)] == [False, True, True]
            assert got["jaccard"][0] == tau and got["i"][0] == 0 and got["k"][0] == 2


@pytest.mark.parametrize("m", FAST_M + (96,))
def test_tau_boundary_containment(m):
    """e = 4000 and 5000, c = m / 2: V = (c * 9000) / ((m + c) * 4000) = 0.75 exactly (m = 96: equal cardinalities, c = 32, V = 0.5)"""
    a, b, c, tau = (4000.0, 5000.0, m // 2, 0.75) if m != 96 else (7000.0, 7000.0, 32, 0.5)
    e = np.array([a, b], dtype=np.uint64)
    assert V.value("max_containment", m, c, e[0], e[1]) == tau > V.value("max_containment", m, c - 1, e[0], e[1])
    aux = CC.random_rows(4, m, 7 * m)
    for j, share in enumerate((c - 1, c, c + 1)):
        CC.plant(aux, 0, j + 1, share, salt=j)
    cards = np.array([a, b, b, b])
    with Selector(0) as sel:
        sel.upload(zeros_hll(4), aux, cards)
        for rule in (dict(c_min=1), dict(gamma=0.3)):
            configure(sel, measure="max_containment", **rule)
            got, st = sel.run(tau, MODE_SMH, 7, 3), sel.stats()
            want, wst = V.expected(aux, cards, tau, False, "max_containment", **rule)
            assert_pass(got, st, want, wst, what=(m, rule))
            assert [(int(x), int(y)) for x, y in zip(got["i"], got["k"]) if x == 0] == [(0, 2), (0, 3)] and got["jaccard"][0] == tau
        # the same pair as a query against the database, and as list entries in both orders
        sel.upload_queries(zeros_hll(1), aux[:1], cards[:1])
        configure(sel, c_min=1, measure="max_containment")
        got = sel.run_queries(tau, MODE_SMH, 7, 3)
        assert_pass(got, sel.stats(), *V.expected_cross(aux[:1], cards[:1], aux, cards, tau, False, "max_containment", c_min=1), what="query")
        assert [(int(x), int(y)) for x, y in zip(got["i"], got["k"])] == [(0, 0), (0, 2), (0, 3)]
        lst = np.array([[0, 1], [2, 0], [0, 3], [3, 0]], dtype=np.int32)
        got = sel.run_pairs(lst, tau, MODE_SMH, 7, 3)
        assert_pass(got, sel.stats(), *V.expected_list(aux, cards, lst, tau, False, "max_containment", c_min=1), what="list")
        assert len(got) == 3


def test_count_floor_is_one():
    """gamma <= 0 asks for 0 equal buckets and c_min was never set: a pair without an equal bucket still has no record"""
    n, m = 65, 128
    aux, cards = case(n, m)
    with Selector(0) as sel:
        sel.upload(zeros_hll(n), aux, cards)
        sel.upload_queries(zeros_hll(5), aux[:5], cards[:5])
        sel.set_criterion(CRIT_SMH_C)
        sel.set_min_containment(-1.0)
        sel.set_estimator("smh")
        lst = np.stack(np.triu_indices(n, 1), axis=1).astype(np.int32)
        for measure in ("jaccard", "max_containment"):
            sel.set_measure(measure)
            want, wst = V.expected(aux, cards, -1.0, False, measure, gamma=-1.0)
            assert 0 < wst["selected"] == wst["survivors"] < wst["evaluated"]
            assert_pass(sel.run(-1.0, MODE_SMH, 7, 3), sel.stats(), want, wst, what=measure)
            assert_pass(sel.run_pairs(lst, -1.0, MODE_SMH, 7, 3), sel.stats(), want, wst, what=(measure, "list"))
            assert_pass(sel.run_queries(-1.0, MODE_SMH, 7, 3), sel.stats(), *V.expected_cross(aux[:5], cards[:5], aux, cards, -1.0, False, measure, gamma=-1.0),
                        what=(measure, "query"))


# ---- 3. no HLL dependence -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [256, 100])
def test_no_hll_dependence(oracle, m):
    n = 129
    hll, aux, cards = M.ranked(oracle, M.hll_pool(n), M.planted_groups(n, m, 31 * m))
    lst = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1).astype(np.int32)
    out = []
    for rows in (hll, zeros_hll(n)):
        with Selector(0) as sel:
            sel.upload(rows, aux, cards)
            sel.upload_queries(rows[:7], aux[:7], cards[:7])
            configure(sel, gamma=0.3, c_min=2, measure="max_containment")
            res = [(M.tuples(sel.run(0.5, MODE_SMH, 7, 3)), sel.stats())]
            res.append((M.tuples(sel.run_queries(0.5, MODE_SMH, 7, 3)), sel.stats()))
            res.append((M.tuples(sel.run_pairs(lst, 0.5, MODE_SMH, 7, 3)), sel.stats()))
            out.append(res)
    assert out[0] == out[1]
    want, wst = V.expected(aux, cards, 0.5, False, "max_containment", c_min=2, gamma=0.3)
    assert out[0][0] == (M.tuples(want), wst) and len(want) > 0


# ---- 4. partitions, overflow --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [256, 100])
def test_partitions_add_up(m):
    n, tau, c_min = 700, 0.3, 1
    aux, cards = case(n, m)
    counts = M.match_counts(aux, aux)
    want, wst = V.expected(aux, cards, tau, True, "jaccard", c_min=c_min, counts=counts)
    assert 0 < len(want) < wst["survivors"]
    with Selector(0) as sel:
        sel.upload(zeros_hll(n), aux, cards)
        configure(sel, c_min=c_min)
        parts, sts = [], []
        for rb, re in ((0, 1), (1, 130), (130, 130), (130, 699), (699, n)):
            got, st = sel.run(tau, MODE_CB_SMH, 7, 3, rows=(rb, re)), sel.stats()
            assert_pass(got, st, *V.expected(aux, cards, tau, True, "jaccard", c_min=c_min, rows=(rb, re), counts=counts), what=(rb, re))
            parts.append(got); sts.append(st)
        assert M.tuples(merged(parts)) == M.tuples(want)
        assert all(sum(s[key] for s in sts) == wst[key] for key in ("evaluated", "survivors", "selected"))
        parts, sts = [], []
        for part in range(3):
            sel.set_row_interleave(32, 3, part)
            parts.append(sel.run(tau, MODE_CB_SMH, 7, 3)); sts.append(sel.stats())
        sel.set_row_interleave(32, 1, 0)
        assert M.tuples(merged(parts)) == M.tuples(want)
        assert all(sum(s[key] for s in sts) == wst[key] for key in ("evaluated", "survivors", "selected"))
        h = 333
        sel.set_candidate_begin(h)
        got, st = sel.run(tau, MODE_CB_SMH, 7, 3, rows=(0, h)), sel.stats()
        sel.set_candidate_begin(0)
        assert_pass(got, st, *V.expected(aux, cards, tau, True, "jaccard", c_min=c_min, rows=(0, h), cand_begin=h, counts=counts), what="cand_begin")
        sel.set_pipeline(2)
        got, st = sel.run(tau, MODE_CB_SMH, 7, 3), sel.stats()
        assert sel.get_param("chunks") == 2
        assert_pass(got, st, want, wst, what="pipeline")


@pytest.mark.parametrize("m", [128, 100])
def test_result_list_overflow(m):
    n = 300
    aux, cards = case(n, m)
    aux[:, : m // 2] = aux[0, : m // 2]                        # every pair shares half its buckets
    want, wst = V.expected(aux, cards, 0.5, False, "jaccard", c_min=m // 2)
    assert wst["selected"] == wst["survivors"] == n * (n - 1) // 2
    lst = np.stack(np.triu_indices(n, 1), axis=1).astype(np.int32)
    with Selector(0) as sel:
        sel.set_param("init_cap", 1024)
        sel.upload(zeros_hll(n), aux, cards)
        configure(sel, c_min=m // 2)
        got, st = sel.run(0.5, MODE_SMH, 7, 3), sel.stats()
        assert sel.last_attempts() > 1
        assert_pass(got, st, want, wst)
    with Selector(0) as sel:
        sel.set_param("init_cap", 1024)
        sel.upload(zeros_hll(n), aux, cards)
        sel.upload_queries(zeros_hll(65), aux[:65], cards[:65])
        configure(sel, c_min=m // 2)
        got, st = sel.run_queries(0.5, MODE_SMH, 7, 3), sel.stats()
        assert sel.last_attempts() > 1
        assert_pass(got, st, *V.expected_cross(aux[:65], cards[:65], aux, cards, 0.5, False, "jaccard", c_min=m // 2), what="query")
    with Selector(0) as sel:
        sel.set_param("init_cap", 1024)
        sel.upload(zeros_hll(n), aux, cards)
        configure(sel, c_min=m // 2)
        got, st = sel.run_pairs(lst, 0.5, MODE_SMH, 7, 3), sel.stats()
        assert sel.last_attempts() > 1
        assert_pass(got, st, *V.expected_list(aux, cards, lst, 0.5, False, "jaccard", c_min=m // 2), what="list")


# ---- 5. query passes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q", [1, 7, 64, 65])
def test_queries(n_q):
    n_rec = 0
    with Selector(0) as sel:
        for m in (128, 512, 1024, 100):
            for n_d in (1, 65, 200):
                rows = M.planted_groups(n_q + n_d, m, 3 * m + n_q + n_d)
                cards_all = V.spread_cards(n_q + n_d)
                pick = np.zeros(n_q + n_d, dtype=bool)
                pick[np.random.default_rng(n_q * 1000 + n_d).choice(n_q + n_d, n_q, replace=False)] = True
                Qa, Qc, Da, Dc = rows[pick], cards_all[pick], rows[~pick], cards_all[~pick]
                sel.upload(zeros_hll(n_d), Da, Dc)
                sel.upload_queries(zeros_hll(n_q), Qa, Qc)
                for rule, measure, mode, tau in ((dict(c_min=1), "jaccard", MODE_CB_SMH, 0.3), (dict(c_min=m // 2), "jaccard", MODE_SMH, 0.5),
                                                 (dict(gamma=0.5), "max_containment", MODE_SMH, 0.6), (dict(gamma=G08, c_min=3), "jaccard", MODE_SMH, -1.0)):
                    configure(sel, measure=measure, **rule)
                    got, st = sel.run_queries(tau, mode, 7, 3), sel.stats()
                    want, wst = V.expected_cross(Qa, Qc, Da, Dc, tau, mode == MODE_CB_SMH, measure, **rule)
                    assert_pass(got, st, want, wst, what=(n_q, n_d, m, rule, measure))
                    n_rec += len(want)
    assert n_rec > 0


# ---- 6. pair lists --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [128, 1024, 100])
def test_pair_lists(m):
    n, tau = 129, 0.3
    aux, cards = case(n, m)
    rng = np.random.default_rng(m)
    x, y = rng.integers(0, n, size=4000), rng.integers(0, n, size=4000)
    lst = np.stack([x, y], axis=1)[x != y].astype(np.int32)
    lst = np.concatenate([lst, lst[:300], lst[300:600, ::-1]])              # entries listed twice, in both orders
    n_rec = n_twice = 0
    with Selector(0) as sel:
        sel.upload(zeros_hll(n), aux, cards)
        for rule, measure, mode in ((dict(c_min=1), "jaccard", MODE_CB_SMH), (dict(c_min=m // 2), "jaccard", MODE_SMH),
                                    (dict(gamma=0.5, c_min=2), "max_containment", MODE_SMH), (dict(gamma=G08), "jaccard", MODE_SMH)):
            configure(sel, measure=measure, **rule)
            got, st = sel.run_pairs(lst, tau, mode, 7, 3), sel.stats()
            want, wst = V.expected_list(aux, cards, lst, tau, mode == MODE_CB_SMH, measure, **rule)
            assert_pass(got, st, want, wst, what=(m, rule, measure))
            n_rec += len(want)
            n_twice += len(want) - len(set(M.tuples(want)))                 # an entry listed twice has two records
        assert sel.get_param("pairs_route_used") == 0
        for bad in ([[0, n]], [[-1, 2]], [[5, 5]]):
            with pytest.raises(SelhipError, match="invalid entries"):
                sel.run_pairs(np.array([[0, 1]] + bad, dtype=np.int32), tau, MODE_SMH, 7, 3)
        configure(sel, c_min=1)
        assert_pass(sel.run_pairs(lst, tau, MODE_SMH, 7, 3), sel.stats(), *V.expected_list(aux, cards, lst, tau, False, "jaccard", c_min=1), what="after")
    assert n_rec > 0 and n_twice > 0


# ---- 7. both top-k cuts, with planted ties -----------------------------------------------------------------------------------------------
def tied_rows(n, m, seed):
    """rows in which MANY pairs have the same count: every row shares its first m / 4 buckets with row 0, and groups of five rows share
    another m / 4"""
    aux = CC.random_rows(n, m, seed)
    aux[:, : m // 4] = aux[0, : m // 4]
    for g in range(0, n - 5, 5):
        aux[g:g + 5, m // 2: m // 2 + m // 4] = aux[g, m // 2: m // 2 + m // 4]
    return aux


@pytest.mark.parametrize("m", [128, 100])
def test_all_pairs_top_k_ties(m):
    n, K = 129, 3
    aux, cards = tied_rows(n, m, 5 * m), V.spread_cards(n)
    want, wst = V.expected(aux, cards, -1.0, False, "jaccard", c_min=1)
    assert len(want) == n * (n - 1) // 2 and len(np.unique(want["jaccard"])) <= 4          # c / m is discrete: ties everywhere
    ref = nbr_reference(want, K)
    with Selector(0) as sel:
        sel.upload(zeros_hll(n), aux, cards)
        configure(sel, c_min=1)
        got = sel.run(-1.0, MODE_SMH, 7, 3, top_k=K)
        assert M.tuples(got) == M.tuples(ref) and len(got) == K * n
        assert sel.stats() == wst and sel.stats()["selected"] == len(want)
        # the documented tie order: within an owner and a value, ascending partner rank
        for j in range(1, len(got)):
            if got["i"][j] == got["i"][j - 1] and got["jaccard"][j] == got["jaccard"][j - 1]:
                assert got["k"][j] > got["k"][j - 1]
        sel.set_allpairs_topk(0)
        assert_pass(sel.run(-1.0, MODE_SMH, 7, 3), sel.stats(), want, wst, what="uncut")


@pytest.mark.parametrize("m", [128, 100])
def test_query_top_k_ties(m):
    n_q, n_d, K = 7, 200, 4
    aux = tied_rows(n_q + n_d, m, 9 * m)
    cards = V.spread_cards(n_q + n_d)
    Qa, Qc, Da, Dc = aux[::30][:n_q], cards[::30][:n_q], np.delete(aux, np.arange(0, 30 * n_q, 30), 0), np.delete(cards, np.arange(0, 30 * n_q, 30))
    assert len(Da) == n_d
    whole, wst = V.expected_cross(Qa, Qc, Da, Dc, -1.0, False, "max_containment", c_min=1)
    assert len(whole) == n_q * n_d
    ref = topk_reference(whole, K)
    with Selector(0) as sel:
        sel.upload(zeros_hll(n_d), Da, Dc)
        sel.upload_queries(zeros_hll(n_q), Qa, Qc)
        configure(sel, c_min=1, measure="max_containment")
        got = sel.run_queries(-1.0, MODE_SMH, 7, 3, top_k=K)
        assert M.tuples(got) == M.tuples(ref) and len(got) == K * n_q
        assert sel.stats() == wst
        # Jaccard: the discrete value, ties by ascending database rank
        configure(sel, c_min=1)
        whole, wst = V.expected_cross(Qa, Qc, Da, Dc, -1.0, False, "jaccard", c_min=1)
        got = sel.run_queries(-1.0, MODE_SMH, 7, 3, top_k=K)
        assert M.tuples(got) == M.tuples(topk_reference(whole, K)) and sel.stats()["selected"] == len(whole)
        for j in range(1, len(got)):
            if got["i"][j] == got["i"][j - 1] and got["jaccard"][j] == got["jaccard"][j - 1]:
                assert got["k"][j] > got["k"][j - 1]
        sel.set_query_topk(0)


# ---- 8. the influenza fixtures and the front ends ----------------------------------------------------------------------------------------
def selection(args):
    out = subprocess.run([str(BIN / "selection")] + args, cwd=GOLDEN, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return out.stdout


@pytest.mark.parametrize("m", [512, 64])
def test_influenza(monkeypatch, m):
    monkeypatch.chdir(GOLDEN)
    ds = pkg.load_dataset("influenza_filelist.txt", m, 0)
    n = len(ds.names)
    e = V.trunc_u64(ds.cards)
    with Selector(0) as sel:
        sel.upload(ds.hll, ds.aux, ds.cards)
        J = sel.matrix("smh_jaccard").cpu().numpy()
        C_ = sel.matrix("smh_matches").cpu().numpy()
        assert np.array_equal(C_, M.match_counts(ds.aux, ds.aux).astype(np.float64))
        n_rec = 0
        for c_min, tau in ((1, -1.0), (1, 0.05), (max(1, m // 24), 0.1), (m // 6, 0.0)):
            configure(sel, c_min=c_min)
            got, st = sel.run(tau, MODE_SMH, 7, 3), sel.stats()
            want, wst = V.expected(ds.aux, ds.cards, tau, False, "jaccard", c_min=c_min)
            assert_pass(got, st, want, wst, what=(m, c_min, tau))
            # ... and the dense matrix of the same context, filtered
            keep = np.triu(np.ones((n, n), dtype=bool), 1) & (e != 0)[None, :] & (C_ >= c_min) & (J >= np.float64(np.float32(tau)))
            i, k = np.nonzero(keep)
            assert list(zip(i.tolist(), k.tolist(), J[i, k].view(np.uint64).tolist())) == M.tuples(got)
            n_rec += len(got)
            if tau == 0.05:                                                  # the file-list helper and the CLI print these records
                text = pkg.format_lines(ds.names, got)
                kw = dict(mode=MODE_SMH, criterion="smh_c", min_matches=c_min, estimator="smh")
                assert pkg.select_from_filelist("influenza_filelist.txt", tau, 8 * m, **kw) == text
                assert selection(["-l", "influenza_filelist.txt", "-c", "smh_c", "-C", str(c_min), "-a", str(8 * m), "-h", str(tau), "-n", "-V", "smh"]) == text
                assert 0 < len(got) < wst["survivors"]
        assert n_rec > 0
        # -V hll: what the criterion printed before the switch existed
        configure(sel, c_min=1, estimator="hll")
        assert selection(["-l", "influenza_filelist.txt", "-c", "smh_c", "-C", "1", "-a", str(8 * m), "-h", "-1", "-n", "-V", "hll"]) == \
            pkg.format_lines(ds.names, sel.run(-1.0, MODE_SMH, 7, 3))


def test_cli_queries_pair_lists_and_top_k(tmp_path, monkeypatch):
    monkeypatch.chdir(GOLDEN)
    m = 512
    names = [l.strip() for l in (GOLDEN / "influenza_filelist.txt").read_text().splitlines() if l.strip()]
    q_names, d_names = names[::3], [x for j, x in enumerate(names) if j % 3]
    (tmp_path / "q.txt").write_text("\n".join(q_names) + "\n")
    (tmp_path / "d.txt").write_text("\n".join(d_names) + "\n")
    q, d = str(tmp_path / "q.txt"), str(tmp_path / "d.txt")
    crit = ["-c", "smh_c", "-C", "2", "-a", str(8 * m), "-h", "0.01", "-n", "-V", "smh"]
    kw = dict(mode=MODE_SMH, criterion="smh_c", min_matches=2, estimator="smh")
    ds = pkg.load_dataset("influenza_filelist.txt", m, 0)
    want, _ = V.expected(ds.aux, ds.cards, 0.01, False, "jaccard", c_min=2)
    union = selection(["-l", "influenza_filelist.txt"] + crit)
    assert union == pkg.format_lines(ds.names, want) and len(want) > 0
    # -q: the model on the two lists
    qs, db = pkg.load_dataset(q, m, 0), pkg.load_dataset(d, m, 0)
    cross, _ = V.expected_cross(qs.aux, qs.cards, db.aux, db.cards, 0.01, False, "jaccard", c_min=2)
    lines = "".join(pkg.format_lines([qs.names[i], db.names[k]], np.array([(0, 1, j)], dtype=PAIR_DTYPE)) for i, k, j in zip(cross["i"], cross["k"], cross["jaccard"]))
    got = selection(["-l", d, "-q", q] + crit)
    assert got == lines and len(cross) > 0
    assert pkg.query_from_filelists(q, d, 0.01, 8 * m, **kw) == got
    best = selection(["-l", d, "-q", q, "-k", "1"] + crit)
    assert best == pkg.query_from_filelists(q, d, 0.01, 8 * m, top_k=1, **kw) and 0 < len(best.splitlines()) <= len(q_names)
    # -p: one run's output is the next run's list
    (tmp_path / "p.txt").write_text(union)
    p = str(tmp_path / "p.txt")
    assert selection(["-l", "influenza_filelist.txt", "-p", p] + crit) == union
    assert pkg.select_pairs_from_filelist("influenza_filelist.txt", p, 0.01, 8 * m, **kw) == union
    # -K 3: every genome's three nearest neighbours by SuperMinHash J
    nbr = selection(["-l", "influenza_filelist.txt", "-K", "3"] + crit)
    ref = nbr_reference(want, 3)
    assert nbr == pkg.format_lines(ds.names, ref) and len(ref) > 0
    assert nbr == pkg.select_from_filelist("influenza_filelist.txt", 0.01, 8 * m, top_k=3, **kw)
    # -S max_containment and -G under the estimator
    wantc, _ = V.expected(ds.aux, ds.cards, 0.5, False, "max_containment", gamma=0.5)
    assert selection(["-l", "influenza_filelist.txt", "-c", "smh_c", "-G", "0.5", "-a", str(8 * m), "-h", "0.5", "-n", "-S", "max_containment", "-V", "smh"]) == \
        pkg.format_lines(ds.names, wantc)
    # -o: the result file takes the records as they come
    o = str(tmp_path / "out.selr")
    assert selection(["-l", "influenza_filelist.txt", "-o", o] + crit) == ""
    assert selection(["-r", o]) == union


# ---- 9. refusals, and the way back --------------------------------------------------------------------------------------------------------
def test_refusals_and_return(oracle):
    n, m, tau = 129, 256, 0.3
    hll, aux, cards = M.ranked(oracle, M.hll_pool(n), M.planted_groups(n, m, 77))
    r, b = 2, 128
    lst = np.array([[0, 1], [2, 3], [5, 4]], dtype=np.int32)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        sel.upload_queries(hll[:5], aux[:5], cards[:5])
        before = {}
        for name, crit, args in (("smh_c", CRIT_SMH_C, (7, 3)), ("smh_a", CRIT_SMH_A, (r, b)), ("none", CRIT_NONE, (1, 1))):
            sel.set_criterion(crit)
            if crit == CRIT_SMH_C:
                sel.set_min_matches(m // 2)
            before[name] = ((M.tuples(sel.run(tau, MODE_CB_SMH, *args)), sel.stats()), (M.tuples(sel.run_queries(tau, MODE_CB_SMH, *args)), sel.stats()),
                            (M.tuples(sel.run_pairs(lst, tau, MODE_CB_SMH, *args)), sel.stats()))
        assert len(before["smh_c"][0][0]) > 0 and len(before["none"][0][0]) > 0
        # unknown codes: refused with a message, the setting left alone
        for bad in (2, -1, 17, 34):
            with pytest.raises(SelhipError, match="estimator"):
                pkg._lib.check(sel._lib.selhip_ctx_set_estimator(sel._ctx, bad), sel._ctx)
        with pytest.raises(ValueError, match="estimator"):
            sel.set_estimator("mash")
        sel.set_criterion(CRIT_SMH_C)
        assert (M.tuples(sel.run(tau, MODE_CB_SMH, 7, 3)), sel.stats()) == before["smh_c"][0]          # still the HLL estimator
        sel.set_estimator("smh")
        for bad in (2, -1):
            with pytest.raises(SelhipError, match="estimator"):
                pkg._lib.check(sel._lib.selhip_ctx_set_estimator(sel._ctx, bad), sel._ctx)
        want, wst = V.expected(aux, cards, tau, True, "jaccard", c_min=m // 2)
        assert_pass(sel.run(tau, MODE_CB_SMH, 7, 3), sel.stats(), want, wst, what="still smh")
        # the measure keeps its codes and its refusals
        for bad in (16, 17):
            with pytest.raises(SelhipError, match="measure"):
                pkg._lib.check(sel._lib.selhip_ctx_set_measure(sel._ctx, bad), sel._ctx)
        # every other criterion is refused by every entry, and nothing is consumed
        for crit, args in ((CRIT_SMH_A, (r, b)), (CRIT_NONE, (1, 1)), (CRIT_HLL_A, (1, 1))):
            sel.set_criterion(crit)
            for run in (lambda: sel.run(tau, MODE_CB_SMH, *args), lambda: sel.run_queries(tau, MODE_CB_SMH, *args), lambda: sel.run_pairs(lst, tau, MODE_CB_SMH, *args),
                        lambda: sel.run_async(tau, MODE_CB_SMH, *args)):
                with pytest.raises(SelhipError, match="estimator smh"):
                    run()
        sel.set_criterion(CRIT_SMH_C)
        # max containment keeps refusing the CB mode; the count's own refusals stay
        sel.set_measure("max_containment")
        for run in (lambda: sel.run(tau, MODE_CB_SMH, 7, 3), lambda: sel.run_queries(tau, MODE_CB_SMH, 7, 3), lambda: sel.run_pairs(lst, tau, MODE_CB_SMH, 7, 3)):
            with pytest.raises(SelhipError, match="max_containment"):
                run()
        sel.set_measure("jaccard")
        sel.set_min_matches(m + 1)
        with pytest.raises(SelhipError, match="smh_c.*exceeds"):
            sel.run(tau, MODE_SMH, 7, 3)
        sel.set_min_matches(m // 2)
        assert_pass(sel.run(tau, MODE_CB_SMH, 7, 3), sel.stats(), want, wst, what="after the refusals")
        # SELHIP_E_STATE while a pass is pending
        sel.run_async(tau, MODE_CB_SMH, 7, 3)
        with pytest.raises(SelhipError, match="pending"):
            sel.set_estimator("hll")
        sel.finish()
        assert_pass(sel.fetch(), sel.stats(), want, wst, what="async")
        # sticky: it survives an upload
        sel.upload(hll, aux, cards)
        sel.upload_queries(hll[:5], aux[:5], cards[:5])
        assert_pass(sel.run(tau, MODE_CB_SMH, 7, 3), sel.stats(), want, wst, what="after an upload")
        # and back: the passes of every criterion return what they returned before the switch was ever touched
        sel.set_estimator("hll")
        for name, crit, args in (("smh_c", CRIT_SMH_C, (7, 3)), ("smh_a", CRIT_SMH_A, (r, b)), ("none", CRIT_NONE, (1, 1))):
            sel.set_criterion(crit)
            after = ((M.tuples(sel.run(tau, MODE_CB_SMH, *args)), sel.stats()), (M.tuples(sel.run_queries(tau, MODE_CB_SMH, *args)), sel.stats()),
                     (M.tuples(sel.run_pairs(lst, tau, MODE_CB_SMH, *args)), sel.stats()))
            assert after == before[name], name
    with pytest.raises(SelhipError, match="smh_c"):
        pkg.ooc_select(hll, aux, cards, 0.3, 10, n_rows=1, n_bands=m, criterion=CRIT_SMH_C)
