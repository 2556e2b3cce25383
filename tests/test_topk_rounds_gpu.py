"""The all-pairs top-k in row rounds (selhip_ctx_set_topk_rounds) on the GPU: every pass in rounds against the
one-shot pass of the same context (records bit for bit in ranked order, statistics), against nbr_reference of the numpy model of the
records, and -- the admitted count -- against the replay of the rounds in tests/topk_rounds_model.py."""
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import smhc_model as M
import smhcc_model as CC
import smhv_model as V
import topk_rounds_model as R
from test_allpairs_topk_host import nbr_reference
from test_smhv_gpu import case, configure, tied_rows, zeros_hll

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import CRIT_NONE, CRIT_SMH_A, CRIT_SMH_C, MODE_CB_SMH, MODE_SMH, SelhipError, Selector

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
AUTO_RECORDS = 1 << 27


def admitted(sel):
    return sel.get_param("topk_admitted_lo") + (sel.get_param("topk_admitted_hi") << 31)


def rounds_of(n_rows, n, rows):
    per = max(1, AUTO_RECORDS // max(1, n)) if rows == "auto" else rows
    return -(-n_rows // per)


def one_shot(sel, K, tau, mode, **kw):
    sel.set_topk_rounds(0)
    got = sel.run(tau, mode, 7, 3, top_k=K, **kw)
    assert sel.get_param("topk_rounds_used") == 0 and admitted(sel) == 0
    return got, sel.stats(), sel.last_attempts()


def in_rounds(sel, K, per_round, tau, mode, **kw):
    got = sel.run(tau, mode, 7, 3, top_k=K, rounds=per_round, **kw)
    return got, sel.stats()


# ---- 1. shapes: both kernel paths, tile / wave / block edges, every K and R, ties everywhere ---------------------------------------------
@pytest.mark.parametrize("m", [128, 256, 512, 1024, 100])
def test_shapes(m):
    n_rec = 0
    with Selector(0) as sel:
        for n in (1, 2, 3, 5, 64, 65, 129, 257):
            aux, cards = tied_rows(n, m, 3 * m + n), V.spread_cards(n)
            sel.upload(zeros_hll(n), aux, cards)
            configure(sel, c_min=1)
            S, wst = V.expected(aux, cards, -1.0, False, "jaccard", c_min=1)
            assert len(S) == n * (n - 1) // 2
            for K in (1, 3, 10, n + 1):
                ref = nbr_reference(S, K)
                whole, st1, _ = one_shot(sel, K, -1.0, MODE_SMH)
                assert M.tuples(whole) == M.tuples(ref) and st1 == wst, (m, n, K)
                for rows in (1, 5, 64, n, n + 7, "auto"):
                    got, st = in_rounds(sel, K, rows, -1.0, MODE_SMH)
                    assert M.tuples(got) == M.tuples(whole), (m, n, K, rows)
                    assert st == st1, (m, n, K, rows, st, st1)
                    assert sel.get_param("topk_rounds_used") == rounds_of(n, n, rows), (m, n, K, rows)
                    assert admitted(sel) <= len(S)
                    if rounds_of(n, n, rows) == 1:
                        assert admitted(sel) == len(S)
                    n_rec += len(got)
                if n >= 2:
                    assert sel.get_param("smhc_path_used") == (1 if m != 100 else 0)
    assert n_rec > 0


# ---- 2. pruning happens, and it is the model's ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [128, 512, 100])
def test_admitted_is_the_models(m):
    """the test a loop without thresholds fails: the count kernels append exactly the records the replay admits"""
    n = 257
    with Selector(0) as sel:
        for aux, cards in (case(n, m), (tied_rows(n, m, 5 * m), V.spread_cards(n))):
            sel.upload(zeros_hll(n), aux, cards)
            configure(sel, c_min=1)
            S, wst = V.expected(aux, cards, -1.0, False, "jaccard", c_min=1)
            for K, rows in ((1, 8), (1, 1), (1, 64), (3, 8), (2, 5)):
                ref, n_adm, per_round, _ = R.replay(S, n, K, rows)
                assert M.tuples(ref) == M.tuples(nbr_reference(S, K))
                got, st = in_rounds(sel, K, rows, -1.0, MODE_SMH)
                print(m, len(S), K, rows, "admitted", admitted(sel), "model", n_adm)
                assert M.tuples(got) == M.tuples(ref) and st == wst
                assert admitted(sel) == n_adm, (m, K, rows)
                assert sel.get_param("topk_rounds_used") == len(per_round) == -(-n // rows)
        # (the planted groups came first) n = 257, K = 1, R = 8: strictly below |S|
        aux, cards = case(n, m)
        sel.upload(zeros_hll(n), aux, cards)
        S, wst = V.expected(aux, cards, -1.0, False, "jaccard", c_min=1)
        in_rounds(sel, 1, 8, -1.0, MODE_SMH)
        assert 0 < admitted(sel) < len(S) == sel.stats()["selected"]


# ---- 3. the boundary of the exact test -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [128, 100])
def test_admission_boundary(m):
    """K = 1, one row per round.  Row 0 gives genome 5 its first record at 20 buckets and the rows 1 .. 4 one at 30.  Then (1, 5) comes
    one bucket below thr[5] and is dropped, (2, 5) EQUALS it and is admitted -- its partner ranks after the one held, so the record
    stays --, (3, 5) is one bucket above and displaces it, and (4, 5), at the old threshold, is dropped.  (A later tie with a LOWER
    partner rank cannot be planted: rounds ascend in the rows, so a later record's partner is, for either owner, larger than every
    partner that owner holds.)"""
    n = 6
    aux = CC.random_rows(n, m, 44 + m)
    cards = V.spread_cards(n)
    aux[0, :20] = aux[5, :20]
    aux[1:5, 50:80] = aux[0, 50:80]
    for i, c in ((1, 19), (2, 20), (3, 21), (4, 20)):
        aux[i, 20:20 + c] = aux[5, 20:20 + c]
    S, wst = V.expected(aux, cards, -1.0, False, "jaccard", c_min=1)
    cnt = {(int(r["i"]), int(r["k"])): int(round(r["jaccard"] * m)) for r in S}
    assert [cnt[(i, 5)] for i in range(5)] == [20, 19, 20, 21, 20] and cnt[(0, 1)] == 30
    ref, n_adm, per_round, lists = R.replay(S, n, 1, 1)
    for rnd, (pair, inside) in enumerate((((1, 5), False), ((2, 5), True), ((3, 5), True), ((4, 5), False)), start=1):
        thr = R.thresholds(lists[rnd - 1], n, 1)
        v = np.float64(cnt[pair]) / np.float64(m)
        assert (v >= thr[pair[0]] or v >= thr[pair[1]]) == inside, (pair, v, thr)
    assert np.float64(20) / np.float64(m) == R.thresholds(lists[1], n, 1)[5]                     # the tie is exact
    held = {int(r["i"]): int(r["k"]) for r in ref}
    assert held[5] == 3 and {int(r["i"]): int(r["k"]) for r in lists[2]}[5] == 0                  # the tie did not displace, the better one did
    with Selector(0) as sel:
        sel.upload(zeros_hll(n), aux, cards)
        configure(sel, c_min=1)
        whole, st1, _ = one_shot(sel, 1, -1.0, MODE_SMH)
        got, st = in_rounds(sel, 1, 1, -1.0, MODE_SMH)
        assert M.tuples(got) == M.tuples(whole) == M.tuples(ref) and st == st1 == wst
        assert admitted(sel) == n_adm < len(S)
        assert sel.get_param("topk_rounds_used") == n
        for K, rows in ((1, 2), (2, 1), (2, 3)):
            ref, n_adm, _, _ = R.replay(S, n, K, rows)
            got, st = in_rounds(sel, K, rows, -1.0, MODE_SMH)
            assert M.tuples(got) == M.tuples(ref) and st == wst and admitted(sel) == n_adm, (K, rows)


# ---- 4. both rules, both measures, the CB mode, two thresholds -----------------------------------------------------------------------------
@pytest.mark.parametrize("m", [128, 256, 100])
def test_rules_and_measures(m):
    n = 129
    n_pruned = 0
    with Selector(0) as sel:
        for aux in (tied_rows(n, m, 7 * m), M.planted_groups(n, m, 31 * m)):
            for cards, rule, measure, mode in ((V.spread_cards(n), dict(gamma=0.3, c_min=max(1, m // 8)), "jaccard", MODE_SMH),
                                               (V.spread_cards(n), dict(gamma=CC.G08), "jaccard", MODE_SMH),
                                               (V.spread_cards(n, ratio=100.0), dict(c_min=1), "max_containment", MODE_SMH),
                                               (V.spread_cards(n, ratio=100.0), dict(gamma=0.3, c_min=2), "max_containment", MODE_SMH),
                                               (V.spread_cards(n, ratio=3.0), dict(c_min=1), "jaccard", MODE_CB_SMH)):
                sel.upload(zeros_hll(n), aux, cards)
                configure(sel, measure=measure, **rule)
                for tau in (-1.0, 0.5):
                    S, wst = V.expected(aux, cards, tau, mode == MODE_CB_SMH, measure, **rule)
                    if measure == "max_containment" and tau < 0 and len(S):
                        assert S["jaccard"].max() > 1.0
                    for K, rows in ((1, 8), (3, 5), (10, 64)):
                        ref, n_adm, _, _ = R.replay(S, n, K, rows)
                        whole, st1, _ = one_shot(sel, K, tau, mode)
                        got, st = in_rounds(sel, K, rows, tau, mode)
                        what = (m, rule, measure, mode, tau, K, rows)
                        assert M.tuples(got) == M.tuples(whole) == M.tuples(ref), what
                        assert st == st1 == wst, what
                        assert admitted(sel) == n_adm, what
                        n_pruned += n_adm < len(S)
                        assert sel.get_param("smhc_rule_used") == (1 if "gamma" in rule else 0)
    assert n_pruned > 0


# ---- 5. composition: row range, candidate begin, row interleave, chunk lanes --------------------------------------------------------------
@pytest.mark.parametrize("m", [128, 100])
def test_composition(m):
    n, K = 257, 3
    aux, cards = tied_rows(n, m, 11 * m), V.spread_cards(n)
    aux[::3, m - 9:] = aux[0, m - 9:]                                     # a third value level
    with Selector(0) as sel:
        sel.upload(zeros_hll(n), aux, cards)
        configure(sel, c_min=1)
        # a row range
        S, wst = V.expected(aux, cards, -1.0, False, "jaccard", c_min=1, rows=(5, n - 3))
        whole, st1, _ = one_shot(sel, K, -1.0, MODE_SMH, rows=(5, n - 3))
        for rows in (1, 8, 64, 300, "auto"):
            got, st = in_rounds(sel, K, rows, -1.0, MODE_SMH, rows=(5, n - 3))
            assert M.tuples(got) == M.tuples(whole) == M.tuples(nbr_reference(S, K)) and st == st1 == wst, rows
            assert sel.get_param("topk_rounds_used") == rounds_of(n - 8, n, rows)
            if rows != "auto":
                assert admitted(sel) == R.replay(S, n, K, rows, rows=(5, n - 3))[1]
        # a candidate begin
        sel.set_candidate_begin(100)
        S, wst = V.expected(aux, cards, -1.0, False, "jaccard", c_min=1, cand_begin=100)
        whole, st1, _ = one_shot(sel, K, -1.0, MODE_SMH)
        for rows in (8, 64):
            got, st = in_rounds(sel, K, rows, -1.0, MODE_SMH)
            assert M.tuples(got) == M.tuples(whole) == M.tuples(nbr_reference(S, K)) and st == st1 == wst, rows
            assert admitted(sel) == R.replay(S, n, K, rows)[1]
        sel.set_candidate_begin(0)
        # a row interleave: a round is whole periods of the deal (2 x 64 x 2 rows), whatever rows says
        for part in (0, 1):
            sel.set_row_interleave(64, 2, part)
            whole, st1, _ = one_shot(sel, K, -1.0, MODE_SMH)
            assert 0 < len(whole)
            for rows in (1, 8, 256, 257):
                got, st = in_rounds(sel, K, rows, -1.0, MODE_SMH)
                assert M.tuples(got) == M.tuples(whole) and st == st1, (part, rows)
                assert sel.get_param("topk_rounds_used") == (1 if rows == 257 else 2)
        sel.set_row_interleave(64, 1, 0)
        # two chunk lanes inside every round
        sel.set_pipeline(2)
        S, wst = V.expected(aux, cards, -1.0, False, "jaccard", c_min=1)
        whole, st1, _ = one_shot(sel, K, -1.0, MODE_SMH)
        assert sel.get_param("chunks") == 2
        for rows in (8, 64):
            got, st = in_rounds(sel, K, rows, -1.0, MODE_SMH)
            assert sel.get_param("chunks") == 2
            assert M.tuples(got) == M.tuples(whole) == M.tuples(nbr_reference(S, K)) and st == st1 == wst, rows
            assert admitted(sel) == R.replay(S, n, K, rows)[1]
        # run_async + finish drive the same rounds
        sel.set_pipeline(-1)
        sel.set_topk_rounds(8)
        sel.run_async(-1.0, MODE_SMH, 7, 3)
        sel.finish()
        assert M.tuples(sel.fetch_ranked()) == M.tuples(whole) and sel.stats() == wst and sel.get_param("topk_rounds_used") == 33
        assert M.tuples(sel.fetch()) == sorted(M.tuples(whole))
        assert sel.result_count() == len(whole)


# ---- 6. an overflow inside a later round ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [128, 100])
def test_overflow_in_a_later_round(m):
    """the first round admits 45 records, the second more than the list holds: that round alone repeats, and C survives it"""
    n, K, rows = 300, 3, 64
    aux, cards = CC.random_rows(n, m, 21 * m), V.spread_cards(n)
    aux[64:, : m // 2] = aux[64, : m // 2]
    aux[:10, m // 2:] = aux[0, m // 2:]
    S, wst = V.expected(aux, cards, -1.0, False, "jaccard", c_min=1)
    ref, n_adm, per_round, _ = R.replay(S, n, K, rows)
    assert per_round[0] == 45 and per_round[1] > 4096 and M.tuples(ref) == M.tuples(nbr_reference(S, K))
    with Selector(0) as sel:
        sel.set_param("init_cap", 1024)
        sel.upload(zeros_hll(n), aux, cards)
        configure(sel, c_min=1)
        got, st = in_rounds(sel, K, rows, -1.0, MODE_SMH)
        assert sel.last_attempts() > 1
        assert M.tuples(got) == M.tuples(ref) and st == wst
        assert sel.get_param("topk_rounds_used") == 5
        assert admitted(sel) == n_adm                                   # (the attempt that overflowed is not counted)
        again, st2 = in_rounds(sel, K, rows, -1.0, MODE_SMH)            # the lists have grown: one attempt a round now
        assert sel.last_attempts() == 1 and M.tuples(again) == M.tuples(ref) and st2 == wst and admitted(sel) == n_adm


# ---- 7. the fixtures, the front ends, the refusals, and what the setting leaves alone ---------------------------------------------------
def selection(args, code=0):
    out = subprocess.run([str(BIN / "selection")] + args, cwd=GOLDEN, capture_output=True, text=True)
    assert out.returncode == code, out.stderr
    return out.stdout if code == 0 else out.stderr


@pytest.mark.parametrize("m", [512, 64])
def test_influenza_front_ends(monkeypatch, m):
    monkeypatch.chdir(GOLDEN)
    base = ["-l", "influenza_filelist.txt", "-c", "smh_c", "-C", "1", "-a", str(8 * m), "-h", "-1", "-n", "-V", "smh", "-K", "3"]
    text = selection(base)
    assert len(text.splitlines()) > 3
    for rows in ("2", "1", "auto", "1000"):
        assert selection(base + ["-R", rows]) == text, rows
    kw = dict(mode=MODE_SMH, criterion="smh_c", min_matches=1, estimator="smh", top_k=3)
    assert pkg.select_from_filelist("influenza_filelist.txt", -1.0, 8 * m, **kw) == text
    assert pkg.select_from_filelist("influenza_filelist.txt", -1.0, 8 * m, top_k_rounds=2, **kw) == text
    assert pkg.select_from_filelist("influenza_filelist.txt", -1.0, 8 * m, top_k_rounds="auto", **kw) == text
    # -K prints text: -o and -r stay refused, with or without -R
    for extra in ([], ["-R", "2"]):
        assert "-K (the best partners of every genome) cannot be combined with -o" in selection(base + extra + ["-o", "x.selr"], code=2)
        assert "-K (the best partners of every genome) cannot be combined with -r" in selection(base + extra + ["-r", "x.selr"], code=2)


def test_refusals_and_what_stays(oracle):
    n, m, tau = 129, 256, 0.3
    hll, aux, cards = M.ranked(oracle, M.hll_pool(n), M.planted_groups(n, m, 77))
    r, b = 2, 128
    lst = np.array([[0, 1], [2, 3], [5, 4]], dtype=np.int32)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        sel.upload_queries(hll[:5], aux[:5], cards[:5])
        assert sel.get_param("topk_rounds") == 0 and sel.get_param("topk_rounds_used") == 0
        before = {}
        for name, crit, args in (("smh_c", CRIT_SMH_C, (7, 3)), ("smh_a", CRIT_SMH_A, (r, b)), ("none", CRIT_NONE, (1, 1))):
            sel.set_criterion(crit)
            if crit == CRIT_SMH_C:
                sel.set_min_matches(m // 2)
            before[name] = ((M.tuples(sel.run(tau, MODE_CB_SMH, *args)), sel.stats()), (M.tuples(sel.run_queries(tau, MODE_CB_SMH, *args)), sel.stats()),
                            (M.tuples(sel.run_pairs(lst, tau, MODE_CB_SMH, *args)), sel.stats()),
                            (M.tuples(sel.run(tau, MODE_CB_SMH, *args, top_k=2)), sel.stats()))
            sel.set_allpairs_topk(0)
        assert len(before["smh_c"][0][0]) > 0 and len(before["none"][3][0]) > 0
        # values: -2 and below are refused with a message, the setting left alone
        for bad in (-2, -3, -(1 << 40)):
            with pytest.raises(SelhipError, match="top-k rounds"):
                pkg._lib.check(sel._lib.selhip_ctx_set_topk_rounds(sel._ctx, bad), sel._ctx)
        with pytest.raises(ValueError, match="rounds"):
            sel.set_topk_rounds(-2)
        assert sel.get_param("topk_rounds") == 0
        sel.set_topk_rounds("auto")
        assert sel.get_param("topk_rounds") == -1
        sel.set_topk_rounds(16)
        assert sel.get_param("topk_rounds") == 16
        # rounds on: an all-pairs pass without the top-k, without smh_c or without the estimator is refused, and nothing is consumed
        sel.set_criterion(CRIT_SMH_C)
        sel.set_estimator("smh")
        with pytest.raises(SelhipError, match="selhip_ctx_set_topk_rounds"):
            sel.run(tau, MODE_CB_SMH, 7, 3)                                  # no top-k
        sel.set_estimator("hll")
        with pytest.raises(SelhipError, match="selhip_ctx_set_topk_rounds"):
            sel.run(tau, MODE_CB_SMH, 7, 3, top_k=2)                         # no estimator smh
        for crit, args in ((CRIT_SMH_A, (r, b)), (CRIT_NONE, (1, 1))):
            sel.set_criterion(crit)
            with pytest.raises(SelhipError, match="selhip_ctx_set_topk_rounds"):
                sel.run(tau, MODE_CB_SMH, *args)
            with pytest.raises(SelhipError, match="selhip_ctx_set_topk_rounds"):
                sel.run_async(tau, MODE_CB_SMH, *args)
        # query passes and pair-list passes do not read it
        sel.set_allpairs_topk(0)
        for name, crit, args in (("smh_c", CRIT_SMH_C, (7, 3)), ("smh_a", CRIT_SMH_A, (r, b)), ("none", CRIT_NONE, (1, 1))):
            sel.set_criterion(crit)
            assert (M.tuples(sel.run_queries(tau, MODE_CB_SMH, *args)), sel.stats()) == before[name][1], name
            assert (M.tuples(sel.run_pairs(lst, tau, MODE_CB_SMH, *args)), sel.stats()) == before[name][2], name
        # the pass it is for, SELHIP_E_STATE while it is pending, and sticky over an upload
        sel.set_criterion(CRIT_SMH_C)
        sel.set_estimator("smh")
        S, wst = V.expected(aux, cards, tau, True, "jaccard", c_min=m // 2)
        ref = nbr_reference(S, 2)
        assert len(ref) > 0
        assert M.tuples(sel.run(tau, MODE_CB_SMH, 7, 3, top_k=2)) == M.tuples(ref) and sel.stats() == wst
        assert sel.get_param("topk_rounds_used") == -(-n // 16)
        sel.run_async(tau, MODE_CB_SMH, 7, 3)
        with pytest.raises(SelhipError, match="pending"):
            sel.set_topk_rounds(0)
        sel.finish()
        assert M.tuples(sel.fetch_ranked()) == M.tuples(ref)
        sel.upload(hll, aux, cards)
        sel.upload_queries(hll[:5], aux[:5], cards[:5])
        assert sel.get_param("topk_rounds") == 16
        assert M.tuples(sel.run(tau, MODE_CB_SMH, 7, 3)) == sorted(M.tuples(ref)) and sel.get_param("topk_rounds_used") == -(-n // 16)
        with pytest.raises(SelhipError, match="framed"):
            import torch
            buf = torch.empty(16 * (len(ref) + 1), dtype=torch.uint8, device="cuda")
            pkg._lib.check(sel._lib.selhip_ctx_copy_results_framed(sel._ctx, buf.data_ptr(), len(ref)), sel._ctx)
        # and off again: every pass returns what it returned before the setting was ever touched
        sel.set_topk_rounds(0)
        sel.set_estimator("hll")
        sel.set_allpairs_topk(0)
        for name, crit, args in (("smh_c", CRIT_SMH_C, (7, 3)), ("smh_a", CRIT_SMH_A, (r, b)), ("none", CRIT_NONE, (1, 1))):
            sel.set_criterion(crit)
            after = ((M.tuples(sel.run(tau, MODE_CB_SMH, *args)), sel.stats()), (M.tuples(sel.run_queries(tau, MODE_CB_SMH, *args)), sel.stats()),
                     (M.tuples(sel.run_pairs(lst, tau, MODE_CB_SMH, *args)), sel.stats()),
                     (M.tuples(sel.run(tau, MODE_CB_SMH, *args, top_k=2)), sel.stats()))
            sel.set_allpairs_topk(0)
            assert after == before[name], name
            assert sel.get_param("topk_rounds_used") == 0
