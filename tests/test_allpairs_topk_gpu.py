"""Top-k of the all-pairs passes on the GPU (selhip_ctx_set_allpairs_topk, include/selection_hip.h section 2): the reduced list must be
nbr_reference(S, K) -- same count, same owner, partner and J bits, in ranked order from fetch_ranked and in (i, k) order from fetch --
where S is the result of the same pass with the setting off.  No tolerance anywhere."""
import functools
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_allpairs_topk_host import nbr_reference
from test_exhaustive_gpu import assert_same, ranked
from test_gpu_parity import assert_same_pairs, sorted_set
from test_query_topk_gpu import big_set, by_ik, cfg2_split, check_topk, lds_cap
import test_query_aux_gpu as aux_t

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import (ALGO_AUTO, ALGO_HASHJOIN, ALGO_SIG, ALGO_STREAM, CRIT_HLL_A, CRIT_HLL_A_SMH_A, CRIT_NONE,
                                         CRIT_SMH_A, MODE_CB_SMH, MODE_SMH, SYNTH_CONFIGS, SelhipError, Selector)

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"


# run() = the all-pairs pass; with the setting at K it must leave nbr_reference(S, K) behind
check_nbr = functools.partial(check_topk, setting="allpairs_topk", reference=nbr_reference)


def owned(S, n):
    """L_g: records of S with i = g or k = g"""
    return np.bincount(S["i"], minlength=n) + np.bincount(S["k"], minlength=n)


def first_genomes(oracle, n):
    """the first n genomes of the generated set the query top-k tests use (cfg2-spread, one generation shared), in rank order"""
    hll, aux, cards = big_set(3 + lds_cap() + 1000)
    perm = pkg.sort_by_card(cards[:n])
    return hll[:n][perm], aux[:n][perm], cards[:n][perm]


def exhaustive(sel, rows=None):
    """every pair of the row range to the J test, all of them selected (tau below every J)"""
    return lambda fetch=False: sel.run(-1.0, MODE_SMH, 1, 1, rows=rows, fetch=fetch)


def baseline_none(sel, data, rows=None, cand_begin=0):
    sel.upload(*data)
    sel.set_candidate_begin(cand_begin)
    sel.set_criterion(CRIT_NONE)
    sel.set_allpairs_topk(0)
    return exhaustive(sel, rows)(fetch=True)


# ---- 1. sparse ------------------------------------------------------------------------------------------------------------------
def test_sparse(oracle):
    cfg = SYNTH_CONFIGS["cfg2"]
    hll, aux, cards, _, _ = sorted_set(cfg, oracle)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        base = {}
        for tau in (cfg.tau, 0.5):
            r, b = pkg.banding(cfg.m, tau)
            S = sel.run(tau, MODE_CB_SMH, r, b)
            assert_same_pairs(S, oracle.select(hll, aux, cards, tau, r, b, use_cb=True)[0])
            base[tau] = (S, r, b)
        per_genome = [owned(S, cfg.n_genomes) for S, _, _ in base.values()]
        assert any(c.max() > 5 for c in per_genome) and any(c.min() == 0 for c in per_genome)    # a genome that is cut, one that owns nothing
        for tau, (S, r, b) in base.items():
            L = owned(S, cfg.n_genomes)
            for K in (1, 2, 5, 64, 1024):
                got = check_nbr(sel, S, K, lambda: sel.run(tau, MODE_CB_SMH, r, b, fetch=False))
                assert len(got) == int(np.minimum(L, K).sum())
                assert (len(got) < 2 * len(S)) == bool((L > K).any())


# ---- 2. segment-length boundaries -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [63, 64, 65, 255, 257, 1023, 1024, 1025, "cap", "cap+1"])
def test_segment_length_boundaries(oracle, L):
    cap = lds_cap()
    assert cap >= 1025
    L = {"cap": cap, "cap+1": cap + 1}.get(L, L)
    n = L + 1
    with Selector(0) as sel:
        S = baseline_none(sel, first_genomes(oracle, n), rows=(0, 3))
        # rows 0..2 against everyone: those three own L records each (n - 1 - g as i, g as k), every other genome the three as k
        assert np.array_equal(owned(S, n), [L] * 3 + [3] * (n - 3))
        for K in (1, 3, 64, 1024):
            check_nbr(sel, S, K, exhaustive(sel, (0, 3)))


# ---- 3. hubs fed from the k side only -------------------------------------------------------------------------------------------
def test_hubs_from_the_k_side(oracle):
    n = lds_cap() + 1000
    with Selector(0) as sel:
        S = baseline_none(sel, first_genomes(oracle, n), cand_begin=n - 2)
        L = owned(S, n)
        assert np.array_equal(L[n - 2:], [n - 1, n - 1]) and L[:n - 2].max() == 2 and len(S) == 2 * (n - 2) + 1
        assert np.bincount(S["i"], minlength=n)[n - 2:].sum() == 1            # all but one of the hubs' records arrive as k
        run = exhaustive(sel)
        sel.set_allpairs_topk(10)
        sel.set_candidate_begin(n - 2)
        check_nbr(sel, S, 10, run)


# ---- 4. both sides mixed, a reduced list longer than S ---------------------------------------------------------------------------
def test_full_triangle(oracle):
    n = 370
    data = first_genomes(oracle, n)
    with Selector(0) as sel:
        S = baseline_none(sel, data)
        assert len(S) == n * (n - 1) // 2 == 68265 and np.array_equal(owned(S, n), [n - 1] * n)
        for K in (10, 368, 369, 1024):
            got = check_nbr(sel, S, K, exhaustive(sel))
            assert len(got) == n * min(K, n - 1)
            assert K < 369 or len(got) == 2 * len(S)
    with Selector(0) as sel:
        sel.set_param("init_cap", 64)                                      # the lists start small: the pass repeats, and the result
        sel.upload(*data)                                                  # buffer it ends with is too small for the reduced list
        sel.set_criterion(CRIT_NONE)
        got = check_nbr(sel, S, 369, exhaustive(sel))
        assert sel.last_attempts() > 1 and len(got) == 2 * len(S)


# ---- 5. ties across the cut -----------------------------------------------------------------------------------------------------
def test_ties_across_the_cut(oracle):
    hll, aux, _ = pkg.synth_host(SYNTH_CONFIGS["cfg2-spread"].scaled(8))
    data = ranked(oracle, np.repeat(hll, 6, axis=0), np.repeat(aux, 6, axis=0))      # 8 genomes, 6 identical copies of each
    Ks = (1, 3, 5, 6, 7, 13)
    with Selector(0) as sel:
        S = baseline_none(sel, data)
        assert len(S) == 48 * 47 // 2
        R = nbr_reference(S, 47)                                           # every genome's whole ranking
        bits = R["jaccard"].view(np.uint64).reshape(48, 47)
        assert any((bits[:, K - 1] == bits[:, K]).any() for K in Ks)       # a tie straddles the cut: the smaller partner must win
        for K in Ks:
            got = check_nbr(sel, S, K, exhaustive(sel))
            assert len(got) == 48 * K


# ---- 6. the other routes --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cfg2_ranked():
    import oracle_py
    return sorted_set(SYNTH_CONFIGS["cfg2"], oracle_py.Oracle())[:3]


def check_route(sel, run, K=3):
    sel.set_allpairs_topk(0)
    S = run(True)
    got = check_nbr(sel, S, K, lambda: run(False))
    assert 0 < len(got) < 2 * len(S)
    return S


@pytest.mark.parametrize("route", ["small_pass_1", "small_pass_0", "stream", "hashjoin", "pipeline_2", "grouping_off", "rows"])
def test_other_routes(oracle, route):
    cfg = SYNTH_CONFIGS["cfg2"]
    tau = cfg.tau
    r, b = pkg.banding(cfg.m, tau)
    algo = {"stream": ALGO_STREAM, "hashjoin": ALGO_HASHJOIN}.get(route, ALGO_AUTO)
    rows = (100, 300) if route == "rows" else None
    with Selector(0) as sel:
        if route.startswith("small_pass"):
            sel.set_param("small_pass", int(route[-1]))
        if route == "pipeline_2":
            sel.set_pipeline(2)
        if route == "grouping_off":
            sel.set_stage2_grouping(False)
        sel.upload(*cfg2_ranked())
        S = check_route(sel, lambda fetch: sel.run(tau, MODE_CB_SMH, r, b, rows=rows, algo=algo, fetch=fetch))
        if route.startswith("small_pass"):
            assert sel.get_param("small_pass_used") == int(route[-1])
        if route == "pipeline_2":
            assert sel.get_param("chunks") == 2
        if route == "rows":
            assert S["i"].min() >= 100 and S["i"].max() < 300
        else:
            hll, aux, cards = cfg2_ranked()
            assert_same_pairs(S, oracle.select(hll, aux, cards, tau, r, b, use_cb=True)[0])


@pytest.mark.parametrize("crit", [CRIT_HLL_A, CRIT_HLL_A_SMH_A])
def test_auxiliary_criteria(oracle, crit):
    cfg = aux_t.CFG_AUX["cfg2"]
    hll, aux, cards, _, aux_hll = sorted_set(cfg, oracle)
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        sel.upload_aux_hll(aux_hll, 8)
        sel.set_criterion(crit)
        S = check_route(sel, lambda fetch: sel.run(cfg.tau, MODE_CB_SMH, r, b, fetch=fetch))
        assert_same_pairs(S, oracle.select(hll, aux, cards, cfg.tau, r, b, use_cb=True, criterion=crit, aux_hll=aux_hll, p_aux=8)[0])


@pytest.mark.parametrize("fused", [1, 0])
def test_criterion_none_cb_mode(oracle, fused):
    with Selector(0) as sel:
        sel.upload(*cfg2_ranked())
        sel.set_criterion(CRIT_NONE)
        sel.set_param("dense_fused", fused)
        check_route(sel, lambda fetch: sel.run(0.5, MODE_CB_SMH, 1, 1, fetch=fetch))
        assert sel.get_param("dense_route_used") == fused


# ---- 7. life cycle --------------------------------------------------------------------------------------------------------------
def test_life_cycle(oracle):
    import torch
    cfg = SYNTH_CONFIGS["cfg2"]
    hll, aux, cards = cfg2_ranked()
    r, b = pkg.banding(cfg.m, 0.5)
    run = lambda sel, fetch=True, **kw: sel.run(0.5, MODE_CB_SMH, r, b, fetch=fetch, **kw)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        S = run(sel)
        assert len(S) > 0
        sel.set_allpairs_topk(4)
        for bad in (1025, -1):
            with pytest.raises(SelhipError) as e:
                sel.set_allpairs_topk(bad)
            assert e.value.code == -1
        assert sel.get_param("allpairs_topk") == 4                         # a refused k leaves the setting alone
        sel.upload(hll, aux, cards)
        assert sel.get_param("allpairs_topk") == 4                         # the setting survives uploads
        got = check_nbr(sel, S, 4, lambda: run(sel, fetch=False))
        assert_same(run(sel, top_k=4), got)                                # run(top_k=...) returns the ranked list
        # run_async + finish
        sel.run_async(0.5, MODE_CB_SMH, r, b)
        with pytest.raises(SelhipError) as e:
            sel.set_allpairs_topk(2)                                       # not while a pass is pending
        assert e.value.code == -5
        sel.finish()
        assert_same(sel.fetch_ranked(), got)
        # framed copies carry the device-side |S| counter: refused while the setting is on
        frame = torch.empty((len(S) + 1) * 16, dtype=torch.uint8, device="cuda")
        lib = pkg.hip_lib()
        assert lib.selhip_ctx_copy_results_framed(sel._ctx, frame.data_ptr(), len(S)) == -5
        assert lib.selhip_ctx_copy_results_framed_async(sel._ctx, frame.data_ptr(), len(S)) == -5
        # a tau that selects nothing: nothing more is launched
        sel.timing(1)
        assert len(sel.run(2.0, MODE_CB_SMH, r, b, top_k=4)) == 0 and sel.stats()["selected"] == 0 and sel.result_count() == 0
        assert len(sel.fetch_ranked()) == 0 and len(sel.fetch()) == 0 and sel.kernel_launches("topk") == 0
        sel.timing(0)
        # an empty row range
        assert len(run(sel, rows=(7, 7))) == 0 and len(sel.fetch_ranked()) == 0 and sel.result_count() == 0
        # the query passes ignore the setting
        Q, D = cfg2_split()
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        with Selector(0) as fresh:
            fresh.upload(D[0], D[1], D[2])
            fresh.upload_queries(Q[0], Q[1], Q[2])
            want_q = fresh.run_queries(0.5)
            want_all = fresh.run(0.5)
        assert len(want_q) > 0 and sel.get_param("allpairs_topk") == 4
        assert_same(sel.run_queries(0.5), want_q)
        assert sel.result_count() == len(want_q)
        with pytest.raises(SelhipError) as e:
            sel.fetch_ranked()
        assert e.value.code == -5
        # ... and query_topk leaves an all-pairs pass uncut
        sel.set_allpairs_topk(0)
        sel.set_query_topk(1)
        assert_same(sel.run(0.5), want_all)
        assert sel.result_count() == len(want_all) > 0
        # off again: S exactly, no ranked list, framed copies back
        sel.upload(hll, aux, cards)
        assert_same(run(sel), S)
        assert sel.result_count() == len(S)
        with pytest.raises(SelhipError) as e:
            sel.fetch_ranked()
        assert e.value.code == -5
        assert lib.selhip_ctx_copy_results_framed(sel._ctx, frame.data_ptr(), len(S)) == 0
        torch.cuda.synchronize()
        assert int(frame[:8].view(torch.int64).item()) == len(S)


def test_query_and_allpairs_cuts_share_a_context(oracle):
    """the two cuts are one reduction over one scratch set: a query pass, an all-pairs pass over the same database and the query pass
    again, all cut, on one context -- then the same round with the cfg2 ranked set as the all-pairs pass's database (other owner
    counts and record counts through the same buffers).  Every list bit for bit its reference, the repeated query lists equal"""
    Q, D = cfg2_split()
    with Selector(0) as sel:
        def split():                                                       # an upload drops the queries
            sel.upload(D[0], D[1], D[2])
            sel.upload_queries(Q[0], Q[1], Q[2])
        query = lambda: sel.run_queries(0.5, fetch=False)
        allpairs = lambda: sel.run(0.5, fetch=False)
        split()
        S_q, S_d = sel.run_queries(0.5), sel.run(0.5)
        sel.upload(*cfg2_ranked())
        S_all = sel.run(0.5)
        assert len(S_q) > 0 and len(S_d) > 0 and len(S_all) > len(S_d)
        split()
        first = check_topk(sel, S_q, 3, query)                             # both settings stay on once set
        assert 0 < len(first) < len(S_q)
        assert 0 < len(check_nbr(sel, S_d, 3, allpairs)) < 2 * len(S_d)
        assert_same(check_topk(sel, S_q, 3, query), first)
        sel.upload(*cfg2_ranked())
        assert 0 < len(check_nbr(sel, S_all, 3, allpairs)) < 2 * len(S_all)
        split()
        assert_same(check_topk(sel, S_q, 3, query), first)


@pytest.mark.parametrize("n", [0, 1])
def test_tiny_sets(oracle, n):
    hll, aux, cards = cfg2_ranked()
    with Selector(0) as sel:
        sel.upload(hll[:n], aux[:n], cards[:n])
        assert len(sel.run(0.5, top_k=3)) == 0 and sel.result_count() == 0 and len(sel.fetch()) == 0
        sel.set_criterion(CRIT_NONE)
        assert len(sel.run(-1.0, MODE_SMH, 1, 1, top_k=3)) == 0 and sel.stats()["selected"] == 0


def test_timing_names_topk(oracle):
    with Selector(0) as sel:
        sel.upload(*cfg2_ranked())
        sel.timing(1)
        sel.run(0.5, top_k=0)
        assert sel.kernel_launches("topk") == 0
        sel.timing(1)
        sel.run(0.5, top_k=3)
        assert sel.kernel_ms("topk") > 0 and sel.kernel_launches("topk") == 1


# ---- 8. CLI and driver ----------------------------------------------------------------------------------------------------------
def cli(*args):
    out = subprocess.run([str(BIN / "selection"), "-l", "influenza_filelist.txt"] + list(args), cwd=GOLDEN, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return out.stdout.splitlines()


def ranked_lines(lines):
    """non-increasing printed J inside every owner's run of lines, one run per owner"""
    seen, last = [], None
    for ln in lines:
        g, _, j = ln.split(" ")
        if not seen or seen[-1] != g:
            assert g not in seen
            seen.append(g)
            last = None
        assert last is None or float(j) <= last
        last = float(j)
    return True


def test_cli_exact_neighbours(monkeypatch):
    monkeypatch.chdir(GOLDEN)                                              # the list holds paths relative to the fixtures
    base = ("-c", "none", "-n", "-h", "-1")
    plain = cli(*base)
    assert len(plain) == 45                                                # every pair of the ten genomes
    top3 = cli(*base, "-K", "3")
    assert len(top3) == 30 and ranked_lines(top3)
    assert top3 == pkg.select_from_filelist("influenza_filelist.txt", -1.0, 0, mode=MODE_SMH, criterion="none", top_k=3).splitlines()
    every = cli(*base, "-K", "1024")                                       # every line of the uncut output once in each direction
    both = plain + [" ".join((b, a, j)) for a, b, j in (ln.split(" ") for ln in plain)]
    assert sorted(every) == sorted(both) and ranked_lines(every)
    owners = [ln.split(" ")[0] for ln in every]
    for g in dict.fromkeys(owners):                                        # the three best of every genome lead its full ranking
        assert [ln for ln in top3 if ln.startswith(g + " ")] == [ln for ln in every if ln.startswith(g + " ")][:3]


def test_cli_smh_a(monkeypatch):
    monkeypatch.chdir(GOLDEN)
    plain = cli("-a", "512", "-h", "0.01")
    top2 = cli("-a", "512", "-h", "0.01", "-K", "2")
    assert top2 == pkg.select_from_filelist("influenza_filelist.txt", 0.01, 512, top_k=2).splitlines()
    both = plain + [" ".join((b, a, j)) for a, b, j in (ln.split(" ") for ln in plain)]
    assert 0 < len(top2) < len(both) and set(top2) <= set(both) and ranked_lines(top2)
