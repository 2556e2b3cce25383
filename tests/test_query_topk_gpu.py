"""Top-k of the query passes on the GPU (selhip_ctx_set_query_topk, include/selection_hip.h section 2b): the reduced list must be
topk_reference(S, K) -- same count, same i, k and J bits, in ranked order from fetch_ranked and in (i, k) order from fetch -- where S is
the result of the same pass with top-k off, which must first equal the oracle's cross pairs.  No tolerance anywhere."""
import functools
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_query_topk_host import topk_reference
from test_query_gpu import assert_same, split_sets, union_reference
from test_exhaustive_gpu import ranked, split as split_none, union_cross_pairs
import test_query_aux_gpu as aux_t

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import (ALGO_INDEX, ALGO_SIG, ALGO_STREAM, CRIT_HLL_A, CRIT_HLL_A_SMH_A, CRIT_NONE, CRIT_SMH_A,
                                         FP_FMA, MODE_CB_SMH, MODE_SMH, PAIR_DTYPE, SYNTH_CONFIGS, SelhipError, Selector)

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"


def by_ik(recs):
    return recs[np.lexsort((recs["k"], recs["i"]))]


def check_topk(sel, S, K, run, setting="query_topk", reference=topk_reference):
    """run() = the pass; with the setting at K it must leave reference(S, K) behind"""
    getattr(sel, "set_" + setting)(K)
    assert sel.get_param(setting) == K
    run()
    want = reference(S, K)
    got = sel.fetch_ranked()
    print(f"K={K}: |S|={len(S)} reduced {len(got)} (want {len(want)}), attempts {sel.last_attempts()}")
    assert_same(got, want)
    assert sel.result_count() == len(want) and sel.stats()["selected"] == len(S)
    assert_same(sel.fetch(), by_ik(want))
    return got


def cross_reference(oracle, Q, D, tau):
    """criterion none, MODE_SMH, from the oracle's union estimator on the cross pairs alone: every (q, d) with e_hi != 0 and
    J = (e_lo + e_hi - U) / U >= (double)(float)tau, in (i, k) order"""
    e_q = Q[2].astype(np.int64).astype(np.float64)
    e_d = D[2].astype(np.int64).astype(np.float64)
    n_q, n_d = len(e_q), len(e_d)
    U = np.array([[oracle.union_size(Q[0][q], D[0][d]) for d in range(n_d)] for q in range(n_q)], dtype=np.float64).reshape(n_q, n_d)
    lo, hi = np.minimum(e_q[:, None], e_d[None, :]), np.maximum(e_q[:, None], e_d[None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        J = ((lo + hi) - U) / U
    ok = (hi != 0) & (J >= np.float64(np.float32(tau)))
    qi, di = np.nonzero(ok)
    out = np.zeros(len(qi), dtype=PAIR_DTYPE)
    out["i"], out["k"], out["jaccard"] = qi, di, J[qi, di]
    return out


def run_none(sel, tau=-1.0):
    return lambda: sel.run_queries(tau, MODE_SMH, 1, 1, fetch=False)


def baseline_none(sel, oracle, Q, D, tau=-1.0, want=None):
    """S of the exhaustive query pass with top-k off, checked against the oracle"""
    sel.upload(D[0], D[1], D[2])
    sel.upload_queries(Q[0], Q[1], Q[2])
    sel.set_criterion(CRIT_NONE)
    sel.set_query_topk(0)
    S = sel.run_queries(tau, MODE_SMH, 1, 1)
    assert_same(S, cross_reference(oracle, Q, D, tau) if want is None else want)
    return S


# ---- 1. sparse segments ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cfg2_split():
    import oracle_py
    return split_sets(oracle_py.Oracle(), SYNTH_CONFIGS["cfg2"], 150, seed=11)


def test_sparse_segments(oracle):
    cfg = SYNTH_CONFIGS["cfg2"]
    Q, D = cfg2_split()
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        base = {}
        for tau in (cfg.tau, 0.5):
            r, b = pkg.banding(cfg.m, tau)
            S = sel.run_queries(tau, MODE_CB_SMH, r, b, algo=ALGO_SIG)
            assert_same(S, union_reference(oracle, Q, D, tau, r, b, True, FP_FMA)[0])
            base[tau] = (S, r, b)
        per_query = [np.bincount(S["i"], minlength=150) for S, _, _ in base.values()]
        assert any(c.max() > 5 for c in per_query) and any(c.min() == 0 for c in per_query)      # cut segments and empty ones
        for tau, (S, r, b) in base.items():
            for K in (1, 2, 5, 64, 1024):
                got = check_topk(sel, S, K, lambda: sel.run_queries(tau, MODE_CB_SMH, r, b, algo=ALGO_SIG, fetch=False))
                assert K > 5 or len(got) < len(S)


# ---- 2. segment-length boundaries, 4. one hot segment ---------------------------------------------------------------------------
def lds_cap():
    with Selector(0) as sel:
        return sel.get_param("query_topk_lds_cap")


@functools.lru_cache(maxsize=None)
def big_set(n):
    """n generated genomes (cfg2-spread) with the oracle's cards, in generation order"""
    import oracle_py
    hll, aux, _ = pkg.synth_host(SYNTH_CONFIGS["cfg2-spread"].scaled(n))
    return hll, aux, oracle_py.Oracle().cards(hll)


def sides(n_q, n_d, total):
    hll, aux, cards = big_set(total)
    def side(sl):
        perm = pkg.sort_by_card(cards[sl])
        return hll[sl][perm], aux[sl][perm], cards[sl][perm]
    return side(slice(0, n_q)), side(slice(n_q, n_q + n_d))


@pytest.mark.parametrize("n_d", [63, 64, 65, 255, 257, 1023, 1024, 1025, "cap", "cap+1"])
def test_segment_length_boundaries(oracle, n_d):
    cap = lds_cap()
    assert cap >= 1025
    n_d = {"cap": cap, "cap+1": cap + 1}.get(n_d, n_d)
    Q, D = sides(3, n_d, 3 + cap + 1000)
    with Selector(0) as sel:
        S = baseline_none(sel, oracle, Q, D)
        assert (S["jaccard"] < 0).any()
        assert np.array_equal(np.bincount(S["i"], minlength=3), [n_d] * 3)      # every segment has the length under test
        for K in (1, 64, 1024):
            check_topk(sel, S, K, run_none(sel))


def test_one_hot_segment(oracle):
    cap = lds_cap()
    Q, D = sides(1, cap + 1000, 3 + cap + 1000)
    with Selector(0) as sel:
        S = baseline_none(sel, oracle, Q, D)
        assert len(S) == cap + 1000
        check_topk(sel, S, 10, run_none(sel))


def test_mixed_queries_in_a_wave(oracle):
    """70 queries x 300 genomes: segments of 300 records, so the waves of the grouping kernels see several query ranks"""
    hll, aux, _ = pkg.synth_host(SYNTH_CONFIGS["cfg2-spread"].scaled(370))
    Q, D = split_none(oracle, hll, aux, 70, seed=3, fp=FP_FMA)
    want, _ = union_cross_pairs(oracle, Q, D, -1.0, False, FP_FMA)
    with Selector(0) as sel:
        S = baseline_none(sel, oracle, Q, D, want=want)
        assert len(S) > 70 * 250
        for K in (10, 299, 300):
            check_topk(sel, S, K, run_none(sel))


# ---- 3. ties across the cut -----------------------------------------------------------------------------------------------------
def test_ties_across_the_cut(oracle):
    hll, aux, _ = pkg.synth_host(SYNTH_CONFIGS["cfg2-spread"].scaled(13))
    Q = ranked(oracle, hll[:5], aux[:5])
    D = ranked(oracle, np.repeat(hll[5:], 6, axis=0), np.repeat(aux[5:], 6, axis=0))     # 8 genomes, 6 identical copies of each
    Ks = (1, 3, 6, 7, 13)
    with Selector(0) as sel:
        S = baseline_none(sel, oracle, Q, D)
        assert len(S) == 5 * 48
        R = topk_reference(S, 48)                                          # every query's whole ranking
        bits = R["jaccard"].view(np.uint64).reshape(5, 48)
        assert any((bits[:, K - 1] == bits[:, K]).any() for K in Ks)       # a tie straddles the cut: the smaller rank must win
        for K in Ks:
            got = check_topk(sel, S, K, run_none(sel))
            assert len(got) == 5 * K


# ---- 5. the other routes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [ALGO_INDEX, ALGO_STREAM])
def test_other_algorithms(oracle, algo):
    cfg = SYNTH_CONFIGS["cfg2"]
    Q, D = cfg2_split()
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        S = sel.run_queries(cfg.tau, MODE_CB_SMH, r, b, algo=algo)
        assert_same(S, union_reference(oracle, Q, D, cfg.tau, r, b, True, FP_FMA)[0])
        got = check_topk(sel, S, 3, lambda: sel.run_queries(cfg.tau, MODE_CB_SMH, r, b, algo=algo, fetch=False))
        assert 0 < len(got) < len(S)


@pytest.mark.parametrize("crit", [CRIT_HLL_A, CRIT_HLL_A_SMH_A])
def test_auxiliary_criteria(oracle, crit):
    cfg = aux_t.CFG_AUX["cfg2"]
    Q, D = aux_t.split_sets(oracle, pkg.synth_host(cfg), 150, seed=17)
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        aux_t.load(sel, Q, D, 8)
        sel.set_criterion(crit)
        S = sel.run_queries(cfg.tau, MODE_CB_SMH, r, b)
        assert_same(S, aux_t.union_reference(oracle, Q, D, cfg.tau, r, b, True, FP_FMA, crit, 8)[0])
        got = check_topk(sel, S, 3, lambda: sel.run_queries(cfg.tau, MODE_CB_SMH, r, b, fetch=False))
        assert 0 < len(got) < len(S)


# ---- 6. life cycle --------------------------------------------------------------------------------------------------------------
def test_life_cycle(oracle):
    cfg = SYNTH_CONFIGS["cfg2"]
    Q, D = cfg2_split()
    r, b = pkg.banding(cfg.m, 0.1)
    with Selector(0) as fresh:
        fresh.upload(D[0], D[1], D[2])
        want_all = fresh.run(cfg.tau)
    with Selector(0) as sel:
        sel.set_param("init_cap", 64)                                      # the lists start small: the pass repeats
        sel.upload(D[0], D[1], D[2])
        for bad in (1025, -1):
            with pytest.raises(SelhipError) as e:
                sel.set_query_topk(bad)
            assert e.value.code == -1
        assert sel.get_param("query_topk") == 0
        # no queries
        sel.upload_queries(Q[0][:0], Q[1][:0], np.zeros(0))
        assert len(sel.run_queries(0.1, MODE_CB_SMH, r, b, top_k=5)) == 0 and sel.result_count() == 0 and len(sel.fetch()) == 0
        # top-k behind a pass that had to repeat
        sel.upload_queries(Q[0], Q[1], Q[2])
        assert sel.get_param("query_topk") == 5                            # the setting survives uploads
        sel.set_query_topk(0)
        S = sel.run_queries(0.1, MODE_CB_SMH, r, b)
        assert_same(S, union_reference(oracle, Q, D, 0.1, r, b, True, FP_FMA)[0])
        assert len(S) > 64
    with Selector(0) as sel:
        sel.set_param("init_cap", 64)
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        got = check_topk(sel, S, 2, lambda: sel.run_queries(0.1, MODE_CB_SMH, r, b, fetch=False))
        assert sel.last_attempts() > 1 and len(got) < len(S)
        assert_same(sel.run_queries(0.1, MODE_CB_SMH, r, b, top_k=2), got)  # run_queries(top_k=...) returns the ranked list
        # a tau that selects nothing
        sel.set_criterion(CRIT_NONE)
        assert len(sel.run_queries(2.0, MODE_SMH, 1, 1, top_k=7)) == 0 and sel.stats()["selected"] == 0
        assert len(sel.fetch_ranked()) == 0
        sel.set_criterion(CRIT_SMH_A)
        # off again: all of S, and no ranked list
        sel.set_query_topk(0)
        assert_same(sel.run_queries(0.1, MODE_CB_SMH, r, b), S)
        with pytest.raises(SelhipError) as e:
            sel.fetch_ranked()
        assert e.value.code == -5
        # an all-pairs pass is not cut, whatever the setting, and has no ranked list
        sel.set_query_topk(1)
        got_all = sel.run(cfg.tau)
        assert_same(got_all, want_all)
        assert len(want_all) > 0
        assert sel.result_count() == len(want_all)
        with pytest.raises(SelhipError) as e:
            sel.fetch_ranked()
        assert e.value.code == -5


def test_timing_names_topk(oracle):
    Q, D = cfg2_split()
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        sel.timing(1)
        sel.run_queries(0.5, top_k=0)
        assert sel.kernel_launches("topk") == 0
        sel.timing(1)
        sel.run_queries(0.5, top_k=3)
        assert sel.kernel_ms("topk") > 0 and sel.kernel_launches("topk") == 1


# ---- 7. CLI and driver ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,a,crit", [(["-a", "512", "-h", "0.01"], 512, "smh_a"), (["-c", "none", "-h", "0.01"], 0, "none")])
def test_cli_topk_on_reference_fixtures(tmp_path, monkeypatch, args, a, crit):
    names = (GOLDEN / "influenza_filelist.txt").read_text().split()
    q_names = [names[0], names[2], names[4]]
    d_names = [x for x in names if x not in q_names]
    q_file, d_file = str(tmp_path / "q.txt"), str(tmp_path / "db.txt")
    (tmp_path / "q.txt").write_text("\n".join(q_names) + "\n")
    (tmp_path / "db.txt").write_text("\n".join(d_names) + "\n")
    monkeypatch.chdir(GOLDEN)                                           # the lists hold paths relative to the fixtures

    def cli(*extra):
        out = subprocess.run([str(BIN / "selection"), "-l", d_file, "-q", q_file] + args + list(extra), cwd=GOLDEN, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        return out.stdout.splitlines()

    def ranked_lines(lines):
        """non-increasing printed J inside every query's run of lines, one run per query"""
        seen, last = [], None
        for ln in lines:
            q, _, j = ln.split(" ")
            if not seen or seen[-1] != q:
                assert q not in seen
                seen.append(q)
                last = None
            assert last is None or float(j) <= last
            last = float(j)
        return True

    plain = cli()
    per_query = {q: sum(ln.startswith(q + " ") for ln in plain) for q in q_names}
    assert max(per_query.values()) > 2                                  # -k 2 cuts something
    top2 = cli("-k", "2")
    assert top2 == pkg.query_from_filelists(q_file, d_file, 0.01, a, criterion=crit, top_k=2).splitlines()
    assert len(top2) == sum(min(2, c) for c in per_query.values()) and set(top2) <= set(plain) and ranked_lines(top2)
    every = cli("-k", "1024")                                           # larger than any segment: the same lines, regrouped
    assert sorted(every) == sorted(plain) and ranked_lines(every)
    assert every == pkg.query_from_filelists(q_file, d_file, 0.01, a, criterion=crit, top_k=1024).splitlines()
    for q in q_names:                                                   # the two best of every query lead its full ranking
        assert [ln for ln in top2 if ln.startswith(q + " ")] == [ln for ln in every if ln.startswith(q + " ")][:2]
