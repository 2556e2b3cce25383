"""ALGO_INDEX of the query passes on the GPU (include/selection_hip.h section 2b): stage 1 as a lookup in the sorted band-signature
index of the database.  Its records (J bit for bit), its four statistics and its overflow behaviour must be those of ALGO_SIG, i.e. the
cross pairs of the all-pairs result over Q u D; the index is built once per (database, band shape) and kept."""
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_query_gpu import _evaluated, _golden_lines, _sorted_side, assert_same, check_pass, split_sets
from test_query_aux_gpu import CFG_AUX
from test_query_aux_gpu import assert_same as aux_assert_same
from test_query_aux_gpu import check_pass as aux_check_pass
from test_query_aux_gpu import load as aux_load
from test_query_aux_gpu import split_sets as aux_split_sets

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import (ALGO_HASHJOIN, ALGO_INDEX, ALGO_SIG, ALGO_STREAM, CRIT_HLL_A, CRIT_HLL_A_SMH_A, FP_FMA,
                                         FP_STRICT, MODE_CB_SMH, MODE_SMH, SelhipError, Selector, SynthConfig)

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
STATS = ("evaluated", "survivors", "selected", "candidates")


def same_as_sig(sel, tau, mode, r, b):
    """an INDEX pass and a SIG pass on the same context: records, J bits and the four statistics"""
    got = sel.run_queries(tau, mode, r, b, algo=ALGO_INDEX)
    st = sel.stats()
    want = sel.run_queries(tau, mode, r, b, algo=ALGO_SIG)
    wst = sel.stats()
    assert_same(got, want)
    assert all(st[k] == wst[k] for k in STATS), (st, wst)
    return got, st


# 1 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["cfg2", "cfg2-spread"])
@pytest.mark.parametrize("fp", [FP_FMA, FP_STRICT])
def test_index_equals_union_cross_pairs(oracle, cfg_name, fp):
    cfg = pkg.SYNTH_CONFIGS[cfg_name]
    Q, D = split_sets(oracle, cfg, 150, seed=11, fp=fp)
    with Selector(0, fp) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        n_selected = 0
        for tau in sorted({cfg.tau, 0.5}):
            for mode in (MODE_CB_SMH, MODE_SMH):
                n_selected += len(check_pass(sel, oracle, Q, D, tau, mode, ALGO_INDEX, fp))
                cand = sel.stats()["candidates"]
                check_pass(sel, oracle, Q, D, tau, mode, ALGO_SIG, fp)
                assert sel.stats()["candidates"] == cand
        assert n_selected > 0


def test_index_without_directory(oracle):
    """the probe searching whole band segments ("query_index_dir" 0) instead of starting from the bucket directory: same answer"""
    cfg = pkg.SYNTH_CONFIGS["cfg2-spread"]
    Q, D = split_sets(oracle, cfg, 150, seed=12)
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        n_selected = 0
        for use_dir in (0, 1, 0):
            sel.set_param("query_index_dir", use_dir)
            for tau in (cfg.tau, 0.5):
                n_selected += len(check_pass(sel, oracle, Q, D, tau, MODE_CB_SMH, ALGO_INDEX, FP_FMA))
        assert n_selected > 0


# 2 ------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(64, 0.01, 1, 64), (512, 0.8, 8, 64), (512, 0.5, 4, 128), (512, 0.95, 32, 16), (128, 0.9, 8, 16), (64, 0.9, 8, 8),
          (1024, 0.9, 16, 64), (2048, 0.9, 16, 128), (256, 0.8, 8, 32), (256, 0.3, 2, 128), (1024, 0.95, 32, 32), (128, 0.01, 1, 128),
          (64, 0.5, 2, 32), (2048, 0.95, 32, 64)]


@pytest.mark.parametrize("m,tau,rows,bands", SHAPES)
def test_index_band_shapes(oracle, m, tau, rows, bands):
    assert pkg.banding(m, tau) == (rows, bands)
    cfg = SynthConfig(f"idx-shape-{m}", 300, m, tau, 0x5EED0700 + m)
    Q, D = split_sets(oracle, cfg, 60, seed=m)
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        for mode in (MODE_CB_SMH, MODE_SMH):
            got = check_pass(sel, oracle, Q, D, tau, mode, ALGO_INDEX, FP_FMA, rows, bands)
            cand = sel.stats()["candidates"]
            assert_same(check_pass(sel, oracle, Q, D, tau, mode, ALGO_SIG, FP_FMA, rows, bands), got)
            assert sel.stats()["candidates"] == cand


def test_index_band_shapes_cover():
    """the shapes above hold every band count the index takes and rows from 1 to 32"""
    assert {s[3] for s in SHAPES} == {8, 16, 32, 64, 128}
    assert {s[2] for s in SHAPES} == {1, 2, 4, 8, 16, 32}


# 3 ------------------------------------------------------------------------------------------------------------------------------
def test_index_two_stage(oracle):
    cfg = CFG_AUX["cfg2-spread"]
    Q, D = aux_split_sets(oracle, pkg.synth_host(cfg), 200, seed=41)
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        aux_load(sel, Q, D, 8)
        got = aux_check_pass(sel, oracle, Q, D, cfg.tau, MODE_CB_SMH, CRIT_HLL_A_SMH_A, FP_FMA, algo=ALGO_INDEX)
        st = sel.stats()
        assert len(got) > 0
        aux_assert_same(aux_check_pass(sel, oracle, Q, D, cfg.tau, MODE_CB_SMH, CRIT_HLL_A_SMH_A, FP_FMA, algo=ALGO_SIG), got)
        assert sel.stats() == st
        assert sel.get_param("query_db_index_builds") == 1
        # hll_a alone reads neither the band shape nor the algorithm
        sel.set_criterion(CRIT_HLL_A)
        want = sel.run_queries(cfg.tau, MODE_CB_SMH, r, b)
        aux_assert_same(sel.run_queries(cfg.tau, MODE_CB_SMH, r + 1, b, algo=ALGO_INDEX), want)
        assert sel.get_param("query_db_index_builds") == 1


# 4 ------------------------------------------------------------------------------------------------------------------------------
def test_index_lifetime(oracle):
    cfg = pkg.SYNTH_CONFIGS["cfg2-spread"]
    Q1, D = split_sets(oracle, cfg, 120, seed=3)
    hll, aux, _ = pkg.synth_host(SynthConfig("q2", 80, cfg.m, cfg.tau, 0xABC, mode=1, n_sh_lo=8_000, n_sh_hi=200_000))
    Q2 = _sorted_side(oracle, hll, aux)
    r, b = pkg.banding(cfg.m, cfg.tau)
    r2, b2 = pkg.banding(cfg.m, 0.5)
    assert (r2, b2) != (r, b)
    want_all, _ = oracle.select(D[0], D[1], D[2], cfg.tau, r, b)
    builds = lambda sel: (sel.get_param("query_db_index_builds"), sel.get_param("query_db_sig_builds"))      # noqa: E731
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q1[0], Q1[1], Q1[2])
        assert builds(sel) == (0, 0)
        first = check_pass(sel, oracle, Q1, D, cfg.tau, MODE_CB_SMH, ALGO_INDEX, FP_FMA, r, b)
        assert len(first) > 0 and builds(sel) == (1, 1)
        # 8 bytes per (genome, band) + the bucket directory (one 4-byte word per 2 .. 4 entries, + 1 per band), rounded up to a KiB
        n_d = D[0].shape[0]
        assert 8 * n_d * b <= 1024 * sel.get_param("query_db_index_kib") <= 10 * n_d * b + 4 * b + 1024
        check_pass(sel, oracle, Q1, D, cfg.tau, MODE_SMH, ALGO_INDEX, FP_FMA, r, b)                           # another mode
        assert builds(sel) == (1, 1)
        sel.upload_queries(Q2[0], Q2[1], Q2[2])                                                              # new queries
        check_pass(sel, oracle, Q2, D, cfg.tau, MODE_CB_SMH, ALGO_INDEX, FP_FMA, r, b)
        assert builds(sel) == (1, 1)
        check_pass(sel, oracle, Q2, D, cfg.tau, MODE_CB_SMH, ALGO_SIG, FP_FMA, r, b)                         # only the algorithm switches
        check_pass(sel, oracle, Q2, D, cfg.tau, MODE_CB_SMH, ALGO_STREAM, FP_FMA, r, b)
        assert builds(sel) == (1, 1)
        got = sel.run(cfg.tau, MODE_CB_SMH, r, b, algo=ALGO_HASHJOIN)                                        # all-pairs sort join in between
        assert np.array_equal(got["i"], want_all["i"]) and np.array_equal(got["k"], want_all["k"])
        check_pass(sel, oracle, Q2, D, cfg.tau, MODE_CB_SMH, ALGO_INDEX, FP_FMA, r, b)
        assert builds(sel) == (1, 1)
        check_pass(sel, oracle, Q2, D, 0.5, MODE_CB_SMH, ALGO_INDEX, FP_FMA, r2, b2)                         # another band shape replaces it
        assert builds(sel) == (2, 2)
        check_pass(sel, oracle, Q2, D, cfg.tau, MODE_CB_SMH, ALGO_INDEX, FP_FMA, r, b)                       # ... and back
        assert builds(sel) == (3, 3)
        # a different database of the same size: the counter restarts, and a stale index would give the old database's pairs
        Qn, Dn = split_sets(oracle, SynthConfig("db2", cfg.n_genomes, cfg.m, cfg.tau, 0x5EED0777, mode=1, n_sh_lo=8_000, n_sh_hi=200_000),
                            120, seed=3)
        assert Dn[0].shape == D[0].shape
        sel.upload(Dn[0], Dn[1], Dn[2])
        assert builds(sel) == (0, 0) and sel.get_param("query_db_index_kib") == 0
        sel.upload_queries(Qn[0], Qn[1], Qn[2])
        assert len(check_pass(sel, oracle, Qn, Dn, cfg.tau, MODE_CB_SMH, ALGO_INDEX, FP_FMA, r, b)) > 0
        assert builds(sel) == (1, 1)


# 5 ------------------------------------------------------------------------------------------------------------------------------
def _with_copies(oracle, n_db_copies, n_q_copies):
    """cfg2 with one genome copied byte for byte: n_db_copies of it among the database's 900 genomes, n_q_copies among 100 queries"""
    cfg = pkg.SYNTH_CONFIGS["cfg2"]
    hll, aux, _ = pkg.synth_host(cfg)
    g = 500
    Q = _sorted_side(oracle, np.concatenate([hll[:100], np.repeat(hll[g:g + 1], n_q_copies, axis=0)]),
                     np.concatenate([aux[:100], np.repeat(aux[g:g + 1], n_q_copies, axis=0)]))
    D = _sorted_side(oracle, np.concatenate([hll[100:], np.repeat(hll[g:g + 1], n_db_copies, axis=0)]),
                     np.concatenate([aux[100:], np.repeat(aux[g:g + 1], n_db_copies, axis=0)]))
    return cfg, Q, D


def test_index_long_runs_against_sig(oracle):
    """40 000 planted pairs, each equal in every band: runs of 2 001 entries in every band of the index; equal cards on both sides"""
    cfg, Q, D = _with_copies(oracle, 2000, 20)
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        for mode in (MODE_CB_SMH, MODE_SMH):
            got, st = same_as_sig(sel, cfg.tau, mode, r, b)
            assert len(got) >= 40_000 and st["candidates"] >= 40_000


def test_index_long_runs_against_oracle(oracle):
    cfg, Q, D = _with_copies(oracle, 100, 5)
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        for mode in (MODE_CB_SMH, MODE_SMH):
            assert len(check_pass(sel, oracle, Q, D, cfg.tau, mode, ALGO_INDEX, FP_FMA)) >= 500


# 6 ------------------------------------------------------------------------------------------------------------------------------
def test_index_list_growth(oracle):
    """tau = 0.1 and init_cap = 64 as test_query_list_growth; banding gives cfg2 (m = 256) one-row bands there, 1 x 256, which is no index
    shape, so the pass runs with 2 x 128 (the oracle with the same)"""
    cfg = pkg.SYNTH_CONFIGS["cfg2"]
    Q, D = split_sets(oracle, cfg, 200, seed=5)
    with Selector(0) as sel:
        sel.set_param("init_cap", 64)
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        got = check_pass(sel, oracle, Q, D, 0.1, MODE_CB_SMH, ALGO_INDEX, FP_FMA, 2, 128)
        assert len(got) > 64 and sel.last_attempts() >= 2


# 7 ------------------------------------------------------------------------------------------------------------------------------
def test_index_edge_cases(oracle):
    cfg = pkg.SYNTH_CONFIGS["cfg2-spread"]
    hll, aux, _ = pkg.synth_host(cfg.scaled(400))
    D = _sorted_side(oracle, hll[100:], aux[100:])
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        # no queries
        sel.upload_queries(hll[:0], aux[:0], np.zeros(0))
        assert len(sel.run_queries(0.5, algo=ALGO_INDEX)) == 0 and sel.stats()["evaluated"] == 0
        # one query
        Q = _sorted_side(oracle, hll[:1], aux[:1])
        sel.upload_queries(Q[0], Q[1], Q[2])
        for mode in (MODE_CB_SMH, MODE_SMH):
            check_pass(sel, oracle, Q, D, 0.5, mode, ALGO_INDEX, FP_FMA)
        # a database smaller than a wave
        Ds = _sorted_side(oracle, hll[100:150], aux[100:150])
        Q = _sorted_side(oracle, np.concatenate([Ds[0][[3, 3, 40]], hll[:30]]), np.concatenate([Ds[1][[3, 3, 40]], aux[:30]]))
        sel.upload(Ds[0], Ds[1], Ds[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        for mode in (MODE_CB_SMH, MODE_SMH):
            assert len(check_pass(sel, oracle, Q, Ds, 0.5, mode, ALGO_INDEX, FP_FMA)) >= 3


def test_index_zero_cardinalities(oracle):
    """all-zero HLL rows (e = 0) on both sides, as test_query_zero_cardinalities builds them"""
    cfg = pkg.SYNTH_CONFIGS["cfg2"]
    hll, aux, _ = pkg.synth_host(cfg.scaled(300))
    hll[::17] = 0
    aux[::34] = aux[1]                                                   # zero rows that also share every bucket with a live one
    Q = _sorted_side(oracle, hll[:90], aux[:90])
    D = _sorted_side(oracle, hll[90:], aux[90:])
    assert (Q[2] == 0).any() and (D[2] == 0).any()
    with Selector(0) as sel:
        sel.upload(D[0], D[1], None)
        sel.upload_queries(Q[0], Q[1], None)
        for mode in (MODE_CB_SMH, MODE_SMH):
            got = check_pass(sel, oracle, Q, D, 0.5, mode, ALGO_INDEX, FP_FMA)
            cand = sel.stats()["candidates"]
            assert_same(check_pass(sel, oracle, Q, D, 0.5, mode, ALGO_SIG, FP_FMA), got)
            assert sel.stats()["candidates"] == cand
        # tau = 0 bands every bucket on its own (256 bands): not a shape of the index, which refuses
        r, b = pkg.banding(cfg.m, 0.0)
        assert (r, b) == (1, 256)
        with pytest.raises(SelhipError) as e:
            sel.run_queries(0.0, MODE_CB_SMH, r, b, algo=ALGO_INDEX)
        assert e.value.code == -1 and "ALGO_INDEX" in str(e.value) and "1 x 256" in str(e.value)


def test_index_empty_windows(oracle):
    """CB mode, every window empty: the 20 smallest genomes of cfg2-spread against its 100 largest at tau = 0.9"""
    cfg = pkg.SYNTH_CONFIGS["cfg2-spread"]
    hll, aux, _ = pkg.synth_host(cfg)
    order = np.argsort(oracle.cards(hll), kind="stable")
    Q = _sorted_side(oracle, hll[order[:20]], aux[order[:20]])
    D = _sorted_side(oracle, hll[order[-100:]], aux[order[-100:]])
    assert _evaluated(Q[2], D[2], 0.9, True) == 0
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        got = check_pass(sel, oracle, Q, D, 0.9, MODE_CB_SMH, ALGO_INDEX, FP_FMA)
        assert len(got) == 0
        assert all(sel.stats()[k] == 0 for k in STATS)
        assert sel.last_attempts() == 1


# 8 ------------------------------------------------------------------------------------------------------------------------------
def test_index_refusals(oracle):
    cfg = pkg.SYNTH_CONFIGS["cfg2"]
    Q, D = split_sets(oracle, cfg.scaled(300), 50, seed=2)
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        with pytest.raises(SelhipError) as e:                            # the all-pairs pass does not take it
            sel.run(cfg.tau, MODE_CB_SMH, r, b, algo=ALGO_INDEX)
        assert e.value.code == -1 and "bad algo 4" in str(e.value)
        with pytest.raises(SelhipError) as e:                            # nor does a query pass take the all-pairs sort join
            sel.run_queries(cfg.tau, MODE_CB_SMH, r, b, algo=ALGO_HASHJOIN)
        assert e.value.code == -1
        check_pass(sel, oracle, Q, D, cfg.tau, MODE_CB_SMH, ALGO_INDEX, FP_FMA, r, b)
    # band shapes outside the index's on an m = 96 set (built as in test_query_shape_sig_rejects)
    rng = np.random.default_rng(7)
    hll, _, _ = pkg.synth_host(SynthConfig("qshape", 160, 128, 0.9, 4321, n_sh_lo=4000, n_sh_hi=4000))
    aux = rng.integers(0, 2, size=(hll.shape[0], 96), dtype=np.uint64)
    for g in range(1, hll.shape[0], 3):
        aux[g] = aux[g - 1]
        aux[g, rng.integers(0, 96)] ^= np.uint64(1)
    Q, D = _sorted_side(oracle, hll[:40], aux[:40]), _sorted_side(oracle, hll[40:], aux[40:])
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        for rows, bands in ((3, 32), (8, 12)):
            with pytest.raises(SelhipError) as e:
                sel.run_queries(0.0, MODE_SMH, rows, bands, algo=ALGO_INDEX)
            assert e.value.code == -1 and "ALGO_INDEX" in str(e.value) and f"{rows} x {bands}" in str(e.value)
            check_pass(sel, oracle, Q, D, 0.0, MODE_SMH, ALGO_STREAM, FP_FMA, rows, bands)
        assert sel.get_param("query_db_index_builds") == 0


# 9 ------------------------------------------------------------------------------------------------------------------------------
def test_index_medium_against_gpu_sig():
    """cfg4's generator, 50 000 database genomes x 1 000 queries, against the GPU's own SIG pass"""
    import torch
    gen = pkg.SYNTH_CONFIGS["cfg4"]
    n_d, n_q = 50_000, 1_000
    cfg = SynthConfig("idx-medium", n_d + n_q, gen.m, gen.tau, gen.seed ^ 0x0051, cluster_size=gen.cluster_size, mode=gen.mode,
                      n_sh_lo=gen.n_sh_lo, n_sh_hi=gen.n_sh_hi)
    hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg)
    is_q = np.zeros(n_d + n_q, dtype=bool)
    is_q[np.random.default_rng(cfg.seed).choice(n_d + n_q, n_q, replace=False)] = True
    mq = torch.from_numpy(is_q).to(hll_t.device)
    q_t = (hll_t[mq].contiguous(), aux_t[mq].contiguous(), cards_t[mq].contiguous())
    d_t = (hll_t[~mq].contiguous(), aux_t[~mq].contiguous(), cards_t[~mq].contiguous())
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        sel.attach(*d_t)
        sel.attach_queries(*q_t)
        for mode in (MODE_CB_SMH, MODE_SMH):
            got, st = same_as_sig(sel, cfg.tau, mode, r, b)
            assert len(got) > 0 and st["candidates"] >= st["survivors"] > 0
        assert sel.get_param("query_db_index_builds") == 1 and sel.get_param("query_db_sig_builds") == 1


# 10 -----------------------------------------------------------------------------------------------------------------------------
def _cli_lists(tmp_path):
    names = (GOLDEN / "influenza_filelist.txt").read_text().split()
    q_names = [names[0], names[2], names[4]]                            # as test_cli_query_on_reference_fixtures
    d_names = [x for x in names if x not in q_names]
    (tmp_path / "q.txt").write_text("\n".join(q_names) + "\n")
    (tmp_path / "db.txt").write_text("\n".join(d_names) + "\n")
    return q_names


def _cli(tmp_path, *args):
    return subprocess.run([str(BIN / "selection"), "-l", str(tmp_path / "db.txt"), "-q", str(tmp_path / "q.txt"), *args], cwd=GOLDEN,
                          capture_output=True, text=True)


def test_cli_index_on_reference_fixtures(tmp_path, monkeypatch):
    q_names = _cli_lists(tmp_path)
    monkeypatch.chdir(GOLDEN)                                           # the lists hold paths relative to the fixtures
    assert pkg.banding(512 // 8, 0.01) == (1, 64)
    for flag, flavour in (("1", "fma"), ("0", "nofma")):
        out = _cli(tmp_path, "-h", "0.01", "-a", "512", "-F", flag, "-A", "index")
        assert out.returncode == 0, out.stderr
        sig = _cli(tmp_path, "-h", "0.01", "-a", "512", "-F", flag, "-A", "sig")
        assert sig.returncode == 0, sig.stderr
        want = _golden_lines(512, "0.01", flavour, set(q_names))
        assert out.stdout == sig.stdout
        assert sorted(out.stdout.splitlines()) == sorted(want) and len(want) > 0
        py = pkg.query_from_filelists(str(tmp_path / "q.txt"), str(tmp_path / "db.txt"), 0.01, 512, fp_mode=int(flag), algo=ALGO_INDEX)
        assert py == out.stdout


def test_cli_index_refuses_other_shapes(tmp_path):
    _cli_lists(tmp_path)
    assert pkg.banding(32 // 8, 0.9) == (2, 2)
    out = _cli(tmp_path, "-h", "0.9", "-a", "32", "-A", "index")
    assert out.returncode != 0 and out.stdout == ""
    assert "ALGO_INDEX" in out.stderr and "2 x 2" in out.stderr
    assert _cli(tmp_path, "-h", "0.9", "-a", "32", "-A", "auto").returncode == 0
