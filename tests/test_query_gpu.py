"""Query-vs-database selection on the GPU (selhip_ctx_run_queries): the result must be the cross pairs -- one member in the
query set Q, one in the database D -- of the all-pairs result over Q u D, pairs and J bits, with the same evaluated / survivor
counts (include/selection_hip.h section 2b)."""
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import (ALGO_AUTO, ALGO_SIG, ALGO_STREAM, FP_FMA, FP_STRICT, MODE_CB_SMH, MODE_SMH, PAIR_DTYPE,
                                         SelhipError, Selector, SynthConfig)

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
EXP = GOLDEN / "expected"


def _sorted_side(oracle, hll, aux):
    cards = oracle.cards(hll)
    perm = pkg.sort_by_card(cards)
    return hll[perm], aux[perm], cards[perm]


def split_sets(oracle, cfg, n_q, seed, fp=FP_FMA):
    """one generated set, a seeded random n_q of it as queries, the rest as database; each side in its own rank order"""
    hll, aux, _ = pkg.synth_host(cfg)
    pick = np.zeros(hll.shape[0], dtype=bool)
    pick[np.random.default_rng(seed).choice(hll.shape[0], n_q, replace=False)] = True
    oracle.set_fma(fp)
    try:
        return _sorted_side(oracle, hll[pick], aux[pick]), _sorted_side(oracle, hll[~pick], aux[~pick])
    finally:
        oracle.set_fma(1)


def _evaluated(cq, cd, tau, use_cb):
    e_q = cq.astype(np.int64).astype(np.uint64)[:, None]
    e_d = cd.astype(np.int64).astype(np.uint64)[None, :]
    e_lo, e_hi = np.minimum(e_q, e_d), np.maximum(e_q, e_d)
    ok = e_hi != 0
    if use_cb:
        with np.errstate(divide="ignore", invalid="ignore"):
            ok &= (e_lo.astype(np.float64) / e_hi.astype(np.float64)) >= np.float64(np.float32(tau))
    return int(ok.sum())


def union_reference(oracle, Q, D, tau, r, b, use_cb, fp):
    """the all-pairs oracle over Q u D, cut to its cross pairs and mapped to (query rank, database rank); plus the expected
    `evaluated` (numpy, from the truncated cards) and `survivors` (union minus the pairs inside Q and inside D)"""
    (hq, aq, _), (hd, ad, _) = Q, D
    n_q = hq.shape[0]
    hll = np.concatenate([hq, hd])
    aux = np.concatenate([aq, ad])
    oracle.set_fma(fp)
    try:
        cards = oracle.cards(hll)
        perm = pkg.sort_by_card(cards)
        pairs, st = oracle.select(hll[perm], aux[perm], cards[perm], tau, r, b, use_cb=use_cb)
        sq = oracle.select(hq, aq, cards[:n_q], tau, r, b, use_cb=use_cb)[1]["survivors"] if n_q > 1 else 0
        sd = oracle.select(hd, ad, cards[n_q:], tau, r, b, use_cb=use_cb)[1]["survivors"] if hd.shape[0] > 1 else 0
    finally:
        oracle.set_fma(1)
    g1, g2 = perm[pairs["i"]], perm[pairs["k"]]
    cross = (g1 < n_q) != (g2 < n_q)
    qi = np.where(g1 < n_q, g1, g2)[cross]
    di = np.where(g1 < n_q, g2, g1)[cross] - n_q
    out = np.zeros(int(cross.sum()), dtype=PAIR_DTYPE)
    out["i"], out["k"], out["jaccard"] = qi, di, pairs["jacc"][cross]
    out = out[np.lexsort((out["k"], out["i"]))]
    return out, {"evaluated": _evaluated(cards[:n_q], cards[n_q:], tau, use_cb), "survivors": st["survivors"] - sq - sd}


def assert_same(got, want):
    assert got.shape[0] == want.shape[0], (got.shape[0], want.shape[0])
    assert np.array_equal(got["i"], want["i"]) and np.array_equal(got["k"], want["k"])
    assert np.array_equal(got["jaccard"].view(np.uint64), want["jaccard"].view(np.uint64))


def check_pass(sel, oracle, Q, D, tau, mode, algo, fp, r=None, b=None):
    m = Q[1].shape[1]
    if r is None:
        r, b = pkg.banding(m, tau)
    want, wst = union_reference(oracle, Q, D, tau, r, b, mode == MODE_CB_SMH, fp)
    got = sel.run_queries(tau, mode, r, b, algo=algo)
    assert_same(got, want)
    st = sel.stats()
    assert st["evaluated"] == wst["evaluated"] and st["survivors"] == wst["survivors"], (st, wst)
    assert st["selected"] == len(want)
    return got


@pytest.mark.parametrize("cfg_name", ["cfg2", "cfg2-spread"])
@pytest.mark.parametrize("fp", [FP_FMA, FP_STRICT])
def test_query_equals_union_cross_pairs(oracle, cfg_name, fp):
    cfg = pkg.SYNTH_CONFIGS[cfg_name]
    Q, D = split_sets(oracle, cfg, 150, seed=11, fp=fp)
    with Selector(0, fp) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        n_selected = 0
        for tau in sorted({cfg.tau, 0.5}):
            for mode in (MODE_CB_SMH, MODE_SMH):
                for algo in (ALGO_SIG, ALGO_STREAM, ALGO_AUTO):
                    n_selected += len(check_pass(sel, oracle, Q, D, tau, mode, algo, fp))
        assert n_selected > 0


def test_query_shape_sig_rejects(oracle):
    """a band count the signature join does not take: SIG refuses, STREAM and AUTO are exact"""
    rng = np.random.default_rng(7)
    cfg = SynthConfig("qshape", 160, 128, 0.9, 4321, n_sh_lo=4000, n_sh_hi=4000)   # (its buckets are replaced)
    hll, _, _ = pkg.synth_host(cfg)
    aux = rng.integers(0, 2, size=(hll.shape[0], 96), dtype=np.uint64)
    for g in range(1, hll.shape[0], 3):
        aux[g] = aux[g - 1]
        aux[g, rng.integers(0, 96)] ^= np.uint64(1)
    Q, D = _sorted_side(oracle, hll[:40], aux[:40]), _sorted_side(oracle, hll[40:], aux[40:])
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        for rows, bands in ((3, 32), (32, 3), (8, 12), (1, 96)):
            if bands not in (8, 16, 32, 64, 128) or rows & (rows - 1):
                with pytest.raises(SelhipError):
                    sel.run_queries(0.0, MODE_SMH, rows, bands, algo=ALGO_SIG)
            for algo in (ALGO_STREAM, ALGO_AUTO):
                check_pass(sel, oracle, Q, D, 0.0, MODE_SMH, algo, FP_FMA, rows, bands)


def test_query_edge_cases(oracle):
    cfg = pkg.SYNTH_CONFIGS["cfg2-spread"]
    hll, aux, _ = pkg.synth_host(cfg.scaled(400))
    D = _sorted_side(oracle, hll[100:], aux[100:])
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        with pytest.raises(SelhipError):                                  # no queries loaded yet
            sel.run_queries(0.9)
        # one query
        Q = _sorted_side(oracle, hll[:1], aux[:1])
        sel.upload_queries(Q[0], Q[1], Q[2])
        for algo in (ALGO_SIG, ALGO_STREAM):
            check_pass(sel, oracle, Q, D, 0.5, MODE_CB_SMH, algo, FP_FMA)
        # no queries
        sel.upload_queries(hll[:0], aux[:0], np.zeros(0))
        assert len(sel.run_queries(0.5)) == 0 and sel.stats()["evaluated"] == 0
        # exact copies of database genomes (J = 1) and cardinality ties across the two sets
        idx = np.array([0, 5, 5, 50, 299])
        Q = _sorted_side(oracle, np.concatenate([D[0][idx], hll[:20]]), np.concatenate([D[1][idx], aux[:20]]))
        sel.upload_queries(Q[0], Q[1], Q[2])
        for algo in (ALGO_SIG, ALGO_STREAM):
            got = check_pass(sel, oracle, Q, D, 0.9, MODE_CB_SMH, algo, FP_FMA)
            assert (got["jaccard"] > 0.999).sum() >= len(idx)          # (J < 1 by the truncation of e: (2 e - U) / U)
        # unsorted query cards are refused
        with pytest.raises(SelhipError):
            sel.upload_queries(Q[0], Q[1], Q[2][::-1].copy())


def test_query_zero_cardinalities(oracle):
    """all-zero HLL rows (e = 0) on both sides: at tau = 0 a zero query meets every non-zero genome, at tau > 0 none"""
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
        for tau in (0.0, 0.5):
            for mode in (MODE_CB_SMH, MODE_SMH):
                for algo in (ALGO_AUTO, ALGO_STREAM):                    # (tau = 0: one-row bands, which only STREAM takes)
                    check_pass(sel, oracle, Q, D, tau, mode, algo, FP_FMA)


def test_query_attach_and_state(oracle):
    """torch device tensors for both sets; two query batches in a row; the database signatures are built once per band shape;
    an all-pairs pass before and after the query passes returns the oracle's all-pairs result"""
    import torch
    cfg = pkg.SYNTH_CONFIGS["cfg2-spread"]
    Q1, D = split_sets(oracle, cfg, 120, seed=3)
    hll, aux, _ = pkg.synth_host(SynthConfig("q2", 80, cfg.m, cfg.tau, 0xABC, mode=1, n_sh_lo=8_000, n_sh_hi=200_000))
    Q2 = _sorted_side(oracle, hll, aux)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    r, b = pkg.banding(cfg.m, cfg.tau)
    want_all, st_all = oracle.select(D[0], D[1], D[2], cfg.tau, r, b)
    with Selector(0) as sel:
        d_t = (t(D[0]), t(D[1].view(np.int64)))
        sel.attach(*d_t)
        got = sel.run(cfg.tau, MODE_CB_SMH, r, b)
        assert np.array_equal(got["i"], want_all["i"]) and np.array_equal(got["jaccard"].view(np.uint64), want_all["jacc"].view(np.uint64))
        for Q in (Q1, Q2):
            q_t = (t(Q[0]), t(Q[1].view(np.int64)))
            sel.attach_queries(*q_t)
            check_pass(sel, oracle, Q, D, cfg.tau, MODE_CB_SMH, ALGO_SIG, FP_FMA, r, b)
            assert sel.get_param("query_db_sig_builds") == 1
        check_pass(sel, oracle, Q2, D, cfg.tau, MODE_CB_SMH, ALGO_AUTO, FP_FMA, r, b)
        assert sel.get_param("query_db_sig_builds") == 1
        got = sel.run(cfg.tau, MODE_CB_SMH, r, b)
        assert np.array_equal(got["i"], want_all["i"]) and np.array_equal(got["k"], want_all["k"])
        assert np.array_equal(got["jaccard"].view(np.uint64), want_all["jacc"].view(np.uint64))
        assert sel.stats()["evaluated"] == st_all["evaluated"]
        # replacing the database drops the queries
        sel.attach(*d_t)
        with pytest.raises(SelhipError):
            sel.run_queries(cfg.tau)


def test_query_attach_device_cards(oracle):
    """attach_queries with the cards on the device: used as given; cards that are not ascending are refused at the run"""
    import torch
    cfg = pkg.SYNTH_CONFIGS["cfg2-spread"]
    Q, D = split_sets(oracle, cfg, 100, seed=21)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        q_t = (t(Q[0]), t(Q[1].view(np.int64)), t(Q[2]))
        sel.attach_queries(*q_t)
        check_pass(sel, oracle, Q, D, cfg.tau, MODE_CB_SMH, ALGO_AUTO, FP_FMA, r, b)
        bad = t(Q[2][::-1].copy())
        sel.attach_queries(q_t[0], q_t[1], bad)
        with pytest.raises(SelhipError) as e:
            sel.run_queries(cfg.tau, MODE_CB_SMH, r, b)
        assert e.value.code == -1                                        # SELHIP_E_BADARG


def test_query_results_not_framed(oracle):
    """the framed copies carry the all-pairs pass's device-side count: refused after a query pass, accepted again after run"""
    import torch
    cfg = pkg.SYNTH_CONFIGS["cfg2"]
    Q, D = split_sets(oracle, cfg, 100, seed=23)
    frame = torch.zeros((1 << 16) * 16, dtype=torch.uint8, device="cuda")
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        want = sel.run(cfg.tau)
        sel.run_queries(cfg.tau)
        with pytest.raises(SelhipError):
            sel.copy_results_framed(frame)
        with pytest.raises(SelhipError):
            sel.copy_results_framed_async(frame)
        sel.run(cfg.tau)
        assert sel.copy_results_framed(frame) == len(want)


def test_query_list_growth(oracle):
    cfg = pkg.SYNTH_CONFIGS["cfg2"]
    Q, D = split_sets(oracle, cfg, 200, seed=5)
    with Selector(0) as sel:
        sel.set_param("init_cap", 64)
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        got = check_pass(sel, oracle, Q, D, 0.1, MODE_CB_SMH, ALGO_AUTO, FP_FMA)
        assert len(got) > 64 and sel.last_attempts() >= 2


def test_query_medium_against_gpu_union():
    """D = 10 000 (cfg3), Q = 500: against the GPU's own all-pairs pass over Q u D"""
    cfg = pkg.SYNTH_CONFIGS["cfg3"]
    hll, aux, _ = pkg.synth_host(cfg.scaled(10_500))
    n_q = 500
    pick = np.zeros(hll.shape[0], dtype=bool)
    pick[np.random.default_rng(9).choice(hll.shape[0], n_q, replace=False)] = True
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        sel.upload(hll, aux, None)
        cards = sel.cards()
    perm = pkg.sort_by_card(cards)
    is_q = pick[perm]
    u_hll, u_aux, u_cards = hll[perm], aux[perm], cards[perm]
    q_rank = np.cumsum(is_q) - 1
    d_rank = np.cumsum(~is_q) - 1
    with Selector(0) as sel:
        sel.upload(u_hll, u_aux, u_cards)
        allp = sel.run(cfg.tau, MODE_CB_SMH, r, b)
        sel.upload(u_hll[~is_q], u_aux[~is_q], u_cards[~is_q])
        sel.upload_queries(u_hll[is_q], u_aux[is_q], u_cards[is_q])
        got = sel.run_queries(cfg.tau, MODE_CB_SMH, r, b)
    cross = is_q[allp["i"]] != is_q[allp["k"]]
    a, c = allp["i"][cross], allp["k"][cross]
    want = np.zeros(int(cross.sum()), dtype=PAIR_DTYPE)
    want["i"] = np.where(is_q[a], q_rank[a], q_rank[c])
    want["k"] = np.where(is_q[a], d_rank[c], d_rank[a])
    want["jaccard"] = allp["jaccard"][cross]
    want = want[np.lexsort((want["k"], want["i"]))]
    assert len(want) > 0
    assert_same(got, want)


def _golden_lines(a, h, flavour, q_names):
    out = []
    for line in (EXP / f"influenza_smh_a_a{a}_h{h}.{flavour}.txt").read_text().splitlines():
        f1, f2, j = line.split(" ")
        if (f1 in q_names) != (f2 in q_names):
            out.append(f"{f1} {f2} {j}" if f1 in q_names else f"{f2} {f1} {j}")
    return out


@pytest.mark.parametrize("a,h", [(512, "0.01"), (32, "0.9")])
def test_cli_query_on_reference_fixtures(tmp_path, monkeypatch, a, h):
    names = (GOLDEN / "influenza_filelist.txt").read_text().split()
    q_names = [names[0], names[2], names[4]]                            # 3 queries that have partners among the other 7
    d_names = [x for x in names if x not in q_names]
    (tmp_path / "q.txt").write_text("\n".join(q_names) + "\n")
    (tmp_path / "db.txt").write_text("\n".join(d_names) + "\n")
    monkeypatch.chdir(GOLDEN)                                           # the lists hold paths relative to the fixtures
    q_rank = {n: r for r, n in enumerate(pkg.load_dataset(str(tmp_path / "q.txt"), a // 8).names)}
    d_rank = {n: r for r, n in enumerate(pkg.load_dataset(str(tmp_path / "db.txt"), a // 8).names)}
    for flag, flavour in (("1", "fma"), ("0", "nofma")):
        out = subprocess.run([str(BIN / "selection"), "-l", str(tmp_path / "db.txt"), "-q", str(tmp_path / "q.txt"), "-h", h, "-a", str(a),
                              "-F", flag], cwd=GOLDEN, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        got = out.stdout.splitlines()
        want = _golden_lines(a, h, flavour, set(q_names))
        assert sorted(got) == sorted(want) and len(want) > 0
        keys = [(q_rank[ln.split(" ")[0]], d_rank[ln.split(" ")[1]]) for ln in got]
        assert keys == sorted(keys)                                     # (query rank, database rank) order
        py = pkg.query_from_filelists(str(tmp_path / "q.txt"), str(tmp_path / "db.txt"), float(h), a, fp_mode=int(flag))
        assert py.splitlines() == got
