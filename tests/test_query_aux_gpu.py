"""Query passes under the auxiliary-HLL criteria on the GPU (hll_a, hll_an, the two-stage hll_a + smh_a): the result must be the cross
pairs -- one member in the query set Q, one in the database D -- of the all-pairs result over Q u D under the same criterion, pairs
and J bits, with the same evaluated / survivor counts (include/selection_hip.h section 2b)."""
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import (ALGO_AUTO, ALGO_HASHJOIN, ALGO_SIG, ALGO_STREAM, CRIT_HLL_A, CRIT_HLL_A_SMH_A, CRIT_HLL_AN,
                                         CRIT_SMH_A, FP_FMA, FP_STRICT, MODE_CB_SMH, MODE_SMH, PAIR_DTYPE, SelhipError, Selector,
                                         SynthConfig)

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
EXP = GOLDEN / "expected"

# cfg2 / cfg2-spread with auxiliary HLL sketches (p_aux = 8)
CFG_AUX = {
    "cfg2": SynthConfig("cfg2-aux8", 1_000, 256, 0.9, 0x5EED0001, p_aux=8),
    "cfg2-spread": SynthConfig("cfg2-spread-aux8", 1_000, 256, 0.9, 0x5EED0011, p_aux=8, mode=1, n_sh_lo=8_000, n_sh_hi=200_000),
}
CRIT_NAMES = {CRIT_HLL_A: "hll_a", CRIT_HLL_AN: "hll_an", CRIT_HLL_A_SMH_A: "hll_a+smh_a"}


def _side(oracle, hll, aux, ah):
    cards = oracle.cards(hll)
    perm = pkg.sort_by_card(cards)
    return hll[perm], aux[perm], cards[perm], ah[perm]


def split_sets(oracle, data, n_q, seed, fp=FP_FMA):
    """(hll, aux, aux_hll) of one set, a seeded random n_q of it as queries, the rest as database; each side in its own rank order"""
    hll, aux, ah = data
    pick = np.zeros(hll.shape[0], dtype=bool)
    pick[np.random.default_rng(seed).choice(hll.shape[0], n_q, replace=False)] = True
    oracle.set_fma(fp)
    try:
        return _side(oracle, hll[pick], aux[pick], ah[pick]), _side(oracle, hll[~pick], aux[~pick], ah[~pick])
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


def union_reference(oracle, Q, D, tau, r, b, use_cb, fp, crit, p_aux):
    """the all-pairs oracle over Q u D under `crit`, cut to its cross pairs and mapped to (query rank, database rank); plus the
    expected `evaluated` and `survivors` (union minus the pairs inside Q and inside D)"""
    (hq, aq, _, xq), (hd, ad, _, xd) = Q, D
    n_q = hq.shape[0]
    hll, aux, ah = np.concatenate([hq, hd]), np.concatenate([aq, ad]), np.concatenate([xq, xd])
    kw = dict(use_cb=use_cb, criterion=crit, p_aux=p_aux)
    oracle.set_fma(fp)
    try:
        cards = oracle.cards(hll)
        perm = pkg.sort_by_card(cards)
        pairs, st = oracle.select(hll[perm], aux[perm], cards[perm], tau, r, b, aux_hll=ah[perm], **kw)
        sq = oracle.select(hq, aq, cards[:n_q], tau, r, b, aux_hll=xq, **kw)[1]["survivors"] if n_q > 1 else 0
        sd = oracle.select(hd, ad, cards[n_q:], tau, r, b, aux_hll=xd, **kw)[1]["survivors"] if hd.shape[0] > 1 else 0
    finally:
        oracle.set_fma(1)
    g1, g2 = perm[pairs["i"]], perm[pairs["k"]]
    cross = (g1 < n_q) != (g2 < n_q)
    out = np.zeros(int(cross.sum()), dtype=PAIR_DTYPE)
    out["i"] = np.where(g1 < n_q, g1, g2)[cross]
    out["k"] = np.where(g1 < n_q, g2, g1)[cross] - n_q
    out["jaccard"] = pairs["jacc"][cross]
    out = out[np.lexsort((out["k"], out["i"]))]
    return out, {"evaluated": _evaluated(cards[:n_q], cards[n_q:], tau, use_cb), "survivors": st["survivors"] - sq - sd}


def assert_same(got, want):
    assert got.shape[0] == want.shape[0], (got.shape[0], want.shape[0])
    assert np.array_equal(got["i"], want["i"]) and np.array_equal(got["k"], want["k"])
    assert np.array_equal(got["jaccard"].view(np.uint64), want["jaccard"].view(np.uint64))


def load(sel, Q, D, p_aux):
    sel.upload(D[0], D[1], D[2])
    sel.upload_aux_hll(D[3], p_aux)
    sel.upload_queries(Q[0], Q[1], Q[2])
    sel.upload_queries_aux_hll(Q[3], p_aux)


def check_pass(sel, oracle, Q, D, tau, mode, crit, fp, p_aux=8, algo=ALGO_AUTO):
    m = Q[1].shape[1]
    r, b = pkg.banding(m, tau)
    want, wst = union_reference(oracle, Q, D, tau, r, b, mode == MODE_CB_SMH, fp, crit, p_aux)
    sel.set_criterion(crit)
    got = sel.run_queries(tau, mode, r, b, algo=algo)
    assert_same(got, want)
    st = sel.stats()
    assert st["evaluated"] == wst["evaluated"] and st["survivors"] == wst["survivors"], (CRIT_NAMES[crit], st, wst)
    assert st["selected"] == len(want)
    return got


@pytest.mark.parametrize("cfg_name", ["cfg2", "cfg2-spread"])
@pytest.mark.parametrize("fp", [FP_FMA, FP_STRICT])
def test_query_aux_equals_union_cross_pairs(oracle, cfg_name, fp):
    cfg = CFG_AUX[cfg_name]
    data = pkg.synth_host(cfg)
    n_selected = 0
    for c, crit in enumerate((CRIT_HLL_A, CRIT_HLL_AN, CRIT_HLL_A_SMH_A)):
        for mode in (MODE_CB_SMH, MODE_SMH):
            Q, D = split_sets(oracle, data, 150, seed=100 + 10 * c + mode + 4 * fp, fp=fp)      # one random split per case
            with Selector(0, fp) as sel:
                load(sel, Q, D, 8)
                n_selected += len(check_pass(sel, oracle, Q, D, cfg.tau, mode, crit, fp))
    assert n_selected > 0


def _aux_of_precision(base, p_aux, rng):
    """auxiliary registers at p_aux > 12 from the p = 12 registers of the same set: every p = 12 bucket split into 2^(p_aux - 12)
    buckets, each of which sees 2^-(p_aux - 12) of the elements, so its register is about p_aux - 12 lower (a jitter of -1, 0 or +1
    per bucket, the same for every genome: equal p = 12 registers stay equal, and a union of two sketches is still the bucket-wise max)"""
    d = p_aux - 12
    jit = rng.integers(-1, 2, size=base.shape[1] << d).astype(np.int16)
    out = np.repeat(base, 1 << d, axis=1).astype(np.int16)
    out = np.where(out > 0, np.clip(out - d + jit, 1, 64 - p_aux + 1), 0)
    return out.astype(np.uint8)


@pytest.mark.parametrize("p_aux", [4, 12, 15])
def test_query_aux_precisions(oracle, p_aux):
    base = SynthConfig("spread-aux", 600, 128, 0.9, 0x5EED0031, p_aux=min(p_aux, 12), mode=1, n_sh_lo=8_000, n_sh_hi=200_000)
    hll, aux, ah = pkg.synth_host(base)
    if p_aux > 12:
        ah = _aux_of_precision(ah, p_aux, np.random.default_rng(5))
    Q, D = split_sets(oracle, (hll, aux, ah), 100, seed=p_aux)
    n_selected = 0
    with Selector(0) as sel:
        load(sel, Q, D, p_aux)
        for tau in (0.9, 0.5):
            for mode in (MODE_CB_SMH, MODE_SMH):
                n_selected += len(check_pass(sel, oracle, Q, D, tau, mode, CRIT_HLL_A, FP_FMA, p_aux))
    assert n_selected > 0


def test_query_aux_two_stage_algos(oracle):
    """the two-stage criterion over the SIG join and over the stream kernel; the auxiliary stage is timed as "aux"; ALGO_HASHJOIN
    stays refused where the smh_a stage runs and is ignored by hll_a alone"""
    cfg = CFG_AUX["cfg2-spread"]
    Q, D = split_sets(oracle, pkg.synth_host(cfg), 200, seed=41)
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        load(sel, Q, D, 8)
        sel.timing(1)
        results = [check_pass(sel, oracle, Q, D, cfg.tau, MODE_CB_SMH, CRIT_HLL_A_SMH_A, FP_FMA, algo=algo) for algo in (ALGO_SIG, ALGO_STREAM)]
        assert len(results[0]) > 0
        assert sel.kernel_ms("aux") > 0
        with pytest.raises(SelhipError) as e:
            sel.run_queries(cfg.tau, MODE_CB_SMH, r, b, algo=ALGO_HASHJOIN)
        assert e.value.code == -1
        with pytest.raises(SelhipError):
            sel.run_queries(cfg.tau, MODE_CB_SMH, r + 1, b)                 # n_rows * n_bands != m
        sel.set_criterion(CRIT_HLL_A)
        want = sel.run_queries(cfg.tau, MODE_CB_SMH, r, b)
        got = sel.run_queries(cfg.tau, MODE_CB_SMH, r + 1, b, algo=ALGO_HASHJOIN)
        assert_same(got, want)


def test_query_aux_edge_cases(oracle):
    cfg = CFG_AUX["cfg2-spread"]
    hll, aux, ah = pkg.synth_host(cfg.scaled(400))
    D = _side(oracle, hll[100:], aux[100:], ah[100:])
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_aux_hll(D[3], 8)
        # no queries
        sel.upload_queries(hll[:0], aux[:0], np.zeros(0))
        sel.upload_queries_aux_hll(ah[:0], 8)
        for crit in (CRIT_HLL_A, CRIT_HLL_A_SMH_A):
            sel.set_criterion(crit)
            assert len(sel.run_queries(0.5)) == 0 and sel.stats()["evaluated"] == 0
        # one query
        Q = _side(oracle, hll[:1], aux[:1], ah[:1])
        sel.upload_queries(Q[0], Q[1], Q[2])
        sel.upload_queries_aux_hll(Q[3], 8)
        for crit in (CRIT_HLL_A, CRIT_HLL_AN, CRIT_HLL_A_SMH_A):
            check_pass(sel, oracle, Q, D, 0.5, MODE_CB_SMH, crit, FP_FMA)
        # exact copies of database genomes and cardinality ties across the two sets
        idx = np.array([0, 5, 5, 50, 299])
        Q = _side(oracle, np.concatenate([D[0][idx], hll[:20]]), np.concatenate([D[1][idx], aux[:20]]), np.concatenate([D[3][idx], ah[:20]]))
        sel.upload_queries(Q[0], Q[1], Q[2])
        sel.upload_queries_aux_hll(Q[3], 8)
        for crit in (CRIT_HLL_A, CRIT_HLL_AN, CRIT_HLL_A_SMH_A):
            got = check_pass(sel, oracle, Q, D, 0.9, MODE_CB_SMH, crit, FP_FMA)
            assert len(got) >= len(idx)
        # queries whose CB windows are empty: far smaller than every database genome
        small = np.argsort(oracle.cards(hll[:100]))[:10]
        hs = hll[small].copy()
        hs[:, 4096:] = 0                                                   # three quarters of the registers empty: a much smaller cardinality
        Q = _side(oracle, hs, aux[small], ah[small])
        sel.upload_queries(Q[0], Q[1], Q[2])
        sel.upload_queries_aux_hll(Q[3], 8)
        for crit in (CRIT_HLL_A, CRIT_HLL_A_SMH_A):
            sel.set_criterion(crit)
            r, b = pkg.banding(cfg.m, 0.9)
            assert len(sel.run_queries(0.9, MODE_CB_SMH, r, b)) == 0
            want, wst = union_reference(oracle, Q, D, 0.9, r, b, True, FP_FMA, crit, 8)
            assert len(want) == 0 and sel.stats()["evaluated"] == wst["evaluated"] and sel.stats()["survivors"] == wst["survivors"]
            check_pass(sel, oracle, Q, D, 0.9, MODE_SMH, crit, FP_FMA)


def test_query_aux_zero_cardinalities(oracle):
    """all-zero HLL rows (e = 0) on both sides: at tau = 0 a zero query meets every non-zero genome, at tau > 0 none"""
    cfg = CFG_AUX["cfg2"]
    hll, aux, ah = pkg.synth_host(cfg.scaled(300))
    hll[::17] = 0
    ah[::34] = ah[1]                                                     # zero rows whose auxiliary sketch equals a live one's
    Q = _side(oracle, hll[:90], aux[:90], ah[:90])
    D = _side(oracle, hll[90:], aux[90:], ah[90:])
    assert (Q[2] == 0).any() and (D[2] == 0).any()
    with Selector(0) as sel:
        sel.upload(D[0], D[1], None)
        sel.upload_aux_hll(D[3], 8)
        sel.upload_queries(Q[0], Q[1], None)
        sel.upload_queries_aux_hll(Q[3], 8)
        for tau in (0.0, 0.5):
            for mode in (MODE_CB_SMH, MODE_SMH):
                for crit in (CRIT_HLL_A, CRIT_HLL_AN, CRIT_HLL_A_SMH_A):
                    check_pass(sel, oracle, Q, D, tau, mode, crit, FP_FMA)


def test_query_aux_state(oracle):
    """missing / mismatched auxiliary sketches, a new query set drops its auxiliary sketches, attach with a torch tensor, and an
    all-pairs hll_a pass before and after a query pass"""
    import torch
    cfg = CFG_AUX["cfg2-spread"]
    data = pkg.synth_host(cfg)
    Q, D = split_sets(oracle, data, 120, seed=3)
    r, b = pkg.banding(cfg.m, cfg.tau)
    want_all, st_all = oracle.select(D[0], D[1], D[2], cfg.tau, r, b, criterion=CRIT_HLL_A, aux_hll=D[3], p_aux=8)
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_aux_hll(D[3], 8)
        sel.set_criterion(CRIT_HLL_A)
        got = sel.run(cfg.tau, MODE_CB_SMH, r, b)
        assert np.array_equal(got["i"], want_all["i"]) and np.array_equal(got["k"], want_all["k"])
        assert np.array_equal(got["jaccard"].view(np.uint64), want_all["jacc"].view(np.uint64))
        with pytest.raises(SelhipError):                                  # no query set yet
            sel.upload_queries_aux_hll(Q[3], 8)
        sel.upload_queries(Q[0], Q[1], Q[2])
        for crit in (CRIT_HLL_A, CRIT_HLL_AN, CRIT_HLL_A_SMH_A):          # the queries' auxiliary sketches are not loaded
            sel.set_criterion(crit)
            with pytest.raises(SelhipError) as e:
                sel.run_queries(cfg.tau, MODE_CB_SMH, r, b)
            assert e.value.code == -5                                     # SELHIP_E_STATE
        sel.set_criterion(CRIT_SMH_A)
        sel.run_queries(cfg.tau, MODE_CB_SMH, r, b)                       # (smh_a needs none)
        # another precision than the database's
        sel.upload_queries_aux_hll(np.zeros((Q[0].shape[0], 1 << 9), dtype=np.uint8), 9)
        sel.set_criterion(CRIT_HLL_A)
        with pytest.raises(SelhipError) as e:
            sel.run_queries(cfg.tau, MODE_CB_SMH, r, b)
        assert e.value.code == -1                                         # SELHIP_E_BADARG
        sel.upload_queries_aux_hll(Q[3], 8)
        first = check_pass(sel, oracle, Q, D, cfg.tau, MODE_CB_SMH, CRIT_HLL_A, FP_FMA)
        assert len(first) > 0
        # re-uploading the queries drops their auxiliary sketches
        sel.upload_queries(Q[0], Q[1], Q[2])
        with pytest.raises(SelhipError) as e:
            sel.run_queries(cfg.tau, MODE_CB_SMH, r, b)
        assert e.value.code == -5
        # torch tensors: the same result
        dev = torch.device("cuda", 0)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
        q_t = (t(Q[0]), t(Q[1].view(np.int64)))
        sel.attach_queries(*q_t)
        sel.attach_queries_aux_hll(t(Q[3]), 8)
        assert_same(sel.run_queries(cfg.tau, MODE_CB_SMH, r, b), first)
        # the all-pairs pass is unaffected
        got = sel.run(cfg.tau, MODE_CB_SMH, r, b)
        assert np.array_equal(got["i"], want_all["i"]) and np.array_equal(got["k"], want_all["k"])
        assert np.array_equal(got["jaccard"].view(np.uint64), want_all["jacc"].view(np.uint64))
        st = sel.stats()
        assert st["evaluated"] == st_all["evaluated"] and st["survivors"] == st_all["survivors"]


@pytest.mark.parametrize("crit", [CRIT_HLL_A, CRIT_HLL_A_SMH_A])
def test_query_aux_list_growth(oracle, crit):
    cfg = CFG_AUX["cfg2"]
    Q, D = split_sets(oracle, pkg.synth_host(cfg), 200, seed=5)
    with Selector(0) as sel:
        sel.set_param("init_cap", 64)
        load(sel, Q, D, 8)
        got = check_pass(sel, oracle, Q, D, 0.1, MODE_CB_SMH, crit, FP_FMA)
        assert len(got) > 64 and sel.last_attempts() >= 2


def test_query_aux_medium_against_gpu_union():
    """D = 20 000, Q = 500 from cfg5 (m 1024, p_aux 8, tau 0.9), two-stage criterion: against the GPU's own all-pairs pass over Q u D"""
    cfg = pkg.SYNTH_CONFIGS["cfg5"].scaled(20_500)
    hll, aux, ah = pkg.synth_host(cfg)
    n_q = 500
    pick = np.zeros(hll.shape[0], dtype=bool)
    pick[np.random.default_rng(9).choice(hll.shape[0], n_q, replace=False)] = True
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        sel.upload(hll, aux, None)
        cards = sel.cards()
    perm = pkg.sort_by_card(cards)
    is_q = pick[perm]
    u_hll, u_aux, u_cards, u_ah = hll[perm], aux[perm], cards[perm], ah[perm]
    q_rank = np.cumsum(is_q) - 1
    d_rank = np.cumsum(~is_q) - 1
    with Selector(0) as sel:
        sel.upload(u_hll, u_aux, u_cards)
        sel.upload_aux_hll(u_ah, 8)
        sel.set_criterion(CRIT_HLL_A_SMH_A)
        allp = sel.run(cfg.tau, MODE_CB_SMH, r, b)
        sel.upload(u_hll[~is_q], u_aux[~is_q], u_cards[~is_q])
        sel.upload_aux_hll(u_ah[~is_q], 8)
        sel.upload_queries(u_hll[is_q], u_aux[is_q], u_cards[is_q])
        sel.upload_queries_aux_hll(u_ah[is_q], 8)
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


# ---- the reference's influenza fixtures: -q -c hll_a / hll_an against the cross pairs of the reference's all-pairs output ----------
Q_PICK = (1, 5)                                                          # 2 queries with partners among the other 8 at every threshold


def _golden_lines(crit, h, flavour, q_names):
    out = []
    for line in (EXP / f"influenza_{crit}_a256_h{h}.{flavour}.txt").read_text().splitlines():
        f1, f2, j = line.split(" ")
        if (f1 in q_names) != (f2 in q_names):
            out.append(f"{f1} {f2} {j}" if f1 in q_names else f"{f2} {f1} {j}")
    return out


@pytest.mark.parametrize("crit", ["hll_a", "hll_an"])
@pytest.mark.parametrize("h", ["0.01", "0.5", "0.9"])
def test_cli_query_hll_on_reference_fixtures(tmp_path, monkeypatch, crit, h):
    names = (GOLDEN / "influenza_filelist.txt").read_text().split()
    q_names = [names[i] for i in Q_PICK]
    d_names = [x for x in names if x not in q_names]
    (tmp_path / "q.txt").write_text("\n".join(q_names) + "\n")
    (tmp_path / "db.txt").write_text("\n".join(d_names) + "\n")
    monkeypatch.chdir(GOLDEN)                                           # the lists hold paths relative to the fixtures
    q_rank = {n: r for r, n in enumerate(pkg.load_dataset(str(tmp_path / "q.txt"), 0, 8).names)}
    d_rank = {n: r for r, n in enumerate(pkg.load_dataset(str(tmp_path / "db.txt"), 0, 8).names)}
    for flag, flavour in (("1", "fma"), ("0", "nofma")):
        out = subprocess.run([str(BIN / "selection"), "-l", str(tmp_path / "db.txt"), "-q", str(tmp_path / "q.txt"), "-c", crit, "-h", h,
                              "-a", "256", "-F", flag], cwd=GOLDEN, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        got = out.stdout.splitlines()
        want = _golden_lines(crit, h, flavour, set(q_names))
        assert sorted(got) == sorted(want) and len(want) > 0
        keys = [(q_rank[ln.split(" ")[0]], d_rank[ln.split(" ")[1]]) for ln in got]
        assert keys == sorted(keys)                                     # (query rank, database rank) order
        py = pkg.query_from_filelists(str(tmp_path / "q.txt"), str(tmp_path / "db.txt"), float(h), 256, fp_mode=int(flag), criterion=crit)
        assert py.splitlines() == got
