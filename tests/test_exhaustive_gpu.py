"""Criterion "none" (SELHIP_CRIT_NONE) on the GPU: every pair that e_k != 0 and (mode CB) the CB bound leave goes to the HLL-14 Jaccard
test.  Expected values come from the oracle WITHOUT a new code path in it: orc_select under smh_a on SuperMinHash sketches that are all
equal is the exhaustive loop (flat_oracle_select, pinned against the reference's own output in test_exhaustive_host.py).
Every case runs on both routes of the library: the fused kernel ("dense_fused" = 1) and the list route (0)."""
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from test_exhaustive_host import flat_oracle_select

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd.selection import multi_select
from cuda_selection_criteria_amd import (CRIT_HLL_A, CRIT_HLL_A_SMH_A, CRIT_HLL_AN, CRIT_NONE, CRIT_SMH_A, FP_FMA, FP_STRICT, MODE_CB_SMH,
                                         MODE_SMH, PAIR_DTYPE, SYNTH_CONFIGS, SelhipError, Selector, SynthConfig)

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
EXP = GOLDEN / "expected"
ROUTES = (1, 0)                 # "dense_fused": the fused kernel, the list route


def ranked(oracle, hll, aux, fp=FP_FMA):
    """(hll, aux, cards) in rank order under the oracle's report() of flavour fp"""
    if hll.shape[0] == 0:
        return hll, aux, np.zeros(0, dtype=np.float64)
    oracle.set_fma(fp)
    try:
        cards = oracle.cards(hll)
    finally:
        oracle.set_fma(1)
    perm = pkg.sort_by_card(cards)
    return hll[perm], aux[perm], cards[perm]


def assert_same(got, want):
    assert got.shape[0] == want.shape[0], (got.shape[0], want.shape[0])
    assert np.array_equal(got["i"], want["i"]) and np.array_equal(got["k"], want["k"])
    assert np.array_equal(got["jaccard"].view(np.uint64), want["jaccard"].view(np.uint64))


def assert_stats(st, wst, n_sel):
    assert st["evaluated"] == wst["evaluated"], (st, wst)
    assert st["survivors"] == st["evaluated"] and st["candidates"] == st["evaluated"], st
    assert st["selected"] == n_sel, (st, n_sel)


def run_none(sel, tau, mode, fused, rows=None):
    sel.set_criterion(CRIT_NONE)
    sel.set_param("dense_fused", fused)
    got = sel.run(tau, mode, 1, 1, rows=rows)
    assert sel.get_param("dense_route_used") == fused
    return got, sel.stats()


def check_all_pairs(oracle, hll, aux, cards, tau, mode, fp):
    want, wst = flat_oracle_select(oracle, hll, cards, tau, mode == MODE_CB_SMH, fp)
    with Selector(0, fp) as sel:
        sel.upload(hll, aux, cards)
        for fused in ROUTES:
            got, st = run_none(sel, tau, mode, fused)
            print(f"n={len(cards)} tau={tau} mode={mode} fp={fp} fused={fused}: {st} want {len(want)} {wst}")
            assert_same(got, want)
            assert_stats(st, wst, len(want))
    return want


# ---- 1. the oracle's figures --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name", ["cfg2", "cfg2-spread"])
@pytest.mark.parametrize("fp", [FP_FMA, FP_STRICT])
def test_equals_flat_oracle(oracle, cfg_name, fp):
    cfg = SYNTH_CONFIGS[cfg_name]
    hll, aux, _ = pkg.synth_host(cfg)
    hll, aux, cards = ranked(oracle, hll, aux, fp)
    for mode in (MODE_CB_SMH, MODE_SMH):
        for tau in (0.9, 0.5):
            want = check_all_pairs(oracle, hll, aux, cards, tau, mode, fp)
            if cfg_name == "cfg2" and tau == 0.9 and fp == FP_FMA:
                # what smh_a loses at its P >= 0.95 banding: 2 969 of the 2 996 pairs (recall 0.991)
                r, b = pkg.banding(cfg.m, tau)
                with Selector(0, fp) as sel:
                    sel.upload(hll, aux, cards)
                    smh = sel.run(tau, mode, r, b)
                print(f"cfg2 tau 0.9 mode {mode}: exhaustive {len(want)}, smh_a {len(smh)}")
                assert (len(want), len(smh)) == (2996, 2969)
                assert_subset(smh, want, len(cards))


def keys(p, n):
    return p["i"].astype(np.int64) * n + p["k"].astype(np.int64)


def assert_subset(part, whole, n):
    """every record of `part` is in `whole` with the same J bits"""
    kp, kw = keys(part, n), keys(whole, n)
    pos = np.searchsorted(kw, kp)
    assert np.all(pos < len(kw)) and np.array_equal(kw[np.minimum(pos, len(kw) - 1)], kp)
    assert np.array_equal(whole["jaccard"][pos].view(np.uint64), part["jaccard"].view(np.uint64))


# ---- 2. cfg3 at full size: every criterion's result is a subset -----------------------------------------------------------------
def test_cfg3_criteria_are_subsets():
    import torch
    base = SYNTH_CONFIGS["cfg3"]
    cfg = SynthConfig("cfg3-aux8", base.n_genomes, base.m, base.tau, base.seed, p_aux=8)
    hll_t, aux_t, cards_t, _, ah_t = pkg.synth_device(cfg, device=0)
    n = cfg.n_genomes
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        sel.attach(hll_t, aux_t, cards_t)
        sel.attach_aux_hll(ah_t, 8)
        none = {}
        for fused in ROUTES:
            none[fused], st = run_none(sel, cfg.tau, MODE_CB_SMH, fused)
            assert_stats(st, st, len(none[fused]))
            ev = st["evaluated"]
        assert_same(none[1], none[0])
        assert ev == n * (n - 1) // 2 and len(none[1]) > 0
        for crit in (CRIT_SMH_A, CRIT_HLL_A, CRIT_HLL_AN, CRIT_HLL_A_SMH_A):
            sel.set_criterion(crit)
            got = sel.run(cfg.tau, MODE_CB_SMH, r, b)
            st = sel.stats()
            print(f"cfg3 criterion {crit}: {len(got)} of {len(none[1])} exhaustive, {st}")
            assert st["evaluated"] == ev
            assert 0 < len(got) <= len(none[1])
            assert_subset(got, none[1], n)
    del hll_t, aux_t, cards_t, ah_t
    torch.cuda.empty_cache()


# ---- 3. partitions --------------------------------------------------------------------------------------------------------------
def merged(parts):
    out = np.concatenate(parts) if parts else np.zeros(0, dtype=PAIR_DTYPE)
    return out[np.lexsort((out["k"], out["i"]))]


@pytest.mark.parametrize("mode", [MODE_CB_SMH, MODE_SMH])
def test_partitions_add_up(oracle, mode):
    cfg = SYNTH_CONFIGS["cfg2-spread"]
    hll, aux, _ = pkg.synth_host(cfg)
    hll, aux, cards = ranked(oracle, hll, aux)
    n, tau = len(cards), 0.5
    want, wst = flat_oracle_select(oracle, hll, cards, tau, mode == MODE_CB_SMH, FP_FMA)
    assert len(want) > 0
    for fused in ROUTES:
        with Selector(0) as sel:
            sel.upload(hll, aux, cards)
            # row ranges
            parts, ev = [], 0
            for rb, re in ((0, 1), (1, 130), (130, 700), (700, n)):
                got, st = run_none(sel, tau, mode, fused, rows=(rb, re))
                parts.append(got); ev += st["evaluated"]
            assert_same(merged(parts), want)
            assert ev == wst["evaluated"]
            # the parts of a row interleave
            parts, ev = [], 0
            for part in range(3):
                sel.set_row_interleave(32, 3, part)
                got, st = run_none(sel, tau, mode, fused)
                parts.append(got); ev += st["evaluated"]
            sel.set_row_interleave(32, 1, 0)
            assert_same(merged(parts), want)
            assert ev == wst["evaluated"]
            # candidate_begin rectangles: rows [0, h) x candidates >= h, the triangle of the first h genomes, the rows from h on
            h = 333
            sel.set_candidate_begin(h)
            rect, st_r = run_none(sel, tau, mode, fused, rows=(0, h))
            sel.set_candidate_begin(0)
            low, st_l = run_none(sel, tau, mode, fused, rows=(h, n))
            assert np.all(rect["k"] >= h) and np.all(rect["i"] < h)
        with Selector(0) as sel:
            sel.upload(hll[:h], aux[:h], cards[:h])
            tri, st_t = run_none(sel, tau, mode, fused)
        assert_same(merged([rect, tri, low]), want)
        assert st_r["evaluated"] + st_t["evaluated"] + st_l["evaluated"] == wst["evaluated"]
    # the drivers built on the context: out-of-core blocks (250 divides n, 300 does not), one device of the multi-GPU entry
    for block, streams in ((250, 1), (300, 2)):
        got, st = pkg.ooc_select(hll, aux, cards, tau, block, mode=mode, n_rows=1, n_bands=1, n_streams=streams, criterion=CRIT_NONE)
        assert_same(got, want)
        assert_stats(st, wst, len(want))
    got, st = multi_select([0], hll, aux, cards, tau, mode=mode, n_rows=1, n_bands=1, gather=0, criterion=CRIT_NONE)
    assert_same(got, want)
    assert_stats(st, wst, len(want))


# ---- 4. edges -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 2, 65, 129])
def test_small_sets(oracle, n):
    cfg = SYNTH_CONFIGS["cfg2"]
    hll, aux, _ = pkg.synth_host(cfg, g_range=(0, max(n, 1)))
    hll, aux, cards = ranked(oracle, hll[:n], aux[:n])
    for mode in (MODE_CB_SMH, MODE_SMH):
        want = check_all_pairs(oracle, hll, aux, cards, 0.5, mode, FP_FMA)
        if n >= 65:
            assert len(want) > 0


def test_empty_sketches(oracle):
    cfg = SYNTH_CONFIGS["cfg2-spread"]
    hll, aux, _ = pkg.synth_host(cfg, g_range=(0, 150))
    hll[:3] = 0                                       # three empty sketches: cardinality 0, the first ranks
    hll, aux, cards = ranked(oracle, hll, aux)
    assert np.all(cards[:3] == 0) and cards[3] > 0
    for mode in (MODE_CB_SMH, MODE_SMH):
        for tau in (0.5, -1.0):
            want = check_all_pairs(oracle, hll, aux, cards, tau, mode, FP_FMA)
            # a pair of two empty sketches is skipped (e_k == 0); an empty sketch against a non-empty one is evaluated without CB
            assert not np.any(want["k"] < 3)
            if mode == MODE_SMH and tau < 0:
                assert np.count_nonzero(want["i"] < 3) == 3 * 147


@pytest.mark.parametrize("vmax", [23, 24, 31, 32, 47, 51])
def test_high_registers(oracle, vmax):
    """register values that take every instantiation (five and six planes) and every optional walk of bs_pair_hist (>= 24, >= 32, >= 48)"""
    rng = np.random.default_rng(100 + vmax)
    n = 70
    hll = np.minimum(rng.geometric(0.5, size=(n, 16384)), vmax).astype(np.uint8)
    hll[1::2] = np.maximum(hll[1::2], hll[0::2])      # neighbours share most registers: some pairs pass tau
    hll[::3, ::97] = vmax                             # every third row reaches the largest value
    for g, cap_v in zip(range(5, 14), (3, 15, 17, 19, 20, 23, 24, 27, 31)):
        hll[g] = np.minimum(hll[g], min(cap_v, vmax))
    aux = np.zeros((n, 4), dtype=np.uint64)
    hll, aux, cards = ranked(oracle, hll, aux)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        assert sel.get_param("hll_khi") == vmax + 1
    for mode, tau in ((MODE_SMH, 0.3), (MODE_CB_SMH, 0.0)):
        want = check_all_pairs(oracle, hll, aux, cards, tau, mode, FP_FMA)
        assert len(want) > 0


def test_span_boundary_inside_cb_range(oracle):
    """rows whose CB range [i + 1, hi(i)] crosses a multiple of 64 -- the fused kernel's candidate spans -- and rows whose range lies
    inside one span: both kinds exist in this set, and the result is the oracle's"""
    cfg = SYNTH_CONFIGS["cfg2-spread"]
    hll, aux, _ = pkg.synth_host(cfg, g_range=(0, 400))
    hll, aux, cards = ranked(oracle, hll, aux)
    tau = 0.9
    e = cards.astype(np.int64).astype(np.float64)
    hi = np.array([np.max(np.nonzero(e[i] / e >= np.float64(np.float32(tau)))[0]) for i in range(len(e))])
    lo = np.arange(len(e)) + 1
    crossing = np.count_nonzero((hi >= lo) & (lo // 64 != hi // 64))
    inside = np.count_nonzero((hi >= lo) & (lo // 64 == hi // 64))
    assert crossing > 0 and inside > 0, (crossing, inside)
    check_all_pairs(oracle, hll, aux, cards, tau, MODE_CB_SMH, FP_FMA)


def test_result_list_grows(oracle):
    cfg = SYNTH_CONFIGS["cfg2"]
    hll, aux, _ = pkg.synth_host(cfg, g_range=(0, 300))
    hll, aux, cards = ranked(oracle, hll, aux)
    n = len(cards)
    want, wst = flat_oracle_select(oracle, hll, cards, -1.0, False, FP_FMA)
    assert len(want) == n * (n - 1) // 2 == wst["evaluated"]             # tau <= 0 without CB: every evaluated pair is selected
    for fused in ROUTES:
        with Selector(0) as sel:
            sel.set_param("init_cap", 1024)
            sel.upload(hll, aux, cards)
            got, st = run_none(sel, -1.0, MODE_SMH, fused)
            assert sel.last_attempts() > 1
            assert_same(got, want)
            assert_stats(st, wst, len(want))


def test_refusals_and_neighbours(oracle):
    cfg = SYNTH_CONFIGS["cfg2"]
    hll, aux, _ = pkg.synth_host(cfg, g_range=(0, 200))
    hll, aux, cards = ranked(oracle, hll, aux)
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        # p_hll != 14: refused, with a message that names the criterion
        sel.upload(hll[:, :4096], aux, None, p_hll=12)
        sel.set_criterion(CRIT_NONE)
        with pytest.raises(SelhipError, match="criterion none"):
            sel.run(0.9, MODE_CB_SMH, 1, 1)
        # no bit planes (byte-row stage 2a chosen before the upload): refused as well, no fallback
        sel.set_param("hist_algo", 0)
        sel.upload(hll, aux, cards)
        with pytest.raises(SelhipError, match="criterion none"):
            sel.run(0.9, MODE_CB_SMH, 1, 1)
        sel.set_param("hist_algo", -1)
        # an smh_a pass returns the same before and after a none pass on the same context
        sel.upload(hll, aux, cards)
        sel.set_criterion(CRIT_SMH_A)
        before, st_before = sel.run(cfg.tau, MODE_CB_SMH, r, b), sel.stats()
        for fused in ROUTES:
            none, _ = run_none(sel, cfg.tau, MODE_CB_SMH, fused)
            sel.set_criterion(CRIT_SMH_A)
            after = sel.run(cfg.tau, MODE_CB_SMH, r, b)
            assert_same(after, before)
            assert sel.stats() == st_before
            assert_subset(before, none, len(cards))
        assert len(before) > 0


# ---- 5. query passes ------------------------------------------------------------------------------------------------------------
def split(oracle, hll, aux, n_q, seed, fp):
    pick = np.zeros(hll.shape[0], dtype=bool)
    pick[np.random.default_rng(seed).choice(hll.shape[0], n_q, replace=False)] = True
    return ranked(oracle, hll[pick], aux[pick], fp), ranked(oracle, hll[~pick], aux[~pick], fp)


def union_cross_pairs(oracle, Q, D, tau, use_cb, fp):
    """the exhaustive all-pairs result over Q u D cut to its cross pairs, as (query rank, database rank); and the evaluated count"""
    n_q = Q[0].shape[0]
    hll = np.concatenate([Q[0], D[0]])
    cards = np.concatenate([Q[2], D[2]])
    perm = pkg.sort_by_card(cards)
    pairs, _ = flat_oracle_select(oracle, hll[perm], cards[perm], tau, use_cb, fp)
    g1, g2 = perm[pairs["i"]], perm[pairs["k"]]
    cross = (g1 < n_q) != (g2 < n_q)
    out = np.zeros(int(cross.sum()), dtype=PAIR_DTYPE)
    out["i"] = np.where(g1 < n_q, g1, g2)[cross]
    out["k"] = np.where(g1 < n_q, g2, g1)[cross] - n_q
    out["jaccard"] = pairs["jaccard"][cross]
    e_q = Q[2].astype(np.int64).astype(np.uint64)[:, None]
    e_d = D[2].astype(np.int64).astype(np.uint64)[None, :]
    e_lo, e_hi = np.minimum(e_q, e_d), np.maximum(e_q, e_d)
    ok = e_hi != 0
    if use_cb:
        with np.errstate(divide="ignore", invalid="ignore"):
            ok &= (e_lo.astype(np.float64) / e_hi.astype(np.float64)) >= np.float64(np.float32(tau))
    return out[np.lexsort((out["k"], out["i"]))], int(ok.sum())


def check_queries(oracle, Q, D, tau, mode, fp):
    want, ev = union_cross_pairs(oracle, Q, D, tau, mode == MODE_CB_SMH, fp)
    with Selector(0, fp) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        sel.set_criterion(CRIT_NONE)
        for fused in ROUTES:
            sel.set_param("dense_fused", fused)
            got = sel.run_queries(tau, mode, 1, 1)
            st = sel.stats()
            print(f"queries {Q[0].shape[0]} x {D[0].shape[0]} tau={tau} mode={mode} fp={fp} fused={fused}: {st} want {len(want)} / {ev}")
            assert_same(got, want)
            assert_stats(st, {"evaluated": ev}, len(want))
    return want


@pytest.mark.parametrize("cfg_name", ["cfg2", "cfg2-spread"])
@pytest.mark.parametrize("fp", [FP_FMA, FP_STRICT])
def test_queries_equal_union_cross_pairs(oracle, cfg_name, fp):
    cfg = SYNTH_CONFIGS[cfg_name]
    hll, aux, _ = pkg.synth_host(cfg)
    n_sel = 0
    for mode in (MODE_CB_SMH, MODE_SMH):
        for n_q in (0, 1, 100):
            Q, D = split(oracle, hll, aux, n_q, seed=7 + n_q + mode, fp=fp)
            n_sel += len(check_queries(oracle, Q, D, cfg.tau if n_q == 100 else 0.3, mode, fp))
    assert n_sel > 0


def test_queries_with_zero_cardinalities(oracle):
    cfg = SYNTH_CONFIGS["cfg2-spread"]
    hll, aux, _ = pkg.synth_host(cfg, g_range=(0, 300))
    hll[:4] = 0
    pick = np.zeros(300, dtype=bool)
    pick[[0, 1, 10, 20, 30, 40, 50, 60, 70]] = True                  # two empty sketches among the queries, two in the database
    Q, D = ranked(oracle, hll[pick], aux[pick]), ranked(oracle, hll[~pick], aux[~pick])
    assert Q[2][1] == 0 and D[2][1] == 0
    for mode in (MODE_CB_SMH, MODE_SMH):
        for tau in (0.3, -1.0):
            check_queries(oracle, Q, D, tau, mode, FP_FMA)


# ---- 6. the CLI on the influenza fixtures ---------------------------------------------------------------------------------------
def selection(args, **kw):
    out = subprocess.run([str(BIN / "selection")] + args, cwd=GOLDEN, capture_output=True, text=True, **kw)
    assert out.returncode == 0, out.stderr
    return out.stdout


@pytest.mark.parametrize("h", ["0.01", "0.5", "0.9"])
def test_cli_none(h, tmp_path):
    base = ["-l", "influenza_filelist.txt", "-c", "none", "-h", h]
    for flag, flavour in (("1", "fma"), ("0", "nofma")):
        want = (EXP / f"influenza_none_h{h}.{flavour}.txt").read_text()
        assert selection(base + ["-F", flag]) == want
        # (on these ten genomes the CB bound removes no pair that reaches tau: the oracle says so in test_exhaustive_host.py's set)
        assert selection(base + ["-F", flag, "-n"]) == want
        assert selection(base + ["-F", flag, "-B", "4"]) == want
        assert selection(base + ["-F", flag, "-g", "1"]) == want
        res = str(tmp_path / f"none_{flavour}.selr")
        assert selection(base + ["-F", flag, "-o", res]) == ""
        assert selection(["-r", res]) == want
    assert selection(base) == (EXP / f"influenza_none_h{h}.fma.txt").read_text()
    assert h not in ("0.01",) or len(want.splitlines()) == 41


def test_cli_none_queries(tmp_path, monkeypatch):
    monkeypatch.chdir(GOLDEN)
    names = [l.strip() for l in (GOLDEN / "influenza_filelist.txt").read_text().splitlines() if l.strip()]
    q_names, d_names = names[::3], [x for j, x in enumerate(names) if j % 3]
    (tmp_path / "q.txt").write_text("\n".join(q_names) + "\n")
    (tmp_path / "d.txt").write_text("\n".join(d_names) + "\n")
    for h in ("0.01", "0.9"):
        union = (EXP / f"influenza_none_h{h}.fma.txt").read_text().splitlines()
        want = set()
        for line in union:
            a, b, j = line.split(" ")
            if (a in q_names) != (b in q_names):
                want.add((a, b, j) if a in q_names else (b, a, j))
        got = selection(["-l", str(tmp_path / "d.txt"), "-q", str(tmp_path / "q.txt"), "-c", "none", "-h", h]).splitlines()
        assert len(got) == len(want) > 0
        assert {tuple(l.split(" ")) for l in got} == want
        text = pkg.query_from_filelists(str(tmp_path / "q.txt"), str(tmp_path / "d.txt"), float(h), 0, criterion="none")
        assert text.splitlines() == got
    # the Python front end of the all-pairs pass prints the same lines as the reference
    assert pkg.select_from_filelist("influenza_filelist.txt", 0.01, 0, criterion="none") == (EXP / "influenza_none_h0.01.fma.txt").read_text()
