"""Cardinalities forged onto every threshold (tests/decision_model.py) through every copy of each decision on the device.

The sets are tiny (at most 200 genomes, m = 64, one shared band: every pair clears smh_a), the cardinalities are the only thing that
varies, and every comparison is exact: the records (i, k, J bits) and the evaluated / survivor counts of oracle.select on the same forged
cards.  Sets whose forged pairs are all accepted are apart from sets whose forged pairs are all rejected, and the forged pairs are looked
up by name.  DESIGN.md (section "Forged cardinalities") lists which test reaches which decision site."""
import functools

import numpy as np
import pytest

import decision_model as M
import sig_model as S
from test_allpairs_topk_host import nbr_reference
from test_exhaustive_gpu import assert_same
from test_gpu_parity import assert_same_pairs

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import (ALGO_AUTO, ALGO_HASHJOIN, ALGO_INDEX, ALGO_SIG, ALGO_STREAM, CRIT_HLL_A, CRIT_HLL_A_SMH_A, CRIT_HLL_AN,
                                         CRIT_NONE, CRIT_SMH_A, FP_FMA, FP_STRICT, MODE_CB_SMH, MODE_SMH, PAIR_DTYPE, Selector)

pytestmark = pytest.mark.gpu

SIDES = {"inside": True, "outside": False}
J_TAUS = (0.5, 0.8, 0.9, 0.95)
FPS = {"fma": FP_FMA, "strict": FP_STRICT}


# ---- references ------------------------------------------------------------------------------------------------------------------
_REF = {}


def reference(oracle, gs, tau, use_cb, crit=CRIT_SMH_A, fp=FP_FMA, p_aux=8, ranks=None):
    """oracle.select on the set's own forged cards (criterion none = smh_a here: one band is shared); ranks: a sub-set, in its order.
    Computed once per set (the sets are cached for the session) and shared by the tests"""
    crit = CRIT_SMH_A if crit == CRIT_NONE else crit
    key = (id(gs), tau, use_cb, crit, fp, p_aux, None if ranks is None else tuple(ranks.tolist()))
    if key not in _REF:
        pick = slice(None) if ranks is None else ranks
        oracle.set_fma(fp)
        try:
            _REF[key] = oracle.select(gs.hll[pick], gs.aux[pick], gs.cards[pick], tau, gs.r, gs.nb, use_cb=use_cb, criterion=crit,
                                      aux_hll=None if gs.aux_hll is None else gs.aux_hll[pick], p_aux=p_aux)
        finally:
            oracle.set_fma(1)
    return _REF[key]


def as_records(want):
    out = np.zeros(len(want), dtype=PAIR_DTYPE)
    out["i"], out["k"], out["jaccard"] = want["i"], want["k"], want["jacc"]
    return out


def cross_reference(oracle, gs, q, d, tau, use_cb, crit=CRIT_SMH_A, fp=FP_FMA, p_aux=8):
    """query pass of the set's ranks q against its ranks d: the cross pairs of the all-pairs oracle over the whole set, as (rank in q,
    rank in d); the counts are the whole set's minus those inside q and inside d"""
    want, st = reference(oracle, gs, tau, use_cb, crit, fp, p_aux)
    inner = [reference(oracle, gs, tau, use_cb, crit, fp, p_aux, ranks=side)[1] if len(side) > 1 else {"evaluated": 0, "survivors": 0} for side in (q, d)]
    pos_q, pos_d = np.full(len(gs.cards), -1), np.full(len(gs.cards), -1)
    pos_q[q], pos_d[d] = np.arange(len(q)), np.arange(len(d))
    i, k = want["i"], want["k"]
    cross = (pos_q[i] >= 0) != (pos_q[k] >= 0)
    out = np.zeros(int(cross.sum()), dtype=PAIR_DTYPE)
    out["i"] = np.where(pos_q[i] >= 0, pos_q[i], pos_q[k])[cross]
    out["k"] = np.where(pos_q[i] >= 0, pos_d[k], pos_d[i])[cross]
    out["jaccard"] = want["jacc"][cross]
    out = out[np.lexsort((out["k"], out["i"]))]
    return out, {key: st[key] - inner[0][key] - inner[1][key] for key in ("evaluated", "survivors")}


def listed(got):
    return set(zip(got["i"].tolist(), got["k"].tolist()))


def check_forged_named(got, gs, accept):
    """inside sets: every forged pair is in the records; outside sets: none is"""
    have = listed(got)
    for a, b, c in gs.forged:
        assert ((a, b) in have) == accept, (a, b, c)


def load(sel, gs, p_aux=None):
    sel.upload(gs.hll, gs.aux, gs.cards)
    if p_aux is not None:
        sel.upload_aux_hll(gs.aux_hll, p_aux)


# ---- CB: cb_bounds_body ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cb_genome_sets(tau, accept):
    return [M.cb_genome_set(cs, seed=0xCB00 + t) for t, cs in enumerate(M.cb_sets(tau, accept))]


ALLPAIRS_ROUTES = {
    "sig": (ALGO_SIG, CRIT_SMH_A, {}),
    "stream": (ALGO_STREAM, CRIT_SMH_A, {}),
    "hashjoin": (ALGO_HASHJOIN, CRIT_SMH_A, {}),
    "small1": (ALGO_AUTO, CRIT_SMH_A, {"small_pass": 1}),                     # the one-launch pass: its own bounds and its own J test
    "small0": (ALGO_AUTO, CRIT_SMH_A, {"small_pass": 0}),
    "none-fused1": (ALGO_AUTO, CRIT_NONE, {"dense_fused": 1}),                # dense_select_kernel
    "none-fused0": (ALGO_AUTO, CRIT_NONE, {"dense_fused": 0}),
}


@pytest.mark.parametrize("route", list(ALLPAIRS_ROUTES))
@pytest.mark.parametrize("side", list(SIDES))
@pytest.mark.parametrize("tau", M.TAUS)
def test_cb_allpairs(oracle, tau, side, route):
    algo, crit, params = ALLPAIRS_ROUTES[route]
    accept = SIDES[side]
    with Selector(0) as sel:
        for name, value in params.items():
            sel.set_param(name, value)
        sel.set_criterion(crit)
        for gs in cb_genome_sets(tau, accept):
            want, wst = reference(oracle, gs, tau, True)
            load(sel, gs)
            got = sel.run(tau, MODE_CB_SMH, gs.r, gs.nb, algo=algo)
            st = sel.stats()
            print(f"tau {tau} {side} {route}: n {len(gs.cards)}, listed {len(got)} / {len(want)}, evaluated {st['evaluated']} / {wst['evaluated']}")
            assert_same_pairs(got, want)
            assert st["evaluated"] == wst["evaluated"] and st["survivors"] == wst["survivors"] and st["selected"] == len(want)
            check_forged_named(got, gs, accept)
            if "small_pass" in params:
                assert sel.get_param("small_pass_used") == params["small_pass"]
            if "dense_fused" in params:
                assert sel.get_param("dense_route_used") == params["dense_fused"]


@pytest.mark.parametrize("side", list(SIDES))
@pytest.mark.parametrize("tau", M.TAUS)
def test_cb_rectangle_and_row_shards(oracle, tau, side):
    """candidate_begin on the boundary rank (the forged partner is the rectangle's first candidate) and one past it; the parts of a
    row interleave"""
    accept = SIDES[side]
    gs = cb_genome_sets(tau, accept)[0]
    n = len(gs.cards)
    want, wst = reference(oracle, gs, tau, True)
    lo, hi = S.allpairs_windows(gs.cards, tau, True)
    assert int(S.window_mask(lo, hi, n).sum()) == wst["evaluated"]
    with Selector(0) as sel:
        load(sel, gs)
        for a, b, _ in gs.forged[:4]:
            for h in (b, b + 1):
                if h >= n:
                    continue
                sel.set_candidate_begin(h)
                got = sel.run(tau, MODE_CB_SMH, gs.r, gs.nb, rows=(0, h), algo=ALGO_SIG)
                exp = want[(want["i"] < h) & (want["k"] >= h)]
                assert_same_pairs(got, exp)
                ev = sum(max(0, int(hi[i]) - max(int(lo[i]), h) + 1) for i in range(h))
                assert sel.stats()["evaluated"] == ev
                assert ((a, b) in listed(got)) == (accept and h == b)
        sel.set_candidate_begin(0)
        parts, ev = [], 0
        for part in range(3):
            sel.set_row_interleave(32, 3, part)
            parts.append(sel.run(tau, MODE_CB_SMH, gs.r, gs.nb, algo=ALGO_SIG))
            ev += sel.stats()["evaluated"]
        cat = np.concatenate(parts)
        assert_same_pairs(cat[np.lexsort((cat["k"], cat["i"]))], want)
        assert ev == wst["evaluated"]


def test_cards_attached_on_the_device(oracle):
    """attach() validates nothing on the host: the forged cards as a device tensor give what upload() gives"""
    import torch
    dev = torch.device("cuda", 0)
    for accept in (True, False):
        gs = cb_genome_sets(0.9, accept)[0]
        want, wst = reference(oracle, gs, 0.9, True)
        t_hll, t_aux = torch.from_numpy(gs.hll).to(dev), torch.from_numpy(gs.aux.view(np.int64)).to(dev)
        t_cards = torch.from_numpy(gs.cards).to(dev)
        with Selector(0) as sel:
            sel.attach(t_hll, t_aux, t_cards)
            for algo in (ALGO_SIG, ALGO_STREAM):
                got = sel.run(0.9, MODE_CB_SMH, gs.r, gs.nb, algo=algo)
                assert_same_pairs(got, want)
                assert sel.stats()["evaluated"] == wst["evaluated"]
                check_forged_named(got, gs, accept)
            assert np.array_equal(sel.cards().view(np.uint64), gs.cards.view(np.uint64))


# ---- CB: query_windows_body ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["sig", "stream", "index"])
@pytest.mark.parametrize("side", list(SIDES))
@pytest.mark.parametrize("tau", M.TAUS)
def test_cb_queries(oracle, tau, side, route):
    """the clusters split between queries and database (decision_model.split_for_queries): the partner above and below P, at the first
    and the last database rank, queries below, equal to and above the database's boundary genome"""
    accept = SIDES[side]
    algo = {"sig": ALGO_SIG, "stream": ALGO_STREAM, "index": ALGO_INDEX}[route]
    with Selector(0) as sel:
        for gs, cs in zip(cb_genome_sets(tau, accept), M.cb_sets(tau, accept)):
            q, d = M.split_for_queries(cs)
            want, wst = cross_reference(oracle, gs, q, d, tau, True)
            sel.upload(gs.hll[d], gs.aux[d], gs.cards[d])
            sel.upload_queries(gs.hll[q], gs.aux[q], gs.cards[q])
            got = sel.run_queries(tau, MODE_CB_SMH, gs.r, gs.nb, algo=algo)
            st = sel.stats()
            print(f"tau {tau} {side} {route}: {len(q)} x {len(d)}, listed {len(got)} / {len(want)}, evaluated {st['evaluated']} / {wst['evaluated']}")
            assert_same(got, want)
            assert st["evaluated"] == wst["evaluated"] and st["survivors"] == wst["survivors"] and st["selected"] == len(want)
            # the forged pairs that the split separates, by name
            rank_q = {int(g): t for t, g in enumerate(q)}
            rank_d = {int(g): t for t, g in enumerate(d)}
            have, crossed = listed(got), 0
            for a, b, c in gs.forged:
                for x, y in ((a, b), (b, a)):
                    if x in rank_q and y in rank_d:
                        assert ((rank_q[x], rank_d[y]) in have) == accept, c
                        crossed += 1
            assert crossed >= 1


# ---- CB: the pair-list kernels -----------------------------------------------------------------------------------------------------
def boundary_list(gs, seed):
    """every forged pair in both orientations, the first repeated, among random entries"""
    rng = np.random.default_rng(seed)
    n = len(gs.cards)
    L = []
    for a, b, _ in gs.forged:
        L += [(a, b), (b, a), (a, b)]
    for _ in range(300):
        x, y = rng.choice(n, size=2, replace=False)
        L.append((int(x), int(y)))
    L = np.array(L, dtype=np.int32)
    return L[rng.permutation(len(L))]


def list_expectation(want, L, cards, tau):
    """one record per entry whose pair the all-pairs pass selects, sorted by (i, k); the entries inside the pair space"""
    j_of = {(int(w["i"]), int(w["k"])): w["jacc"] for w in want}
    lo, hi = S.allpairs_windows(cards, tau, True)
    mask = S.window_mask(lo, hi, len(cards))
    rec = sorted((min(x, y), max(x, y)) for x, y in L.tolist() if (min(x, y), max(x, y)) in j_of)
    out = np.zeros(len(rec), dtype=PAIR_DTYPE)
    for t, (i, k) in enumerate(rec):
        out[t] = (i, k, j_of[(i, k)])
    return out, int(sum(mask[min(x, y), max(x, y)] for x, y in L.tolist()))


@pytest.mark.parametrize("algo", [ALGO_SIG, ALGO_STREAM], ids=["sig", "direct"])
@pytest.mark.parametrize("side", list(SIDES))
@pytest.mark.parametrize("tau", M.TAUS)
def test_cb_pair_lists(oracle, tau, side, algo):
    accept = SIDES[side]
    with Selector(0) as sel:
        for t, gs in enumerate(cb_genome_sets(tau, accept)):
            want, _ = reference(oracle, gs, tau, True)
            L = boundary_list(gs, seed=t)
            exp, evaluated = list_expectation(want, L, gs.cards, tau)
            load(sel, gs)
            got = sel.run_pairs(L, tau, MODE_CB_SMH, gs.r, gs.nb, algo=algo)
            assert_same(got, exp)
            st = sel.stats()
            assert st["evaluated"] == evaluated and st["survivors"] == evaluated and st["selected"] == len(exp)
            have = listed(got)
            for a, b, c in gs.forged:
                assert ((a, b) in have) == accept, c
                entries = sum((min(x, y), max(x, y)) == (a, b) for x, y in L.tolist())      # both orientations, one repeated
                assert entries >= 3 and int(((got["i"] == a) & (got["k"] == b)).sum()) == (entries if accept else 0)


def run_launcher(fn, gs, pairs, tau, cnt_dtype):
    """a drop-in launcher on device copies of the set; -> sorted (x, y, float J) records"""
    import torch
    dev = torch.device("cuda", 0)
    lib = pkg.hip_lib()
    d_hll, d_aux = torch.from_numpy(gs.hll).to(dev), torch.from_numpy(gs.aux.view(np.int64)).to(dev)
    d_cards = torch.from_numpy(gs.cards).to(dev)
    n = len(gs.cards)
    total = n * (n - 1) // 2 if pairs is None else len(pairs)
    d_pairs = None if pairs is None else torch.from_numpy(pairs).to(dev)
    d_out = torch.zeros((total, 3), dtype=torch.int32, device=dev)
    d_cnt = torch.full((1,), -1, dtype=cnt_dtype, device=dev)
    rc = fn(d_hll.data_ptr(), d_aux.data_ptr(), d_cards.data_ptr(), None if pairs is None else d_pairs.data_ptr(), total, M.tau_double(tau),
            gs.aux.shape[1], 16384, gs.r, gs.nb, d_out.data_ptr(), d_cnt.data_ptr(), 256)
    assert rc == 0, lib.selhip_last_error(None)
    torch.cuda.synchronize()
    rec = d_out[:int(d_cnt.item())].cpu().numpy()
    return sorted((int(x), int(y), float(np.int32(s).view(np.float32))) for x, y, s in rec)


def launcher_expectation(want):
    with np.errstate(over="ignore"):
        return [(int(w["i"]), int(w["k"]), float(np.float32(w["jacc"]))) for w in want]


@pytest.mark.parametrize("side", list(SIDES))
@pytest.mark.parametrize("tau", M.TAUS)
def test_cb_launchers(oracle, tau, side):
    """launch_kernel_CBsmh(64) on the explicit triangle (pairs_direct_kernel's launcher form reads the cards itself) and on the
    implicit one"""
    import torch
    accept = SIDES[side]
    lib = pkg.hip_lib()
    gs = cb_genome_sets(tau, accept)[0]
    want, _ = reference(oracle, gs, tau, True)
    exp = launcher_expectation(want)
    ii, kk = np.triu_indices(len(gs.cards), 1)
    tri = np.stack([ii, kk], axis=1).astype(np.int32)
    for fn, pairs, cnt in ((lib.launch_kernel_CBsmh, tri, torch.int32), (lib.launch_kernel_CBsmh64, tri, torch.int64), (lib.launch_kernel_CBsmh, None, torch.int32)):
        got = run_launcher(fn, gs, pairs, tau, cnt)
        assert got == exp
        have = {(x, y) for x, y, _ in got}
        for a, b, c in gs.forged:
            assert ((a, b) in have) == accept, c


# ---- J >= tau --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _j_sets(tau, fp):
    import oracle_py
    oracle = oracle_py.Oracle()
    oracle.set_fma(fp)
    try:
        return M.j_genome_sets(oracle, tau, seed=0x1A + int(tau * 100))
    finally:
        oracle.set_fma(1)


@functools.lru_cache(maxsize=None)
def _j_low_sets(tau, fp):
    import oracle_py
    oracle = oracle_py.Oracle()
    oracle.set_fma(fp)
    try:
        return M.j_low_genome_sets(oracle, tau, seed=0x51 + int(tau * 100))
    finally:
        oracle.set_fma(1)


J_ROUTES = {
    "stage2-sig": (ALGO_SIG, CRIT_SMH_A, {"small_pass": 0}),                  # ertl_select_kernel
    "stage2-stream": (ALGO_STREAM, CRIT_SMH_A, {"small_pass": 0}),
    "small": (ALGO_AUTO, CRIT_SMH_A, {"small_pass": 1}),                      # small_pass_kernel: main registers below 32 (j_low_genome_sets)
    "dense": (ALGO_AUTO, CRIT_NONE, {"dense_fused": 1}),                      # dense_select_kernel
    "none-list": (ALGO_AUTO, CRIT_NONE, {"dense_fused": 0}),
}


# tau = 0.01: one J == tau at best (ulp(tau) = 2^-59), none below register 32: it runs through the routes that take high registers
J_CASES = [(tau, fp, route) for tau in J_TAUS + (0.01,) for fp in FPS for route in J_ROUTES if not (route == "small" and tau == 0.01)]


@pytest.mark.parametrize("tau,fp,route", J_CASES)
def test_j_allpairs(oracle, tau, fp, route):
    """J == tau exactly, the nearest J on either side, t = +inf (NaN: rejected) and t = 0 (+inf: accepted, +inf in the record); then the
    top-k cut behind the same pass with k above every genome's partners: nothing is cut"""
    algo, crit, params = J_ROUTES[route]
    inside, outside, _ = (_j_low_sets if route == "small" else _j_sets)(tau, FPS[fp])
    with Selector(0, FPS[fp]) as sel:
        for name, value in params.items():
            sel.set_param(name, value)
        sel.set_criterion(crit)
        for gs, accept in ((inside, True), (outside, False)):
            load(sel, gs)
            for mode, use_cb in ((MODE_CB_SMH, True), (MODE_SMH, False)):
                want, wst = reference(oracle, gs, tau, use_cb, fp=FPS[fp])
                sel.set_allpairs_topk(0)
                got = sel.run(tau, mode, gs.r, gs.nb, algo=algo)
                st = sel.stats()
                print(f"tau {tau} {fp} {route} {'inside' if accept else 'outside'} cb={use_cb}: listed {len(got)} / {len(want)}, survivors {st['survivors']}")
                assert_same_pairs(got, want)
                assert st["evaluated"] == wst["evaluated"] and st["survivors"] == wst["survivors"] and st["selected"] == len(want)
                check_forged_named(got, gs, accept)
                if "small_pass" in params:
                    assert sel.get_param("small_pass_used") == params["small_pass"]
                ranked = sel.run(tau, mode, gs.r, gs.nb, algo=algo, top_k=64)
                assert_same(ranked, nbr_reference(as_records(want), 64))
                assert len(ranked) == 2 * len(want)
            if accept:
                assert np.isposinf(got["jaccard"]).sum() == 1                # the pair of empty sketches


@pytest.mark.parametrize("tau", J_TAUS)
def test_j_launchers(oracle, tau):
    """compat_select_kernel (the explicit list) and the implicit triangle, without and with CB"""
    import torch
    lib = pkg.hip_lib()
    inside, outside, _ = _j_sets(tau, FP_FMA)
    for gs, accept in ((inside, True), (outside, False)):
        ii, kk = np.triu_indices(len(gs.cards), 1)
        tri = np.stack([ii, kk], axis=1).astype(np.int32)
        for use_cb, fns in ((False, (lib.launch_kernel_smh, lib.launch_kernel_smh64)), (True, (lib.launch_kernel_CBsmh, lib.launch_kernel_CBsmh64))):
            want, _ = reference(oracle, gs, tau, use_cb)
            exp = launcher_expectation(want)
            for fn, pairs, cnt in ((fns[0], tri, torch.int32), (fns[1], tri, torch.int64), (fns[0], None, torch.int32)):
                got = run_launcher(fn, gs, pairs, tau, cnt)
                assert got == exp
                have = {(x, y) for x, y, _ in got}
                for a, b, c in gs.forged:
                    assert ((a, b) in have) == accept, c


# ---- hll_a, hll_an, hll_a + smh_a ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _aux_sets(crit_name, tau, p_aux):
    import oracle_py
    return M.aux_genome_sets(oracle_py.Oracle(), crit_name, tau, p_aux)[0]


AUX_CRITS = {"hll_a": ("hll_a", CRIT_HLL_A), "hll_an": ("hll_an", CRIT_HLL_AN), "hll_a+smh_a": ("hll_a", CRIT_HLL_A_SMH_A)}


@pytest.mark.parametrize("fp", list(FPS))
@pytest.mark.parametrize("p_aux", [8, 4, 12])
@pytest.mark.parametrize("tau", [0.9, 0.5])
@pytest.mark.parametrize("crit_name", list(AUX_CRITS))
def test_aux_criteria(oracle, crit_name, tau, p_aux, fp):
    """K+ and J^ + C on and next to tau, in both flavours (the fused (1 + gamma) * e_hi - t+ decides some), (double)(e_lo + e_hi) where
    the sum is no double: all-pairs passes (aux_fused_kernel) and query passes (kernel_query_aux.cuh)"""
    model_crit, crit = AUX_CRITS[crit_name]
    sets = _aux_sets(model_crit, tau, p_aux)
    fma = 1 if FPS[fp] == FP_FMA else 0
    with Selector(0, FPS[fp]) as sel:
        for accept in (True, False):
            gs = sets[(fma, accept)]
            n = len(gs.cards)
            load(sel, gs, p_aux)
            sel.set_criterion(crit)
            for mode, use_cb in ((MODE_SMH, False), (MODE_CB_SMH, True)):
                want, wst = reference(oracle, gs, tau, use_cb, crit, FPS[fp], p_aux)
                got = sel.run(tau, mode, gs.r, gs.nb)
                st = sel.stats()
                print(f"{crit_name} tau {tau} p_aux {p_aux} {fp} accept={accept} cb={use_cb}: listed {len(got)} / {len(want)}, "
                      f"evaluated {st['evaluated']} / {wst['evaluated']}, survivors {st['survivors']} / {wst['survivors']}")
                assert_same_pairs(got, want)
                assert st["evaluated"] == wst["evaluated"] and st["survivors"] == wst["survivors"] and st["selected"] == len(want)
                if not use_cb:
                    check_forged_named(got, gs, accept)
            # queries: the smaller member of every other forged pair and the larger member of the rest
            is_q = np.zeros(n, dtype=bool)
            for t, (a, b, _) in enumerate(gs.forged):
                is_q[a if t % 2 == 0 else b] = True
            for a, b, _ in gs.forged:
                if is_q[a] and is_q[b]:                                      # (two cases can share a genome's rank order neighbours only)
                    is_q[b] = False
            q, d = np.nonzero(is_q)[0], np.nonzero(~is_q)[0]
            sel.upload(gs.hll[d], gs.aux[d], gs.cards[d])
            sel.upload_aux_hll(gs.aux_hll[d], p_aux)
            sel.upload_queries(gs.hll[q], gs.aux[q], gs.cards[q])
            sel.upload_queries_aux_hll(gs.aux_hll[q], p_aux)
            sel.set_criterion(crit)
            rank_q = {int(g): t for t, g in enumerate(q)}
            rank_d = {int(g): t for t, g in enumerate(d)}
            for mode, use_cb in ((MODE_SMH, False), (MODE_CB_SMH, True)):
                want, wst = cross_reference(oracle, gs, q, d, tau, use_cb, crit, FPS[fp], p_aux)
                got = sel.run_queries(tau, mode, gs.r, gs.nb)
                st = sel.stats()
                assert_same(got, want)
                assert st["evaluated"] == wst["evaluated"] and st["survivors"] == wst["survivors"] and st["selected"] == len(want)
                if not use_cb:
                    have, crossed = listed(got), 0
                    for a, b, c in gs.forged:
                        for x, y in ((a, b), (b, a)):
                            if x in rank_q and y in rank_d:
                                assert ((rank_q[x], rank_d[y]) in have) == accept, c
                                crossed += 1
                    assert crossed >= 1
