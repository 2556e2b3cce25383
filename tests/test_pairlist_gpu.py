"""Pair-list passes on the GPU (selhip_ctx_run_pairs, include/selection_hip.h section 2e): the context's criterion over a caller's list
of pairs.  Let E be the pair space of the all-pairs pass over all rows and S its result; a list pass must return one record
{min, max, J of S} for every entry whose pair is in S -- with multiplicity -- and count entries in its statistics.

Expected values come from the oracle and tests/sig_model.py only: S from oracle.select; E per entry from the truncated cards and
orc_cb; the entries that pass a criterion from the oracle's predicates (smh_a: the literal band comparison; the auxiliary criteria:
the oracle's pair list over primary sketches that are all one row, where the final Jaccard test passes every pair, checked against
the survivor count of the real run); the signature route's candidates from sig_model.band_sigs."""
import subprocess

import numpy as np
import pytest

import sig_model as S
from conftest import GOLDEN, ROOT
from test_exhaustive_host import flat_oracle_select
from test_gpu_parity import sorted_set
from test_query_aux_gpu import CFG_AUX
from test_sig_collisions_gpu import FORBIDDEN, N as N_PLANTED, RUNS, SHAPE_IDS, case

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import (ALGO_AUTO, ALGO_HASHJOIN, ALGO_INDEX, ALGO_SIG, ALGO_STREAM, CRIT_HLL_A, CRIT_HLL_A_SMH_A, CRIT_HLL_AN,
                                         CRIT_NONE, CRIT_SMH_A, FP_FMA, FP_STRICT, MODE_CB_SMH, MODE_SMH, PAIR_DTYPE, SelhipError, Selector,
                                         SynthConfig)

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
EXP = GOLDEN / "expected"
E_BADARG, E_STATE = -1, -5
CRITS = {"smh_a": CRIT_SMH_A, "hll_a": CRIT_HLL_A, "hll_an": CRIT_HLL_AN, "hll_a+smh_a": CRIT_HLL_A_SMH_A, "none": CRIT_NONE}
ORC_CRIT = {CRIT_SMH_A: 0, CRIT_HLL_A: 1, CRIT_HLL_AN: 2, CRIT_HLL_A_SMH_A: 3}
_CACHE = {}


def test_error_codes():
    header = (ROOT / "include" / "selection_hip.h").read_text()
    assert "#define SELHIP_E_BADARG" in header and "#define SELHIP_E_STATE" in header
    import re
    assert int(re.search(r"#define SELHIP_E_BADARG\s+(-?\d+)", header).group(1)) == E_BADARG
    assert int(re.search(r"#define SELHIP_E_STATE\s+(-?\d+)", header).group(1)) == E_STATE


# ---- the reference of a list --------------------------------------------------------------------------------------------------
def sig_ok(r, nb):
    return r & (r - 1) == 0 and nb in (8, 16, 32, 64, 128)


def in_E(oracle, cards, tau, use_cb, lo, hi):
    """bool per entry (lo < hi, ranks): e_hi != 0 and, under CB, orc_cb(tau, e_lo, e_hi)"""
    e = S.trunc_cards(cards)
    tau_d = float(np.float32(tau))
    out = e[hi] != 0
    if use_cb:
        out &= np.array([bool(oracle.lib.orc_cb(tau_d, float(e[a]), float(e[b]))) for a, b in zip(lo.tolist(), hi.tolist())], dtype=bool)
    return out


def records_of(S_dict, lo, hi):
    """the entries of the list found in S, with multiplicity, sorted by (i, k)"""
    hit = [(a, b, S_dict[(a, b)]) for a, b in zip(lo.tolist(), hi.tolist()) if (a, b) in S_dict]
    hit.sort(key=lambda t: (t[0], t[1]))
    out = np.zeros(len(hit), dtype=PAIR_DTYPE)
    if hit:
        out["i"], out["k"], out["jaccard"] = zip(*hit)
    return out


def assert_same(got, want):
    assert got.shape[0] == want.shape[0], (got.shape[0], want.shape[0])
    assert np.array_equal(got["i"], want["i"]) and np.array_equal(got["k"], want["k"])
    assert np.array_equal(got["jaccard"].view(np.uint64), want["jaccard"].view(np.uint64))


def as_dict(pairs, key="jacc"):
    return {(int(i), int(k)): float(j) for i, k, j in zip(pairs["i"], pairs["k"], pairs[key])}


def make_list(S_keys, n, n_random, n_repeat, seed):
    """every pair of S in random orientation + n_random uniformly random valid entries + n_repeat repeats drawn from the whole (one more
    where the length would come out as a multiple of the 64 lanes of a wave), shuffled"""
    rng = np.random.default_rng(seed)
    base = np.array(sorted(S_keys), dtype=np.int32).reshape(-1, 2)
    flip = rng.random(len(base)) < 0.5
    base[flip] = base[flip][:, ::-1]
    x = rng.integers(0, n, n_random, dtype=np.int32)
    y = (x + rng.integers(1, n, n_random, dtype=np.int32)) % n              # never x
    L = np.concatenate([base, np.stack([x, y], axis=1).astype(np.int32)])
    if (len(L) + n_repeat) % 64 == 0:
        n_repeat += 1                                                         # the length is never a multiple of 64 (or 512)
    L = np.concatenate([L, L[rng.integers(0, len(L), n_repeat)]])
    rng.shuffle(L)
    return np.ascontiguousarray(L, dtype=np.int32)


class Ref:
    """one synthetic set (with auxiliary HLL sketches) in rank order under an estimator flavour, and what passes over it must give"""

    def __init__(self, oracle, cfg_name, fp):
        self.oracle, self.fp = oracle, fp
        self.hll, self.aux, self.cards, _, self.aux_hll = sorted_set(CFG_AUX[cfg_name], oracle, fp)
        self.n, self.m = self.aux.shape
        self._sel, self._lit, self._sig, self._pass = {}, {}, {}, {}

    def select(self, crit, tau, use_cb, r, nb):
        """(S as a dict, the oracle's statistics) of the all-pairs pass"""
        key = (crit, tau, use_cb)
        if key not in self._sel:
            if crit == CRIT_NONE:
                pairs, st = flat_oracle_select(self.oracle, self.hll, self.cards, tau, use_cb, self.fp)
                self._sel[key] = (as_dict(pairs, "jaccard"), st)
            else:
                self.oracle.set_fma(self.fp)
                try:
                    pairs, st = self.oracle.select(self.hll, self.aux, self.cards, tau, r, nb, use_cb=use_cb, criterion=ORC_CRIT[crit],
                                                   aux_hll=self.aux_hll, p_aux=8)
                finally:
                    self.oracle.set_fma(1)
                self._sel[key] = (as_dict(pairs), st)
        return self._sel[key]

    def literal(self, r, nb):
        if (r, nb) not in self._lit:
            self._lit[(r, nb)] = S.literal_matrix(self.aux, self.aux, r, nb)
        return self._lit[(r, nb)]

    def sig_match(self, r, nb):
        if (r, nb) not in self._sig:
            sg = S.band_sigs(self.aux, r, nb)
            self._sig[(r, nb)] = S.sig_match_matrix(sg, sg)
        return self._sig[(r, nb)]

    def passing(self, crit, tau, use_cb, r, nb):
        """the pairs of E that pass an auxiliary criterion, as a set: the oracle's pair list over primary sketches that are all the
        smallest genome's row -- the union estimate t is then its cardinality, e_i + e_k - t >= t - 2, and J >= 1 - 2 / t passes tau"""
        key = (crit, tau, use_cb)
        if key not in self._pass:
            assert self.cards[0] > 1000 and tau < 0.95
            flat = np.repeat(self.hll[:1], self.n, axis=0)
            self.oracle.set_fma(self.fp)
            try:
                pairs, st = self.oracle.select(flat, self.aux, self.cards, tau, r, nb, use_cb=use_cb, criterion=ORC_CRIT[crit],
                                               aux_hll=self.aux_hll, p_aux=8)
            finally:
                self.oracle.set_fma(1)
            assert len(pairs) == st["survivors"] == self.select(crit, tau, use_cb, r, nb)[1]["survivors"]
            self._pass[key] = set(zip(pairs["i"].tolist(), pairs["k"].tolist()))
        return self._pass[key]


def ref(oracle, cfg_name, fp):
    if (cfg_name, fp) not in _CACHE:
        _CACHE[(cfg_name, fp)] = Ref(oracle, cfg_name, fp)
    return _CACHE[(cfg_name, fp)]


def loaded(R, crit, **params):
    sel = Selector(0, R.fp)
    for name, value in params.items():
        sel.set_param(name, value)
    sel.upload(R.hll, R.aux, R.cards)
    sel.upload_aux_hll(R.aux_hll, 8)
    sel.set_criterion(crit)
    return sel


# ---- 1. criteria x routes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crit_name", list(CRITS))
@pytest.mark.parametrize("tau", [0.9, 0.5])
@pytest.mark.parametrize("mode", [MODE_CB_SMH, MODE_SMH], ids=["cb", "smh"])
@pytest.mark.parametrize("fp", [FP_FMA, FP_STRICT], ids=["fma", "strict"])
@pytest.mark.parametrize("cfg_name", ["cfg2", "cfg2-spread"])
def test_criteria_and_routes(oracle, cfg_name, fp, mode, tau, crit_name):
    R, crit, use_cb = ref(oracle, cfg_name, fp), CRITS[crit_name], mode == MODE_CB_SMH
    r, nb = pkg.banding(R.m, tau)
    S_dict, _ = R.select(crit, tau, use_cb, r, nb)
    L = make_list(S_dict, R.n, 20011, 500, seed=int(tau * 10) + 100 * mode + 1000 * fp + 7 * crit)
    assert len(L) % 64 and len(L) % 512
    lo, hi = L.min(axis=1), L.max(axis=1)
    want = records_of(S_dict, lo, hi)
    inE = in_E(oracle, R.cards, tau, use_cb, lo, hi)
    assert len(want) > 0 and any((a, b) not in S_dict for a, b in zip(lo.tolist(), hi.tolist()))
    if cfg_name == "cfg2-spread" and use_cb:
        assert not inE.all()                                                  # entries outside E
    smh = crit in (CRIT_SMH_A, CRIT_HLL_A_SMH_A)
    if crit == CRIT_NONE:
        passed = int(inE.sum())
    elif crit == CRIT_SMH_A:
        passed = int((inE & R.literal(r, nb)[lo, hi]).sum())
    else:
        ok = R.passing(crit, tau, use_cb, r, nb)
        passed = sum(1 for a, b, e in zip(lo.tolist(), hi.tolist(), inE.tolist()) if e and (a, b) in ok)
    if crit == CRIT_SMH_A and cfg_name == "cfg2" and tau == 0.9:
        # entries that reach tau and fail the criterion exist: they are listed (L holds the exhaustive result's pairs) and not reported
        S_none, _ = R.select(CRIT_NONE, tau, use_cb, 1, 1)
        assert len(S_none) > len(S_dict)
        L = np.ascontiguousarray(np.concatenate([L, np.array(sorted(set(S_none) - set(S_dict)), dtype=np.int32)]))
        lo, hi = L.min(axis=1), L.max(axis=1)
        extra = in_E(oracle, R.cards, tau, use_cb, lo, hi)
        passed = int((extra & R.literal(r, nb)[lo, hi]).sum())
        inE = extra
    routes = [(ALGO_SIG, 1), (ALGO_STREAM, 0), (ALGO_AUTO, 1 if sig_ok(r, nb) else 0)] if smh else [(ALGO_AUTO, 2)]
    with loaded(R, crit) as sel:
        assert sel.get_param("pairs_route_used") == -1
        for algo, route in routes:
            if algo == ALGO_SIG and not sig_ok(r, nb):
                with pytest.raises(SelhipError, match="ALGO_SIG needs") as ei:
                    sel.run_pairs(L, tau, mode, r, nb, algo=algo)
                assert ei.value.code == E_BADARG
                continue
            got = sel.run_pairs(L, tau, mode, r, nb, algo=algo)
            st = sel.stats()
            print(f"{cfg_name} fp={fp} mode={mode} tau={tau} {crit_name} algo={algo}: P={len(L)} records {len(got)} / {len(want)} stats {st} "
                  f"in E {int(inE.sum())} passed {passed}")
            assert_same(got, want)
            assert sel.get_param("pairs_route_used") == route
            assert st["evaluated"] == int(inE.sum()) and st["survivors"] == passed and st["selected"] == len(want)
            if route == 1:
                assert st["candidates"] == int((inE & R.sig_match(r, nb)[lo, hi]).sum())
            elif crit == CRIT_NONE:
                assert st["candidates"] == st["evaluated"]
            elif route == 0 and crit == CRIT_SMH_A:
                assert st["candidates"] == passed
            assert sel.get_param("chunks") == 1 and sel.get_param("small_pass_used") == 0 and sel.last_attempts() >= 1


# ---- 2. the whole triangle as a list, on forged signature collisions ------------------------------------------------------------
@pytest.mark.parametrize("route", ["sig", "sig-fb", "direct"])
@pytest.mark.parametrize("m,r,nb", S.SHAPES, ids=SHAPE_IDS)
def test_whole_triangle_with_forged_collisions(oracle, m, r, nb, route):
    """the only test that shows pairs_verify_kernel a signature collision: every class of tests/sig_model.py's planted set"""
    c = case(oracle, m, r, nb)
    n = N_PLANTED
    ii, kk = np.triu_indices(n, 1)
    L = np.ascontiguousarray(np.stack([kk, ii], axis=1)[np.random.default_rng(r).permutation(len(ii))], dtype=np.int32)   # larger rank first
    assert len(L) == 19900
    algo = ALGO_STREAM if route == "direct" else ALGO_SIG
    with Selector(0) as sel:
        sel.set_param("verify_fb", 1 if route == "sig-fb" else 0)
        sel.upload(c.hll, c.aux, c.cards)
        for run in RUNS:
            tau, mode, _ = RUNS[run]
            want, _, survivors, cand = c.expect(run)
            sel.run(tau, mode, c.r, c.nb, algo=algo)
            st_all = sel.stats()
            got = sel.run_pairs(L, tau, mode, c.r, c.nb, algo=algo)
            st = sel.stats()
            print(f"{r}x{nb} {route} {run}: listed {len(got)} / {len(want)} stats {st} all-pairs {st_all} model candidates {cand}")
            assert sel.get_param("pairs_route_used") == (0 if route == "direct" else 1)
            assert np.array_equal(got["i"], want["i"]) and np.array_equal(got["k"], want["k"])
            assert np.array_equal(got["jaccard"].view(np.uint64), want["jacc"].view(np.uint64))
            listed = set(zip(got["i"].tolist(), got["k"].tolist()))
            assert len(listed) == len(got)                                    # no pair twice
            assert not listed & set(c.P.of(*FORBIDDEN))
            if run == "smh":
                assert set(c.P.of("C2", "C3")) <= listed
            assert st == st_all
            assert st["survivors"] == survivors
            if route != "direct":
                assert st["candidates"] == cand


# ---- 3. band shapes the join does not take: the direct route only ----------------------------------------------------------------
ODD_SHAPES = [(256, 64, 4), (256, 1, 256), (96, 3, 32), (96, 24, 4), (68, 17, 4)]


@pytest.mark.parametrize("m,r,nb", ODD_SHAPES, ids=[f"{r}x{nb}" for _, r, nb in ODD_SHAPES])
def test_direct_route_any_band_shape(oracle, m, r, nb):
    n = 300
    if "odd-hll" not in _CACHE:
        hll, _, cards, _, _ = sorted_set(SynthConfig("pairlist-shapes", n, 128, 0.9, 0x5EED0C03, mode=1, n_sh_lo=3000, n_sh_hi=40000), oracle)
        _CACHE["odd-hll"] = (hll, cards)
    hll, cards = _CACHE["odd-hll"]
    rng = np.random.default_rng(m * 1000 + r)
    aux = rng.integers(0, 1 << 64, size=(n, m), dtype=np.uint64)
    straddling = [b for b in range(nb) if (b * r) // 16 != (b * r + r - 1) // 16]
    plant = {"first": 0, "last": nb - 1}
    if straddling:
        plant["straddle"] = straddling[len(straddling) // 2]
    planted, near = {}, {}
    g = 0
    for name, band in plant.items():
        a, b = g, g + 1
        aux[b, band * r:(band + 1) * r] = aux[a, band * r:(band + 1) * r]
        planted[name] = (a, b)
        a, b = g + 2, g + 3                                                   # the same band equal in all but its last bucket
        aux[b, band * r:(band + 1) * r - 1] = aux[a, band * r:(band + 1) * r - 1]
        near[name] = (a, b)
        g += 4
    ii, kk = np.triu_indices(n, 1)
    L = np.stack([ii, kk], axis=1).astype(np.int32)
    flip = rng.random(len(L)) < 0.5
    L[flip] = L[flip][:, ::-1]
    L = np.ascontiguousarray(L[rng.permutation(len(L))])
    lo, hi = L.min(axis=1), L.max(axis=1)
    passes = np.array([oracle.smh_a(aux[a], aux[b], r, nb) for a, b in zip(lo.tolist(), hi.tolist())], dtype=bool)
    for name in plant:
        assert oracle.smh_a(aux[planted[name][0]], aux[planted[name][1]], r, nb), name
        assert r == 1 or not oracle.smh_a(aux[near[name][0]], aux[near[name][1]], r, nb), name
    tau = -1.0                                                                # J >= -1 always: every survivor is a record
    want, wst = oracle.select(hll, aux, cards, tau, r, nb, use_cb=False)
    assert wst["survivors"] == int(passes.sum()) == len(want) >= len(plant)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        with pytest.raises(SelhipError, match="ALGO_SIG needs") as ei:
            sel.run_pairs(L, tau, MODE_SMH, r, nb, algo=ALGO_SIG)
        assert ei.value.code == E_BADARG
        for algo in (ALGO_STREAM, ALGO_AUTO):
            got = sel.run_pairs(L, tau, MODE_SMH, r, nb, algo=algo)
            st = sel.stats()
            print(f"{r}x{nb} algo={algo}: {st} want {len(want)}")
            assert sel.get_param("pairs_route_used") == 0
            assert_same(got, records_of(as_dict(want), lo, hi))
            assert st == {"evaluated": len(L), "survivors": int(passes.sum()), "selected": len(want), "candidates": int(passes.sum())}
            listed = set(zip(got["i"].tolist(), got["k"].tolist()))
            assert set(planted.values()) <= listed and (r == 1 or not set(near.values()) & listed)


# ---- 4. list lengths and contents ---------------------------------------------------------------------------------------------
def smh_case(oracle, tau=0.9, mode=MODE_CB_SMH, cfg_name="cfg2"):
    R = ref(oracle, cfg_name, FP_FMA)
    r, nb = pkg.banding(R.m, tau)
    S_dict, st = R.select(CRIT_SMH_A, tau, mode == MODE_CB_SMH, r, nb)
    return R, r, nb, S_dict, st


def check_list(sel, oracle, R, S_dict, L, tau, mode, r, nb, algo):
    L = np.ascontiguousarray(L, dtype=np.int32).reshape(-1, 2)
    lo, hi = L.min(axis=1), L.max(axis=1)
    want = records_of(S_dict, lo, hi)
    got = sel.run_pairs(L, tau, mode, r, nb, algo=algo)
    st = sel.stats()
    assert_same(got, want)
    inE = in_E(oracle, R.cards, tau, mode == MODE_CB_SMH, lo, hi) if len(L) else np.zeros(0, dtype=bool)
    assert st["evaluated"] == int(inE.sum()) and st["selected"] == len(want)
    if sel.criterion == CRIT_SMH_A:
        assert st["survivors"] == int((inE & R.literal(r, nb)[lo, hi]).sum())
    return got


@pytest.mark.parametrize("algo", [ALGO_SIG, ALGO_STREAM], ids=["sig", "direct"])
def test_list_lengths(oracle, algo):
    R, r, nb, S_dict, _ = smh_case(oracle)
    tau, mode = 0.9, MODE_CB_SMH
    full = make_list(S_dict, R.n, 3000, 100, seed=41)
    with loaded(R, CRIT_SMH_A) as sel:
        n_rec = []
        for P in (0, 1, 63, 64, 65, 511, 512, 513, 1025):
            got = check_list(sel, oracle, R, S_dict, full[:P], tau, mode, r, nb, algo)
            n_rec.append(len(got))
            if P == 0:
                assert sel.stats() == {"evaluated": 0, "survivors": 0, "selected": 0, "candidates": 0} and sel.last_attempts() == 1
        assert n_rec[0] == 0 and n_rec[-1] > 0
        # the first entry of S at every position of a block's first and last wave
        first = np.array(sorted(S_dict)[0], dtype=np.int32)
        for pos in (0, 63, 64, 447, 448, 511, 512):
            L = full[1025:1625].copy()
            L[pos] = first
            got = check_list(sel, oracle, R, S_dict, L, tau, mode, r, nb, algo)
            assert (int(first[0]), int(first[1])) in set(zip(got["i"].tolist(), got["k"].tolist()))


@pytest.mark.parametrize("algo", [ALGO_SIG, ALGO_STREAM], ids=["sig", "direct"])
def test_repeats_rows_and_columns(oracle, algo):
    R, r, nb, S_dict, _ = smh_case(oracle)
    tau, mode = 0.9, MODE_CB_SMH
    keys = sorted(S_dict)
    with loaded(R, CRIT_SMH_A) as sel:
        # one selected pair listed 1 000 times: 1 000 equal records
        one = keys[len(keys) // 2]
        L = np.tile(np.array([one[1], one[0]], dtype=np.int32), (1000, 1))
        got = check_list(sel, oracle, R, S_dict, L, tau, mode, r, nb, algo)
        assert len(got) == 1000 and set(zip(got["i"].tolist(), got["k"].tolist())) == {one}
        assert len(set(got["jaccard"].view(np.uint64).tolist())) == 1
        assert sel.stats()["evaluated"] == 1000 and sel.stats()["survivors"] == 1000
        # every entry in one row: the row with the most partners in S against every other genome
        rows = np.bincount([i for i, _ in keys], minlength=R.n)
        i = int(rows.argmax())
        L = np.array([[i, k] for k in range(R.n) if k != i], dtype=np.int32)
        got = check_list(sel, oracle, R, S_dict, L, tau, mode, r, nb, algo)
        assert len(got) >= rows[i] > 0
        # every entry with the same larger member
        k = int(np.bincount([k for _, k in keys], minlength=R.n).argmax())
        L = np.array([[k, x] for x in range(k)], dtype=np.int32)
        got = check_list(sel, oracle, R, S_dict, L, tau, mode, r, nb, algo)
        assert len(got) > 0 and np.all(got["k"] == k)


@pytest.mark.parametrize("crit_name", ["smh_a", "none"])
def test_empty_sketches_outside_E(oracle, crit_name):
    """empty sketches (e = 0) take the first ranks: an entry of two of them is outside E whatever the mode"""
    cfg = CFG_AUX["cfg2-spread"]
    hll, aux, ah = pkg.synth_host(cfg, g_range=(0, 150))
    hll[:40] = 0
    cards = oracle.cards(hll)
    perm = pkg.sort_by_card(cards)
    hll, aux, ah, cards = hll[perm], aux[perm], ah[perm], cards[perm]
    assert np.all(cards[:40] == 0) and cards[40] > 0
    ii, kk = np.triu_indices(40, 1)
    L = np.ascontiguousarray(np.stack([kk, ii], axis=1), dtype=np.int32)      # 780 entries, all among the empty sketches
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        sel.set_criterion(CRITS[crit_name])
        for mode in (MODE_SMH, MODE_CB_SMH):
            for algo in ((ALGO_SIG, ALGO_STREAM) if crit_name == "smh_a" else (ALGO_AUTO,)):
                got = sel.run_pairs(L, 0.0, mode, 8, 32, algo=algo)
                assert len(got) == 0
                assert sel.stats() == {"evaluated": 0, "survivors": 0, "selected": 0, "candidates": 0}
        # one empty sketch against a non-empty one IS in E without CB
        got = sel.run_pairs(np.array([[100, 3]], dtype=np.int32), -1.0, MODE_SMH, 8, 32)
        assert sel.stats()["evaluated"] == 1


# ---- 5. invalid entries -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", [ALGO_SIG, ALGO_STREAM], ids=["sig", "direct"])
def test_invalid_entries(oracle, algo):
    R, r, nb, S_dict, st_all = smh_case(oracle)
    tau, mode = 0.9, MODE_CB_SMH
    good = make_list(S_dict, R.n, 1000, 0, seed=5)[:1000]
    bad = {"x == y": (17, 17), "x == n": (R.n, 3), "y == -1": (5, -1)}
    with loaded(R, CRIT_SMH_A) as sel:
        for what, entry in bad.items():
            for pos in (0, 500, 999):
                L = good.copy()
                L[pos] = entry
                with pytest.raises(SelhipError) as ei:
                    sel.run_pairs(L, tau, mode, r, nb, algo=algo)
                assert ei.value.code == E_BADARG, (what, pos)
                assert "1 invalid entries" in str(ei.value) and f"entry {pos} is one" in str(ei.value), str(ei.value)
                with pytest.raises(SelhipError) as ei:
                    sel.stats()
                assert ei.value.code == E_STATE
                with pytest.raises(SelhipError):
                    sel.fetch()
        # several: the count is exact, the index is one of them
        L = good.copy()
        L[[3, 600, 998]] = [(0, 0), (R.n + 5, 1), (-3, 2)]
        with pytest.raises(SelhipError, match="3 invalid entries") as ei:
            sel.run_pairs(L, tau, mode, r, nb, algo=algo)
        assert any(f"entry {p} is one" in str(ei.value) for p in (3, 600, 998))
        # the same context then runs a valid list and an all-pairs pass correctly
        check_list(sel, oracle, R, S_dict, good, tau, mode, r, nb, algo)
        got = sel.run(tau, mode, r, nb)
        assert as_dict(got, "jaccard") == S_dict
        assert sel.stats()["evaluated"] == st_all["evaluated"] and sel.stats()["survivors"] == st_all["survivors"]
    # the hll_a filter kernel reports them too
    with loaded(R, CRIT_HLL_A) as sel:
        L = good.copy()
        L[999] = (R.n, 0)
        with pytest.raises(SelhipError, match="entry 999 is one"):
            sel.run_pairs(L, tau, mode, r, nb)


# ---- 6. growth ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crit_name,algo", [("smh_a", ALGO_SIG), ("smh_a", ALGO_STREAM), ("hll_a+smh_a", ALGO_SIG), ("hll_an", ALGO_AUTO), ("none", ALGO_AUTO)])
def test_lists_grow_and_the_pass_repeats(oracle, crit_name, algo):
    import torch
    crit = CRITS[crit_name]
    R = ref(oracle, "cfg2", FP_FMA)
    tau, mode = 0.9, MODE_CB_SMH
    r, nb = pkg.banding(R.m, tau)
    S_dict, _ = R.select(crit, tau, True, r, nb)
    L = make_list(S_dict, R.n, 5000, 50, seed=6)
    want = records_of(S_dict, L.min(axis=1), L.max(axis=1))
    t = torch.from_numpy(L).to("cuda")
    with loaded(R, crit, init_cap=1, enum_pairs=1500) as sel:
        got = sel.run_pairs(t, tau, mode, r, nb, algo=algo)
        assert sel.last_attempts() > 1
        assert_same(got, want)
        assert np.array_equal(t.cpu().numpy(), L)                             # the caller's list was read again, not written
        got = sel.run_pairs(t, tau, mode, r, nb, algo=algo)                   # the lists have grown: one attempt now
        assert sel.last_attempts() == 1
        assert_same(got, want)
        dev_ptr, cnt = sel.result_device()
        assert cnt == len(want) and dev_ptr
        out = torch.zeros(len(want) * 16, dtype=torch.uint8, device="cuda")
        assert sel.copy_results_to(out) == len(want)
        torch.cuda.synchronize()
        rec = np.sort(out.cpu().numpy().view(PAIR_DTYPE), order=["i", "k"])
        assert np.array_equal(rec["i"], want["i"]) and np.array_equal(rec["k"], want["k"])


# ---- 7. state -----------------------------------------------------------------------------------------------------------------
def test_refusals(oracle):
    R, r, nb, S_dict, _ = smh_case(oracle)
    tau, mode = 0.9, MODE_CB_SMH
    L = make_list(S_dict, R.n, 100, 0, seed=7)
    with Selector(0) as sel:
        with pytest.raises(SelhipError) as ei:                                # before upload
            sel.run_pairs(L, tau, mode, r, nb)
        assert ei.value.code == E_STATE
    with loaded(R, CRIT_SMH_A) as sel:
        sel.run_pairs_async(L, tau, mode, r, nb)                              # while pending
        with pytest.raises(SelhipError, match="pending") as ei:
            sel.run_pairs_async(L, tau, mode, r, nb)
        assert ei.value.code == E_STATE
        sel.finish()
        assert_same(sel.fetch(), records_of(S_dict, L.min(axis=1), L.max(axis=1)))
        sel.set_allpairs_topk(3)
        with pytest.raises(SelhipError, match="top-k") as ei:
            sel.run_pairs(L, tau, mode, r, nb)
        assert ei.value.code == E_STATE
        sel.set_allpairs_topk(0)
        sel.set_row_interleave(32, 2, 1)
        with pytest.raises(SelhipError, match="interleave") as ei:
            sel.run_pairs(L, tau, mode, r, nb)
        assert ei.value.code == E_STATE
        sel.set_row_interleave(32, 1, 0)
        sel.set_candidate_begin(10)
        with pytest.raises(SelhipError, match="candidate begin") as ei:
            sel.run_pairs(L, tau, mode, r, nb)
        assert ei.value.code == E_STATE
        sel.set_candidate_begin(0)
        for algo in (ALGO_HASHJOIN, ALGO_INDEX, 9):
            with pytest.raises(SelhipError) as ei:
                sel.run_pairs(L, tau, mode, r, nb, algo=algo)
            assert ei.value.code == E_BADARG
        for kw in (dict(mode=7), dict(n_rows=3, n_bands=5)):
            with pytest.raises(SelhipError) as ei:
                sel.run_pairs(L, tau, **{"mode": mode, "n_rows": r, "n_bands": nb, **kw})
            assert ei.value.code == E_BADARG
        check_list(sel, oracle, R, S_dict, L, tau, mode, r, nb, ALGO_AUTO)    # after all the refusals
    with Selector(0) as sel:                                                  # an auxiliary criterion without auxiliary sketches
        sel.upload(R.hll, R.aux, R.cards)
        for crit in (CRIT_HLL_A, CRIT_HLL_AN, CRIT_HLL_A_SMH_A):
            sel.set_criterion(crit)
            with pytest.raises(SelhipError, match="auxiliary HLL") as ei:
                sel.run_pairs(L, tau, mode, r, nb)
            assert ei.value.code == E_STATE


def test_auto_route_rule(oracle):
    """ALGO_AUTO: the signature route from n / 2 entries on, or when the signatures are cached"""
    R, r, nb, S_dict, _ = smh_case(oracle)
    assert sig_ok(r, nb)
    tau, mode = 0.9, MODE_CB_SMH
    L = make_list(S_dict, R.n, 100, 0, seed=8)
    with loaded(R, CRIT_SMH_A) as sel:
        for P, route in ((R.n // 2 - 1, 0), (R.n // 2, 1)):
            check_list(sel, oracle, R, S_dict, L[:P], tau, mode, r, nb, ALGO_AUTO)
            assert sel.get_param("pairs_route_used") == route
        sel.set_param("sig_cache", 1)
        check_list(sel, oracle, R, S_dict, L[:10], tau, mode, r, nb, ALGO_AUTO)
        assert sel.get_param("pairs_route_used") == 0                         # nothing cached yet
        sel.timing(1)
        check_list(sel, oracle, R, S_dict, L[:10], tau, mode, r, nb, ALGO_SIG)   # builds and leaves the signatures behind
        check_list(sel, oracle, R, S_dict, L[:10], tau, mode, r, nb, ALGO_AUTO)
        assert sel.get_param("pairs_route_used") == 1
        assert sel.kernel_ms("stage1") > 0
        sel.timing(0)


@pytest.mark.parametrize("sig_cache", [0, 1])
def test_passes_of_other_kinds_in_between(oracle, sig_cache):
    """list pass -> all-pairs pass -> list pass -> query pass on one context, each equal to what a fresh context gives"""
    R, r, nb, S_dict, st_all = smh_case(oracle)
    tau, mode = 0.9, MODE_CB_SMH
    L = make_list(S_dict, R.n, 2000, 20, seed=9)
    nq = 100

    def fresh(fn):
        with loaded(R, CRIT_SMH_A, sig_cache=sig_cache) as s:
            s.upload_queries(R.hll[:nq], R.aux[:nq], R.cards[:nq])
            out = fn(s)
            return out, s.stats()

    steps = [lambda s: s.run_pairs(L, tau, mode, r, nb, algo=ALGO_SIG),
             lambda s: s.run(tau, mode, r, nb),
             lambda s: s.run_pairs(L[::-1].copy(), tau, mode, r, nb, algo=ALGO_AUTO),
             lambda s: s.run_queries(tau, mode, r, nb),
             lambda s: s.run_pairs(L, tau, mode, r, nb, algo=ALGO_STREAM),
             lambda s: s.run(tau, mode, r, nb)]
    wants = [fresh(fn) for fn in steps]
    assert as_dict(wants[1][0], "jaccard") == S_dict and wants[1][1]["evaluated"] == st_all["evaluated"]
    assert len(wants[3][0]) > 0
    with loaded(R, CRIT_SMH_A, sig_cache=sig_cache) as sel:
        sel.upload_queries(R.hll[:nq], R.aux[:nq], R.cards[:nq])
        for step, (fn, (want, wst)) in enumerate(zip(steps, wants)):
            got = fn(sel)
            assert_same(got, want), step
            assert sel.stats() == wst, (step, sel.stats(), wst)


# ---- 8. the CLI and the Python driver on the influenza fixtures ---------------------------------------------------------------
NAMES = [l.strip() for l in (GOLDEN / "influenza_filelist.txt").read_text().splitlines() if l.strip()]


def all_pairs_file(tmp_path):
    f = tmp_path / "all45.txt"
    lines = []
    for a in range(len(NAMES)):
        for b in range(a + 1, len(NAMES)):
            x, y = (NAMES[a], NAMES[b]) if (a + b) % 3 else (NAMES[b], NAMES[a])     # mixed orientation
            lines.append(f"{x} {y} 0.0\n")
    assert len(lines) == 45
    f.write_text("".join(lines))
    return f


def cli(*args):
    return subprocess.run([str(BIN / "selection"), "-l", "influenza_filelist.txt", *[str(a) for a in args]], cwd=GOLDEN, capture_output=True, text=True)


@pytest.mark.parametrize("crit,a", [("smh_a", 512), ("hll_a", 256), ("hll_an", 256), ("none", None)])
def test_cli_all_pairs_as_a_list_reproduces_the_fixtures(tmp_path, crit, a):
    f = all_pairs_file(tmp_path)
    for h in ("0.01", "0.5", "0.9"):
        for flag, flavour in (("1", "fma"), ("0", "nofma")):
            name = f"influenza_{crit}_a{a}_h{h}.{flavour}.txt" if a else f"influenza_none_h{h}.{flavour}.txt"
            want = (EXP / name).read_text()
            out = cli("-p", f, "-h", h, "-c", crit, "-F", flag, *(("-a", a) if a else ()))
            assert out.returncode == 0, out.stderr
            assert out.stdout == want, (crit, h, flavour)
            if crit == "smh_a":
                for algo in ("stream", "sig"):
                    alt = cli("-p", f, "-h", h, "-c", crit, "-F", flag, "-a", a, "-A", algo)
                    if algo == "sig" and alt.returncode != 0:
                        assert "ALGO_SIG needs" in alt.stderr
                        continue
                    assert alt.returncode == 0 and alt.stdout == want, (algo, alt.stderr)
            if flavour == "fma":
                import os
                cwd = os.getcwd()
                os.chdir(GOLDEN)
                try:
                    got = pkg.select_pairs_from_filelist("influenza_filelist.txt", str(f), float(h), a or 0, criterion=crit)
                finally:
                    os.chdir(cwd)
                assert got == want
    if crit == "none":                                                        # -n: no CB bound
        out, ref_out = cli("-p", f, "-h", "0.5", "-c", "none", "-n"), cli("-h", "0.5", "-c", "none", "-n")
        assert out.returncode == 0 and ref_out.returncode == 0 and out.stdout == ref_out.stdout != ""


def test_cli_one_runs_output_is_the_next_runs_pair_file(tmp_path):
    pair_file = EXP / "influenza_none_h0.5.fma.txt"
    listed = {tuple(l.split()[:2]) for l in pair_file.read_text().splitlines()}
    assert len(listed) == 7
    full = (EXP / "influenza_smh_a_a512_h0.01.fma.txt").read_text().splitlines(keepends=True)
    assert len(full) == 27
    want = [l for l in full if tuple(l.split()[:2]) in listed or tuple(l.split()[:2][::-1]) in listed]
    assert len(want) == 7
    out = cli("-p", pair_file, "-c", "smh_a", "-a", 512, "-h", "0.01")
    assert out.returncode == 0, out.stderr
    assert out.stdout == "".join(want)
    # -o then -r round-trips
    res = tmp_path / "res.selr"
    out = cli("-p", pair_file, "-c", "smh_a", "-a", 512, "-h", "0.01", "-o", res)
    assert out.returncode == 0 and out.stdout == "", out.stderr
    back = subprocess.run([str(BIN / "selection"), "-r", str(res)], capture_output=True, text=True)
    assert back.returncode == 0 and back.stdout == "".join(want)
    # a pair file the list does not know, and an empty one
    bad = tmp_path / "bad.txt"
    bad.write_text(f"{NAMES[0]} {NAMES[1]} 1\n{NAMES[0]} nobody 1\n")
    out = cli("-p", bad, "-a", 512, "-h", "0.01")
    assert out.returncode == 5 and ":2:" in out.stderr and "unknown name nobody" in out.stderr
    empty = tmp_path / "empty.txt"
    empty.write_text("")
    out = cli("-p", empty, "-a", 512, "-h", "0.01")
    assert out.returncode == 0 and out.stdout == ""


@pytest.mark.parametrize("extra", [("-q", "influenza_filelist.txt"), ("-K", "3"), ("-q", "influenza_filelist.txt", "-k", "3"), ("-k", "3"), ("-B", "4"), ("-g", "2")])
def test_cli_refused_combinations(tmp_path, extra):
    out = cli("-p", all_pairs_file(tmp_path), "-a", 512, "-h", "0.5", *extra)
    assert out.returncode == 2, (extra, out.stderr)
    assert "-p" in out.stderr and out.stdout == ""
