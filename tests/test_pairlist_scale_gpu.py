"""Pair-list passes at the lengths that change their launch shape (selhip_ctx_run_pairs; csrc/kernel_pairs.cuh, csrc/host_pairs.hpp).

pairs_direct_kernel and the four pairs_count_kernel instantiations take gpw = clamp(P / 32 768, 1, 16) groups of four entries per wave
and batch and index by it (src = 4 t + quarter, pairs_quarter_bits(.., 4 t), the EMIT form's `(lane >> 2) == t`); every list kernel runs
a second trip of its grid-stride loop beyond one grid of 1 024 blocks, carrying its LDS append state and its per-wave tallies over.  The
other list tests stop at 44 850 entries: gpw = 1, one trip.  Here the lists are prefixes of ONE list of 1 124 250 distinct entries
(pairlist_scale_model.py), cut on the edges of the rule, and every case asserts the shape that ran -- get_param "pairs_gpw" and
"pairs_grid" -- before it compares records and statistics, bit for bit, with the oracle and the host models.  No tolerance anywhere."""
import numpy as np
import pytest

import cuda_selection_criteria_amd as pkg
import pairlist_scale_model as PS
import smhv_model as V
from pairlist_scale_model import BEYOND_ONE_GRID, LENGTHS, N, P_HLL, RB, TAU_CB, TOTAL
from test_pairlist_gpu import CFG_AUX, Ref

from cuda_selection_criteria_amd import (ALGO_AUTO, ALGO_SIG, ALGO_STREAM, CRIT_HLL_A, CRIT_NONE, CRIT_SMH_C, FP_FMA, MODE_CB_SMH,
                                         MODE_SMH, SelhipError, Selector)

pytestmark = pytest.mark.gpu

E_BADARG = -1
MODES = {"smh": (MODE_SMH, -1.0, False), "cb": (MODE_CB_SMH, TAU_CB, True)}      # tau = -1: every survivor is a record
_DEV = {}


def device_list(Sc, key="L", L=None):
    """the list on the device, copied once; a prefix is a view of it"""
    import torch
    if key not in _DEV:
        _DEV[key] = torch.from_numpy(Sc.L if L is None else L).to("cuda")
    return _DEV[key]


def loaded(Sc, aux=None, **params):
    sel = Selector(0, FP_FMA)
    for name, value in params.items():
        sel.set_param(name, value)
    sel.upload(Sc.hll, Sc.aux if aux is None else aux, Sc.cards, p_hll=P_HLL)
    return sel


def tuples(rec):
    return rec["i"].tolist(), rec["k"].tolist(), rec["jaccard"].view(np.uint64).tolist()


def assert_same(got, want):
    assert len(got) == len(want), (len(got), len(want))
    assert np.array_equal(got["i"], want["i"]) and np.array_equal(got["k"], want["k"])
    assert np.array_equal(got["jaccard"].view(np.uint64), want["jaccard"].view(np.uint64))


def assert_shape(sel, P, route, what):
    """the launch shape that ran, against the rule restated in pairlist_scale_model.py; printed, so that the test output shows it"""
    gpw, grid = sel.get_param("pairs_gpw"), sel.get_param("pairs_grid")
    want = PS.direct_shape(P) if route == 0 else (0, PS.flat_grid(P))
    n_trips = PS.trips(P, gpw)
    print(f"{what}: P={P} route={sel.get_param('pairs_route_used')} pairs_gpw={gpw} pairs_grid={grid} trips={n_trips}")
    assert sel.get_param("pairs_route_used") == route
    assert (gpw, grid) == want, (gpw, grid, want)
    return gpw, n_trips


def test_lengths_sit_on_the_edges():
    """(host arithmetic: the table of the lengths against the rule, so that a change of the rule shows here and not as a silent loss)"""
    shape = {P: PS.direct_shape(P) for P in LENGTHS}
    assert [shape[P][0] for P in LENGTHS] == [1, 2, 2, 3, 15, 16, 16, 16, 16]
    assert PS.trips(524288, 16) == 1 and PS.trips(524289, 16) == 2 and PS.trips(524288) == 1 and PS.trips(524289) == 2
    assert shape[65535] == (1, 1024) and shape[524288] == (16, 1024) and shape[65536] == (2, 1024) and shape[98305] == (3, 1024)
    assert PS.trips(65535, 1) == 2 and PS.trips(491537, 15) == 2                # (1 024 blocks of 32 gpw entries: short lists trip too)


# ---- 1. the direct route --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", list(LENGTHS), ids=[str(P) for P in LENGTHS])
@pytest.mark.parametrize("mode_name", list(MODES))
def test_direct_route(oracle, mode_name, P):
    Sc = PS.scale(oracle)
    mode, tau, use_cb = MODES[mode_name]
    want, wst = Sc.smh_a(P, tau, use_cb)
    assert 0 < wst["selected"] <= wst["survivors"] < wst["evaluated"] <= P
    if use_cb:
        assert wst["evaluated"] < P and wst["selected"] < wst["survivors"]
    d_L = device_list(Sc)
    with loaded(Sc) as sel:
        assert sel.get_param("pairs_gpw") == -1 and sel.get_param("pairs_grid") == -1          # no list pass yet
        got = sel.run_pairs(d_L[:P], tau, mode, *RB, algo=ALGO_STREAM)
        st = sel.stats()
        assert_shape(sel, P, 0, f"direct {mode_name}")
        assert st == wst, (st, wst)
        assert_same(got, want)
        assert sel.last_attempts() == 1 and sel.get_param("chunks") == 1      # default capacities: one attempt


def test_direct_route_clipped_stores(oracle):
    """a survivor list far too small: the counts stay exact when the stores are clipped, over both trips, and the repeat is right"""
    Sc = PS.scale(oracle)
    P = 1048613
    want, wst = Sc.smh_a(P, -1.0, False)
    d_L = device_list(Sc)
    with loaded(Sc, init_cap=1000) as sel:
        got = sel.run_pairs(d_L[:P], -1.0, MODE_SMH, *RB, algo=ALGO_STREAM)
        assert sel.last_attempts() > 1
        assert_shape(sel, P, 0, "direct, init_cap = 1000")
        assert sel.stats() == wst
        assert_same(got, want)
        got = sel.run_pairs(d_L[:P], -1.0, MODE_SMH, *RB, algo=ALGO_STREAM)   # the lists have grown
        assert sel.last_attempts() == 1 and sel.stats() == wst
        assert_same(got, want)


def test_direct_route_odd_band_shape_at_gpw_16(oracle):
    """17 x 4 on rows of 68 buckets: bands that straddle the 16-bucket steps, at 16 groups per wave and over two trips"""
    Sc = PS.scale(oracle)
    aux, planted, near, lit, J = Sc.odd
    r, nb = PS.ODD_RB
    sel_e = lit & ~np.isnan(J)
    assert bool((lit == sel_e).all()) and 0.01 < lit.mean() < 0.5
    want = PS.records(Sc.lo[sel_e], Sc.hi[sel_e], J[sel_e])
    d_L = device_list(Sc)
    with loaded(Sc, aux=aux) as sel:
        with pytest.raises(SelhipError, match="ALGO_SIG needs") as ei:
            sel.run_pairs(d_L, -1.0, MODE_SMH, r, nb, algo=ALGO_SIG)
        assert ei.value.code == E_BADARG
        for algo in (ALGO_STREAM, ALGO_AUTO):
            got = sel.run_pairs(d_L, -1.0, MODE_SMH, r, nb, algo=algo)
            gpw, n_trips = assert_shape(sel, TOTAL, 0, "direct 17x4")
            assert gpw == 16 and n_trips > 1
            n_lit = int(lit.sum())
            assert sel.stats() == {"evaluated": TOTAL, "survivors": n_lit, "selected": n_lit, "candidates": n_lit}
            assert_same(got, want)
            listed = set(zip(got["i"].tolist(), got["k"].tolist()))
            assert set(planted) <= listed and not set(near) & listed


# ---- 2. the signature route -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", BEYOND_ONE_GRID, ids=[str(P) for P in BEYOND_ONE_GRID])
@pytest.mark.parametrize("mode_name", list(MODES))
def test_signature_route(oracle, mode_name, P):
    Sc = PS.scale(oracle)
    mode, tau, use_cb = MODES[mode_name]
    want, wst = Sc.smh_a(P, tau, use_cb, route="sig")
    assert wst["candidates"] >= wst["survivors"] > 0
    d_L = device_list(Sc)
    with loaded(Sc) as sel:
        for algo in (ALGO_SIG, ALGO_AUTO):                                    # (P >= n / 2: the automatic choice is this route)
            got = sel.run_pairs(d_L[:P], tau, mode, *RB, algo=algo)
            _, n_trips = assert_shape(sel, P, 1, f"signature {mode_name}")
            assert n_trips >= 2
            assert sel.stats() == wst, (sel.stats(), wst)
            assert_same(got, want)
            assert sel.last_attempts() == 1


# ---- 3. the filter kernel: criteria without an smh_a stage -------------------------------------------------------------------------------
N_FILTER = 1100                               # 604 450 entries: a second trip of 80 162
TAU_FILTER = 0.9


class FilterSet(Ref):
    """test_pairlist_gpu.Ref on cfg2-spread scaled to N_FILTER genomes: p_hll = 14 (criterion none needs the bit planes) with
    auxiliary sketches; the CB bound at 0.9 keeps the pair space -- the oracle's work -- at a few percent of the list"""

    def __init__(self, oracle):
        CFG_AUX["cfg2-spread@scale"] = CFG_AUX["cfg2-spread"].scaled(N_FILTER)
        try:
            super().__init__(oracle, "cfg2-spread@scale", FP_FMA)
        finally:
            del CFG_AUX["cfg2-spread@scale"]
        self.rb = pkg.banding(self.m, TAU_FILTER)
        ii, kk = np.triu_indices(self.n, 1)
        rng = np.random.default_rng(N_FILTER)
        L = np.stack([ii, kk], axis=1).astype(np.int32)
        flip = rng.random(len(L)) < 0.5
        L[flip] = L[flip][:, ::-1]
        self.L = np.ascontiguousarray(L[rng.permutation(len(L))])
        self.lo, self.hi = self.L.min(axis=1).astype(np.int64), self.L.max(axis=1).astype(np.int64)
        e = PS.S.trunc_cards(self.cards)
        self.inE = (e[self.hi] != 0) & PS.cb_matrix(e, TAU_FILTER)[self.lo, self.hi]
        for j in range(0, len(self.L), 499):
            assert bool(self.inE[j]) == (e[self.hi[j]] != 0 and oracle.cb(TAU_FILTER, e[self.lo[j]], e[self.hi[j]])), j
        assert 1000 < int(self.inE.sum()) < len(self.L) // 4

    def expect(self, crit, P):
        """(records, statistics) of the first P entries"""
        S_dict, st_all = self.select(crit, TAU_FILTER, True, *self.rb)
        assert st_all["evaluated"] == int(self.inE.sum())
        J = np.full((self.n, self.n), np.nan)
        keys = np.array(sorted(S_dict), dtype=np.int64).reshape(-1, 2)
        J[keys[:, 0], keys[:, 1]] = [S_dict[tuple(k)] for k in keys.tolist()]
        Je = J[self.lo[:P], self.hi[:P]]
        sel = ~np.isnan(Je)
        inside = self.inE[:P]
        if crit == CRIT_NONE:
            passed = inside
        else:
            ok = np.zeros((self.n, self.n), dtype=bool)
            pk = np.array(sorted(self.passing(crit, TAU_FILTER, True, *self.rb)), dtype=np.int64).reshape(-1, 2)
            ok[pk[:, 0], pk[:, 1]] = True
            passed = inside & ok[self.lo[:P], self.hi[:P]]
        assert bool((sel <= passed).all())
        st = {"evaluated": int(inside.sum()), "survivors": int(passed.sum()), "selected": int(sel.sum())}
        return PS.records(self.lo[:P][sel], self.hi[:P][sel], Je[sel]), st


_FILTER = []


def filter_set(oracle):
    if not _FILTER:
        _FILTER.append(FilterSet(oracle))
    return _FILTER[0]


@pytest.mark.parametrize("crit_name,enum_pairs", [("none", None), ("hll_a", None), ("hll_a", 150001)])
def test_filter_kernel(oracle, crit_name, enum_pairs):
    R = filter_set(oracle)
    crit = {"none": CRIT_NONE, "hll_a": CRIT_HLL_A}[crit_name]
    total = len(R.L)
    assert total == N_FILTER * (N_FILTER - 1) // 2 > PS.ONE_GRID
    d_L = device_list(R, key="filter", L=R.L)
    sel = Selector(0, FP_FMA)
    with sel:
        if enum_pairs:
            sel.set_param("enum_pairs", enum_pairs)
        sel.upload(R.hll, R.aux, R.cards)
        sel.upload_aux_hll(R.aux_hll, 8)
        sel.set_criterion(crit)
        for P in (PS.ONE_GRID + 1, total):
            want, wst = R.expect(crit, P)
            assert 0 < wst["selected"] < wst["survivors"] <= wst["evaluated"] < P
            got = sel.run_pairs(d_L[:P], TAU_FILTER, MODE_CB_SMH, *R.rb)
            st = sel.stats()
            window = min(P, enum_pairs or P)
            gpw, grid = sel.get_param("pairs_gpw"), sel.get_param("pairs_grid")
            print(f"filter {crit_name} enum_pairs={enum_pairs}: P={P} windows={-(-P // window)} pairs_gpw={gpw} pairs_grid={grid} "
                  f"trips per window={PS.trips(window)} stats {st}")
            assert sel.get_param("pairs_route_used") == 2 and gpw == 0 and grid == PS.flat_grid(window)
            assert (PS.trips(window) > 1) == (enum_pairs is None)
            assert {k: st[k] for k in wst} == wst, (st, wst)
            if crit == CRIT_NONE:
                assert st["candidates"] == st["evaluated"]
            assert_same(got, want)
            assert sel.last_attempts() == 1


# ---- 4. the count kernel, all four instantiations -----------------------------------------------------------------------------------------
COUNT_LENGTHS = (65536, 524289, TOTAL)
C_MIN, GAMMA = 4, 0.1
# name: (estimator, c_min, gamma, measure, mode, tau, CB)
COUNT_CASES = {"fixed": ("hll", C_MIN, None, "jaccard", MODE_CB_SMH, TAU_CB, True),
               "containment": ("hll", None, GAMMA, "jaccard", MODE_SMH, -1.0, False),
               "fixed-emit": ("smh", C_MIN, None, "jaccard", MODE_CB_SMH, 0.07, True),
               "containment-emit": ("smh", None, GAMMA, "max_containment", MODE_SMH, 0.15, False)}


def count_expect(Sc, name, P):
    estimator, c_min, gamma, measure, _, tau, use_cb = COUNT_CASES[name]
    if estimator == "hll":
        return Sc.smh_c(P, tau, use_cb, Sc.need(c_min, gamma))
    return Sc.smh_v(P, tau, use_cb, measure, c_min, gamma)


def test_count_model_restatement(oracle):
    """Scale.smh_v IS smhv_model.expected_list, on the shortest of the lengths (the model gathers both rows of every entry)"""
    Sc = PS.scale(oracle)
    P = COUNT_LENGTHS[0]
    for name in ("fixed-emit", "containment-emit"):
        _, c_min, gamma, measure, _, tau, use_cb = COUNT_CASES[name]
        want, wst = V.expected_list(Sc.aux, Sc.cards, Sc.L[:P], tau, use_cb, measure, c_min=c_min, gamma=gamma)
        got, st = count_expect(Sc, name, P)
        assert st == wst and tuples(got) == tuples(want) and len(want) > 0
    need = Sc.need(None, GAMMA)
    assert {2, 3, 4} <= set(np.unique(need).tolist()) and int(need.min()) >= 1     # the per-entry thresholds differ


@pytest.mark.parametrize("P", COUNT_LENGTHS, ids=[str(P) for P in COUNT_LENGTHS])
@pytest.mark.parametrize("name", list(COUNT_CASES))
def test_count_kernel(oracle, name, P):
    Sc = PS.scale(oracle)
    estimator, c_min, gamma, measure, mode, tau, use_cb = COUNT_CASES[name]
    want, wst = count_expect(Sc, name, P)
    share = wst["survivors"] / P
    print(f"count {name}: P={P} share of entries that pass the count {share:.3f} expected {wst}")
    assert 0.05 <= share <= 0.5 and 0 < wst["selected"]
    if name != "containment":
        assert wst["selected"] < wst["survivors"]                             # tau cuts records too
    if use_cb:
        assert wst["evaluated"] < P
    d_L = device_list(Sc)
    with loaded(Sc) as sel:
        sel.set_criterion(CRIT_SMH_C)
        if c_min is not None:
            sel.set_min_matches(c_min)
        elif estimator == "smh":
            sel.set_min_matches(1)                                            # (the floor under the estimator; never set under "hll")
        sel.set_min_containment(gamma)
        sel.set_measure(measure)
        sel.set_estimator(estimator)
        got = sel.run_pairs(d_L[:P], tau, mode, 7, 3)                         # (n_rows, n_bands are ignored)
        st = sel.stats()
        gpw, n_trips = assert_shape(sel, P, 0, f"count {name}")
        assert gpw == PS.direct_shape(P)[0] and (n_trips > 1) == (P > PS.ONE_GRID)
        assert sel.get_param("smhc_rule_used") == (1 if gamma is not None else 0)
        assert st == wst, (st, wst)
        assert_same(got, want)
        assert sel.last_attempts() == 1


# ---- 5. invalid entries far into the list ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,route", [(ALGO_STREAM, 0), (ALGO_SIG, 1)], ids=["direct", "signature"])
def test_invalid_entries_in_the_second_trip(oracle, algo, route):
    import torch
    Sc = PS.scale(oracle)
    P = 1048613
    at_rank, at_equal = 600000, 1000                                          # an out-of-range rank in the second trip, x == y before it
    assert at_rank > PS.ONE_GRID > at_equal
    L = Sc.L[:P].copy()
    L[at_rank] = (N, 3)
    L[at_equal] = (17, 17)
    d_bad = torch.from_numpy(L).to("cuda")
    d_L = device_list(Sc)
    want, wst = Sc.smh_a(P, TAU_CB, True, route="sig" if route == 1 else "direct")
    with loaded(Sc) as sel:
        with pytest.raises(SelhipError, match="2 invalid entries") as ei:
            sel.run_pairs(d_bad, TAU_CB, MODE_CB_SMH, *RB, algo=algo)
        assert ei.value.code == E_BADARG and f"entry {at_rank} is one" in str(ei.value), str(ei.value)
        assert_shape(sel, P, route, "invalid entries")
        with pytest.raises(SelhipError):
            sel.stats()
        got = sel.run_pairs(d_L[:P], TAU_CB, MODE_CB_SMH, *RB, algo=algo)     # a valid pass on the same context
        assert sel.stats() == wst
        assert_same(got, want)
