"""The model of the threshold decisions (tests/decision_model.py) and its forged cases, without a GPU: the exact reference against
orc_cb, the coverage the generators reach (asserted, not assumed), the wrong variants the cases must tell from the reference, and the
shape of every set the device tests upload (test_decision_boundaries_gpu.py)."""
import math
import random
from fractions import Fraction

import numpy as np
import pytest

import decision_model as M

J_TAUS = (0.5, 0.8, 0.9, 0.95)      # tau = 0.01: ulp(tau) = 2^-59 and the step of J at t >= 2^52 is 2^-54 or more: J == tau is not asserted there
AUX = [(crit, tau, p_aux) for crit in ("hll_a", "hll_an") for tau in (0.9, 0.5) for p_aux in (8, 4, 12)]


# ---- the exact reference itself --------------------------------------------------------------------------------------------------
def test_round_to_double_is_ieee():
    """round_to_double against the host's own correctly rounded operations: int -> float, float / float"""
    rnd = random.Random(5)
    for _ in range(3000):
        a = rnd.getrandbits(rnd.randint(1, 63)) | 1
        b = rnd.getrandbits(rnd.randint(1, 63)) | 1
        assert M.u64_to_f64(a) == float(a)
        assert M.round_to_double(Fraction(float(a)) / Fraction(float(b))) == float(a) / float(b)
        assert M.u64_to_f64(a, toward_zero=True) <= float(a)
    # ties go to even, toward_zero drops
    assert M.u64_to_f64((1 << 53) + 1) == float(1 << 53) and M.u64_to_f64((1 << 53) + 3) == float((1 << 53) + 4)
    assert M.u64_to_f64((1 << 53) + 3, toward_zero=True) == float((1 << 53) + 2)
    assert M.u64_to_f64((1 << 63) - 1) == 2.0 ** 63


def test_trunc_card():
    assert M.trunc_card(0.25) == 0 and M.trunc_card(M.just_below_next(0)) == 0 and M.trunc_card(5e-324) == 0
    for e in (1, 7549747, (1 << 40) + 3, (1 << 52) - 1):
        assert M.trunc_card(float(e)) == M.trunc_card(e + 0.5) == M.trunc_card(M.just_below_next(e)) == e
        assert round(M.just_below_next(e)) == e + 1                          # rounding would move it
    assert M.trunc_card(float((1 << 62) + (1 << 10))) == (1 << 62) + (1 << 10)
    # the model of sig_model.py (numpy) truncates the same way
    cards = np.array([0.25, 1.5, M.just_below_next(12345), float(1 << 60)])
    assert M.S.trunc_cards(cards).tolist() == [M.trunc_card(c) for c in cards]


def test_tau_forms():
    assert M.tau_parts(0.9) == (7549747, 23) and M.tau_parts(0.5) == (1, 1)
    for tau in M.TAUS:
        num, k = M.tau_parts(tau)
        assert Fraction(num, 1 << k) == Fraction(M.tau_double(tau)) and (num & 1)


# ---- CB --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", M.TAUS)
def test_orc_cb_agrees_with_the_exact_reference(oracle, tau):
    cases = M.cb_cases(tau)
    assert len(cases) > 500
    for c in cases:
        assert oracle.cb(tau, c.e_lo, c.e_hi) == c.accept, c
        assert c.accept == M.cb_ref(tau, c.e_lo, c.e_hi) and c.dist == M.cb_distance(tau, c.e_lo, c.e_hi)
        assert 0 < c.e_lo <= c.e_hi < M.TWO63


@pytest.mark.parametrize("tau", M.TAUS)
def test_cb_coverage(tau):
    reach, model = M.cb_counts(tau, True), M.cb_counts(tau, False)
    print(tau, "reachable", sorted(reach.items()), "model only", sorted(model.items()))
    for big in (False, True):
        assert reach.get(("on", big), 0) >= 1                                # exactly on the threshold, below and beyond 2^53
        assert reach.get(("above", big), 0) >= 1                             # the first integer pair above
    assert reach.get(("below-rejected", True), 0) >= 1                       # rejected within one ulp
    if tau != 0.5:
        # tau = 0.5: 1/2 + d / (2 e_hi) is an ulp or more from 1/2 for every d != 0 and e_hi < 2^53 (decision_model.cb_cases)
        for big in (False, True):
            assert reach.get(("below-accepted", big), 0) >= 1                # accepted although the exact value is below tau
        assert reach.get(("below-rejected", False), 0) >= 1
    # beyond 2^53 with integers that are no doubles (model only: no card carries them): every kind, and the conversions decide
    for kind in ("above", "below-accepted", "below-rejected"):
        assert model.get((kind, True), 0) >= 1, kind
    assert sum(c.convert_decides for c in M.cb_cases(tau) if not c.reachable) >= 1
    assert not any(c.convert_decides for c in M.cb_cases(tau) if c.reachable)      # a double converts exactly
    # the labels mean what they say
    for c in M.cb_cases(tau):
        if c.kind == "below-accepted":
            assert c.accept and Fraction(-1, 2) <= c.dist < 0 or not c.reachable
        if c.reachable and c.kind == "below-rejected":
            assert not c.accept and -1 < c.dist <= Fraction(-1, 2)


CB_MUTANTS = {
    "mul-compare": M.cb_mul_compare,              # e_lo >= tau * e_hi
    "trunc-divide": M.cb_trunc_divide,            # a division that is not correctly rounded
    "float-gamma": M.cb_float_gamma,              # gamma held in a float
    "strict-greater": M.cb_strict_greater,        # > for >=
}


# tau = 1/2 is left out for two: tau * e_hi is exact, and no quotient of two doubles lies within half an ulp below 1/2
CB_MUTANT_CASES = [(tau, name) for tau in M.TAUS for name in CB_MUTANTS if not (tau == 0.5 and name in ("mul-compare", "trunc-divide"))]


@pytest.mark.parametrize("tau,name", CB_MUTANT_CASES)
def test_cb_cases_tell_the_wrong_variants(tau, name):
    """each wrong variant decides at least one REACHABLE case differently from the reference -- and one that the sets carry"""
    f = CB_MUTANTS[name]
    killed = [c for c in M.cb_cases(tau) if c.reachable and f(tau, c.e_lo, c.e_hi) != c.accept]
    in_sets = [c for accept in (True, False) for cs in M.cb_sets(tau, accept) for _, _, c in cs.forged if f(tau, c.e_lo, c.e_hi) != c.accept]
    print(tau, name, len(killed), "cases,", len(in_sets), "in the sets")
    assert killed and in_sets


@pytest.mark.parametrize("tau", M.TAUS)
def test_wrong_conversion_shows_on_integers_that_are_no_doubles(tau):
    """a truncating u64 -> f64: no reachable case can show it in CB (a double converts exactly); the model's integers do"""
    cases = M.cb_cases(tau)
    assert any(M.cb_trunc_convert(tau, c.e_lo, c.e_hi) != c.accept for c in cases if not c.reachable)
    assert all(M.cb_trunc_convert(tau, c.e_lo, c.e_hi) == c.accept for c in cases if c.reachable)


@pytest.mark.parametrize("accept", [True, False], ids=["inside", "outside"])
@pytest.mark.parametrize("tau", M.TAUS)
def test_cb_sets(oracle, tau, accept):
    sets = M.cb_sets(tau, accept)
    shown = set()
    seen = dict.fromkeys(("next rank", "ranks away", "run of e_hi", "run of e_lo", "fraction", "partner above P", "partner below P",
                          "query equal to a database genome"), False)
    for cs in sets:
        e = [M.trunc_card(c) for c in cs.cards]
        assert len(cs.cards) <= 256 and np.all(np.isfinite(cs.cards)) and np.all(np.diff(cs.cards) >= 0) and cs.cards[-1] < 2.0 ** 63
        assert e[:3] == [0, 0, 0] and e[3] != 0                              # cards in (0, 1): no candidates
        lo, hi = M.S.allpairs_windows(cs.cards, tau, True)
        for lo_rank, hi_rank, c in cs.forged:
            assert (e[lo_rank], e[hi_rank]) == (c.e_lo, c.e_hi) and c.accept == accept
            assert oracle.cb(tau, e[lo_rank], e[hi_rank]) == accept
            shown.add((c.kind, c.big))
            # the forged partner is the boundary of its row: the last k inside (its run included), or the first k outside
            run_end = max(g for g in range(len(e)) if e[g] == c.e_hi)
            assert hi[lo_rank] == (run_end if accept else hi_rank - 1)
        assert cs.forged[0][:2] == (63, 64)                                  # across two waves
        assert max(g for g in range(len(e)) if e[g] == cs.forged[-1][2].e_hi) == len(e) - 1      # the partner is the last rank
        seen["next rank"] |= any(h == l + 1 for l, h, _ in cs.forged)
        seen["ranks away"] |= not accept or any(h > l + 1 for l, h, _ in cs.forged)
        # runs of equal e on either side of a boundary, held equal by truncation alone
        seen["run of e_hi"] |= any(e.count(c.e_hi) > 1 for _, _, c in cs.forged)
        seen["run of e_lo"] |= any(e.count(c.e_lo) > 1 for _, _, c in cs.forged)
        seen["fraction"] |= any(c != math.floor(c) and c > 1 << 31 for c in cs.cards) or all(c.e_lo >= M.TWO52 for _, _, c in cs.forged)
        # the query split: the partner at the first and at the last database rank, above and below P, queries equal to database genomes
        q, d = M.split_for_queries(cs)
        assert sorted(q.tolist() + d.tolist()) == list(range(len(e))) and len(q) and len(d)
        assert e[d[0]] == cs.forged[0][2].e_lo and e[d[-1]] == cs.forged[-1][2].e_hi
        sides = {(lo_rank in set(d.tolist()), hi_rank in set(d.tolist())) for lo_rank, hi_rank, _ in cs.forged}
        seen["partner above P"] |= (False, True) in sides
        seen["partner below P"] |= (True, False) in sides
        seen["query equal to a database genome"] |= bool({e[g] for g in q} & {e[g] for g in d})
    assert shown == {(c.kind, c.big) for c in M.pick_cb_cases(tau, accept)}   # every reachable kind of this side is in some set
    assert all(seen.values()), seen                                           # (over the sets of this side: one of them may hold one cluster)


# ---- J ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def j_sets(oracle):
    return {tau: M.j_genome_sets(oracle, tau, seed=0x1A + int(tau * 100)) for tau in J_TAUS + (0.01,)}


@pytest.mark.parametrize("tau", J_TAUS + (0.01,))
def test_j_cases(oracle, j_sets, tau):
    inside, outside, cases = j_sets[tau]
    td = M.tau_double(tau)
    sides = [c.side for c in cases]
    print(tau, {s: sides.count(s) for s in (-1, 0, 1)}, [f"2^{math.log2(c.t):.1f}" for c in cases if c.side == 0])
    if tau in J_TAUS:
        assert sides.count(0) >= 1                                           # J == tau exactly
    assert sides.count(-1) >= 3 and sides.count(1) >= 3
    assert any(c.t < 2.0 ** 53 for c in cases) and any(c.t > 2.0 ** 61 for c in cases)
    assert any(c.e1 > M.TWO53 and c.side == 0 for c in cases) or tau not in J_TAUS
    for c in cases:
        assert M.is_double(c.e1) and M.is_double(c.e2) and 0 < c.e1 <= c.e2 < M.TWO63
        assert abs(c.j - td) <= 160 * math.ulp(td) and (c.side == 0) == (c.j == td) and (c.side < 0) == (c.j < td)
        assert oracle.cb(0.95, c.e1, c.e2)                                   # nearly equal: the pair clears CB at every tau
    for gs, accept in ((inside, True), (outside, False)):
        assert len(gs.cards) <= 256 and np.all(np.isfinite(gs.cards)) and np.all(np.diff(gs.cards) >= 0) and gs.cards[-1] < 2.0 ** 63
        for a, b, c in gs.forged:
            # the value reference: selection.cpp:286-287 as the oracle restates it, on the set's own rows
            j = oracle.jaccard(gs.hll[a], gs.hll[b], gs.cards[a], gs.cards[b])
            if math.isnan(c.j):
                assert j is None and not accept                              # t = +inf: NaN, rejected
            else:
                assert j == c.j and (j >= td) == accept
    assert math.isinf(inside.forged[-1][2].j) and inside.forged[-1][2].t == 0.0      # t = 0: J = +inf, accepted


@pytest.mark.parametrize("fma", [1, 0], ids=["fma", "strict"])
@pytest.mark.parametrize("tau", J_TAUS)
def test_j_cases_below_register_32(oracle, tau, fma):
    """the sets of the one-launch pass: J == tau on rows whose registers stay below 32, one step of 1 / t on either side"""
    oracle.set_fma(fma)
    try:
        inside, outside, cases = M.j_low_genome_sets(oracle, tau, seed=0x51 + int(tau * 100))
        td = M.tau_double(tau)
        assert len(cases) >= 3 and [c.side for c in cases[:3]] == [-1, 0, 1] and outside is not None
        assert inside.hll.max() < 32 and outside.hll.max() < 32
        for gs, accept in ((inside, True), (outside, False)):
            assert np.all(np.diff(gs.cards) >= 0) and gs.cards[-1] < 2.0 ** 53
            for a, b, c in gs.forged:
                j = oracle.jaccard(gs.hll[a], gs.hll[b], gs.cards[a], gs.cards[b])
                assert j == c.j and (j >= td) == accept == c.accept and (c.side == 0) == (j == td)
    finally:
        oracle.set_fma(1)


@pytest.mark.parametrize("tau", J_TAUS)
def test_j_wrong_variants(oracle, j_sets, tau):
    td = M.tau_double(tau)
    cases = j_sets[tau][2]
    assert any((c.j > td) != c.accept for c in cases)                        # > for >=
    # (double)(e1 + e2) for (double)e1 + (double)e2, and a truncating conversion: equal to the reference on every pair of doubles ...
    for c in cases:
        assert M.j_value_sum_first(c.e1, c.e2, c.t) == c.j == M.j_value_trunc_convert(c.e1, c.e2, c.t)
    # ... and on opposite sides of tau for integers beyond 2^53 that are no doubles (model only)
    found = [M.sum_order_case(tau, c.t) for c in cases if c.t > 2.0 ** 55]
    assert found and all(f is not None for f in found)
    for e1, e2, j_ref, j_mut in found:
        assert e1 > M.TWO53 and not (M.is_double(e1) and M.is_double(e2)) and (j_ref >= td) != (j_mut >= td)


# ---- hll_a, hll_an ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def aux_sets(oracle):
    return {key: M.aux_genome_sets(oracle, *key) for key in AUX}


@pytest.mark.parametrize("crit,tau,p_aux", AUX)
def test_aux_cases(oracle, aux_sets, crit, tau, p_aux):
    sets, cases = aux_sets[(crit, tau, p_aux)]
    td = M.tau_double(tau)
    on = [sum(c.value[f] == td for c in cases) for f in (0, 1)]
    flips = [c for c in cases if c.accept[0] != c.accept[1]]
    print(crit, tau, p_aux, len(cases), "cases, on tau", on, "flavours differ", len(flips), "of them on one union estimate",
          sum(c.union[0] == c.union[1] for c in flips), "sum rounds", sum(not M.is_double(c.e_lo + c.e_hi) for c in cases))
    assert len({c.pair for c in cases}) == 8
    assert on[0] + on[1] >= 1                                                # the criterion's value equals tau where the scan reaches it
    for f in (0, 1):
        assert any(c.value[f] < td for c in cases) and any(c.value[f] > td for c in cases)
        assert min(abs(c.value[f] - td) for c in cases if c.value[f] != td) <= 2 * math.ulp(td)
    assert flips or crit == "hll_an"                                        # (hll_an: the flavour enters through the union estimate alone)
    for c in cases:
        assert all(math.isfinite(u) and 0 < u < 2.0 ** 63 for u in c.union)   # beyond: undefined in the reference
        assert M.is_double(c.e_lo) and M.is_double(c.e_hi) and 0 < c.e_lo <= c.e_hi < M.TWO63
        for f in (0, 1):
            oracle.set_fma(f)
            assert M.aux_decide(oracle, crit, tau, c.e_lo, c.e_hi, c.union[f], p_aux) == c.accept[f] == (c.value[f] >= td)
        oracle.set_fma(1)
    for (f, accept), gs in sets.items():
        assert len(gs.cards) <= 256 and np.all(np.isfinite(gs.cards)) and np.all(np.diff(gs.cards) >= 0) and gs.cards[-1] < 2.0 ** 63
        assert all(c.accept[f] == accept for _, _, c in gs.forged)
        oracle.set_fma(f)
        for a, b, c in gs.forged:
            assert oracle.union_size(gs.aux_hll[a], gs.aux_hll[b], p_aux) == c.union[f]
            assert (M.trunc_card(gs.cards[a]), M.trunc_card(gs.cards[b])) == (c.e_lo, c.e_hi)
        oracle.set_fma(1)
    assert set(sets) == {(f, a) for f in (0, 1) for a in (False, True)}


def test_fused_product_decides(aux_sets):
    """hll_a: on ONE union estimate, (1 + gamma) * e_hi - t+ fused puts K+ on the other side of tau than the product rounded first"""
    hits = [c for (crit, _, _), (_, cases) in aux_sets.items() if crit == "hll_a" for c in cases
            if c.accept[0] != c.accept[1] and c.union[0] == c.union[1]]
    assert hits
    assert any(c.value[f] == M.tau_double(c.tau) for c in hits for f in (0, 1))      # on the boundary in one flavour, off it in the other


def test_sum_conversion_decides(oracle, aux_sets):
    """hll_an's (double)(e_lo + e_hi) is the one conversion of the device that rounds: cases where a truncating conversion of the sum
    decides differently are in the sets"""
    hits = 0
    for (crit, tau, p_aux), (_, cases) in aux_sets.items():
        if crit != "hll_an":
            continue
        for c in cases:
            s = c.e_lo + c.e_hi
            if M.is_double(s):
                continue
            for f in (0, 1):
                oracle.set_fma(f)
                U = c.union[f]
                wrong = (M.u64_to_f64(s, toward_zero=True) - U) / U + oracle.cota_n(c.e_lo, c.e_hi, U, p_aux)
                hits += (wrong >= M.tau_double(tau)) != c.accept[f]
    oracle.set_fma(1)
    assert hits >= 1
