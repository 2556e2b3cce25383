"""launcher_model.py on the host: on the canonical triangle (ascending cards, i < k, row-major) the model IS the oracle's all-pairs pass,
for both launchers; and its answers on the entries no other launcher test lists -- reversed, repeated, x == y, an empty sketch on
either side, cards that are not ascending -- are the ones include/selection_hip.h section 1 states.  test_launchers_lists_gpu.py holds
the launchers to this model."""
import numpy as np
import pytest

import launcher_model as LM
import precision_model as pm
import sig_model as S
from conftest import ROOT


def bits(j):
    return int(np.float32(j).view(np.int32))


@pytest.mark.parametrize("use_cb", [False, True], ids=["smh", "CBsmh"])
@pytest.mark.parametrize("p", [10, 13])
def test_model_is_the_oracle_on_the_canonical_triangle(oracle, p, use_cb):
    hll, aux, cards, _ = pm.pass_set(p)
    ii, kk = np.triu_indices(pm.N, 1)
    L = np.stack([ii, kk], axis=1).astype(np.int32)
    eq, J = LM.per_entry(oracle, hll, aux, cards, L, *pm.RB, p=p)
    for tau in (pm.TAU, 0.8):
        want, st = oracle.select(hll, aux, cards, tau, *pm.RB, use_cb=use_cb, p=p)
        got = LM.expected(oracle, cards, L, tau, use_cb, eq, J)
        assert 0 < len(want) < st["survivors"]
        exp = LM.sort_records(np.array([(int(w["i"]), int(w["k"]), bits(w["jacc"])) for w in want], dtype=np.int32))
        assert np.array_equal(got, exp)
        assert int(LM.live(oracle, cards, L, tau, use_cb).sum()) == st["evaluated"]
        assert int((LM.live(oracle, cards, L, tau, use_cb) & eq).sum()) == st["survivors"]
    if use_cb:
        assert not LM.live(oracle, cards, L, pm.TAU, True).all()              # the CB bound cuts entries of this set


def test_awkward_entries(oracle):
    p = 10
    hll, aux, cards, empty, twin = LM.awkward_set(oracle, p)
    n = len(cards)
    e = S.trunc_cards(cards)
    L = LM.awkward_list(n, empty)
    assert len(L) == n * n + 1500
    eq, J = LM.per_entry(oracle, hll, aux, cards, L, *pm.RB, p=p)
    x, y = L[:, 0], L[:, 1]
    rec = {(tau, cb): LM.expected(oracle, cards, L, tau, cb, eq, J) for tau in (0.5, -1.0) for cb in (False, True)}
    live = {(tau, cb): LM.live(oracle, cards, L, tau, cb) for tau in (0.5, -1.0) for cb in (False, True)}

    def listed(r, a, b):
        return int(((r[:, 0] == a) & (r[:, 1] == b)).sum())

    def times(a, b):
        return int(((x == a) & (y == b)).sum())

    # x == y: live like any entry, every band equal, J = (2 e - t) / t with t the estimate of the row itself; once per occurrence
    g = int(np.argmax(cards))
    assert times(g, g) >= 1
    j_self = oracle.jaccard(hll[g], hll[g], cards[g], cards[g], p)
    t = oracle.union_size(hll[g], hll[g], p)
    assert j_self == (float(e[g]) + float(e[g]) - t) / t and j_self > 0.99
    for key in rec:
        own = rec[key][(rec[key][:, 0] == g) & (rec[key][:, 1] == g)]
        assert len(own) == times(g, g) and set(own[:, 2].tolist()) == {bits(j_self)}, key
    # the empty sketch as y: skipped by every launcher at every tau; {empty, empty} too
    for key in rec:
        assert not live[key][y == empty].any() and not (rec[key][:, 1] == empty).any(), key
    # the empty sketch as x: live without CB, and under CB exactly when tau <= 0 (0 / e_y = 0)
    as_x = (x == empty) & (y != empty)
    assert live[(0.5, False)][as_x].all() and live[(-1.0, False)][as_x].all() and live[(-1.0, True)][as_x].all()
    assert not live[(0.5, True)][as_x].any()
    # ... and with an equal band (its row is twin's) it has a record wherever J = (0 + e_y - t) / t >= tau: at tau = -1, not at 0.5
    j_et = oracle.jaccard(hll[empty], hll[twin], cards[empty], cards[twin], p)
    assert -1.0 < j_et <= 0.0
    for cb in (False, True):
        assert listed(rec[(-1.0, cb)], empty, twin) == times(empty, twin) >= 1
        assert listed(rec[(0.5, cb)], empty, twin) == 0
        assert listed(rec[(-1.0, cb)], twin, empty) == 0
    # a reversed entry under CB: the ratio is x over y as listed, so {larger, smaller} is never cut and {smaller, larger} may be
    small, large = int(np.argmin(np.where(e == 0, e.max(), e))), g
    assert float(e[small]) / float(e[large]) < 0.5
    assert not live[(0.5, True)][(x == small) & (y == large)].any() and live[(0.5, True)][(x == large) & (y == small)].all()
    assert live[(0.5, False)][(x == small) & (y == large)].all()
    # both orientations of a selected pair are two records with the same J, each as listed; a repeated entry repeats its record
    r05 = rec[(0.5, False)]
    fwd = r05[r05[:, 0] < r05[:, 1]]
    a, b, jb = (int(v) for v in fwd[0])
    assert listed(r05, a, b) == times(a, b) >= 1 and listed(r05, b, a) == times(b, a) >= 1
    assert set(r05[(r05[:, 0] == b) & (r05[:, 1] == a)][:, 2].tolist()) == {jb}
    pairs_twice = [(int(a), int(b)) for a, b in zip(r05[:, 0], r05[:, 1]) if times(int(a), int(b)) > 1]
    assert pairs_twice and all(listed(r05, a, b) == times(a, b) for a, b in pairs_twice[:20])
    # cards are not ascending and the model never sorted anything
    assert np.any(np.diff(cards) < 0)
    assert len(rec[(0.5, True)]) <= len(rec[(0.5, False)]) < len(rec[(-1.0, False)]) == int((live[(-1.0, False)] & eq).sum())


def test_header_states_the_rules():
    import re
    text = " ".join(re.sub(r"\n\s*\*", " ", (ROOT / "include" / "selection_hip.h").read_text()).split())
    for phrase in ("in the orientation listed", "x == y is no special case", "cards need not be ascending", "once per occurrence",
                   '"pairs_gpw" and "pairs_grid"'):
        assert phrase in text, phrase
