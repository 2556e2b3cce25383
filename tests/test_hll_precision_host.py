"""What keeps test_hll_precision_gpu.py from passing vacuously, checked on the oracle alone (no GPU): at every precision the pass tests
use, the generated set of precision_model.py gives the join survivors, the J test both outcomes and the CB bound pairs to cut; the
numpy model of the union histogram agrees with the oracle's; and libselhost's estimator -- the code the device estimator is compiled
from (csrc/ertl_mle.hpp) -- gives the oracle's bits at every precision the ABI accepts, in both FP flavours."""
import inspect
import math

import numpy as np
import pytest

import cuda_selection_criteria_amd as pkg
import precision_model as pm
from precision_model import ALL_PS, M, N, PASS_PS, RB, TAU


@pytest.mark.parametrize("p", PASS_PS)
def test_pass_sets_are_not_vacuous(oracle, p):
    hll, aux, cards, _ = pm.pass_set(p)
    assert hll.shape == (N, 1 << p) and aux.shape == (N, M) and hll.dtype == np.uint8 and aux.dtype == np.uint64
    assert int(hll.max()) <= 64 - p + 1                                      # valid sketches only
    assert (np.diff(cards) >= 0).all() and cards[0] > 0 and np.isfinite(cards).all()
    assert np.array_equal(cards.view(np.uint64), oracle.cards(hll, p).view(np.uint64))
    total = N * (N - 1) // 2
    for use_cb in (True, False):
        want, st = oracle.select(hll, aux, cards, TAU, *RB, use_cb=use_cb, p=p)
        print(f"p={p} cb={use_cb}: evaluated {st['evaluated']} of {total}, survivors {st['survivors']}, selected {len(want)}")
        assert st["survivors"] >= 40
        assert len(want) >= 5
        assert st["survivors"] - len(want) >= 5                              # survivors that the J test rejects
        assert st["evaluated"] == int(pm.pair_space(cards, TAU, use_cb).sum())
        owned = np.bincount(want["i"], minlength=N) + np.bincount(want["k"], minlength=N)
        assert owned.max() > 3 and owned.min() == 0                          # a top-3 per genome cuts someone, someone owns nothing
        if use_cb:
            assert st["evaluated"] < total                                   # CB really prunes
        else:
            assert st["evaluated"] == total
    # the strict flavour's own ranking gives a set that passes the same conditions (the GPU tests run both)
    hll0, aux0, cards0, _ = pm.pass_set(p, fma=0)
    oracle.set_fma(0)
    try:
        want0, st0 = oracle.select(hll0, aux0, cards0, TAU, *RB, use_cb=True, p=p)
    finally:
        oracle.set_fma(1)
    assert st0["survivors"] >= 40 and len(want0) >= 5 and st0["survivors"] - len(want0) >= 5 and st0["evaluated"] < total


@pytest.mark.parametrize("p", PASS_PS)
def test_smhc_threshold_cuts_and_keeps(oracle, p):
    """the count threshold of the smh_c tests removes some of the selected pairs of the one-bucket-band pass and keeps some"""
    hll, aux, cards, _ = pm.pass_set(p)
    for use_cb in (True, False):
        c, want, kept = pm.smhc_threshold(oracle, hll, aux, cards, p, TAU, use_cb)
        assert 1 < c <= M and 0 < int(kept.sum()) < len(want), (p, c, len(want), int(kept.sum()))
    # bands of one bucket: a pair passes iff some bucket is equal -- the oracle's survivors are the numpy count's
    _, st = oracle.select(hll, aux, cards, TAU, 1, M, use_cb=False, p=p)
    assert st["survivors"] == int(np.triu(pm.match_counts(aux) >= 1, 1).sum())


@pytest.mark.parametrize("p", (10, 15))
def test_aux_criteria_sets_are_not_vacuous(oracle, p):
    hll, aux, cards, aux_hll = pm.pass_set(p, p_aux=8)
    assert aux_hll.shape == (N, 256) and int(aux_hll.max()) <= 57
    assert np.array_equal(hll, pm.pass_set(p)[0])                            # the same genomes in the same order
    for crit in (1, 2, 3):                                                   # hll_a, hll_an, hll_a + smh_a
        for use_cb in (True, False):
            want, st = oracle.select(hll, aux, cards, TAU, *RB, use_cb=use_cb, criterion=crit, aux_hll=aux_hll, p=p, p_aux=8)
            assert len(want) >= 5 and st["survivors"] - len(want) >= 5, (p, crit, use_cb, st, len(want))


@pytest.mark.parametrize("p", ALL_PS)
def test_union_model_and_host_estimator(oracle, host, p):
    """union_hist sums to 2^p; Oracle.estimate of it is Oracle.union_size; libselhost's estimator gives the oracle's bits on the edge
    rows and a few generated ones, both flavours (0 for the empty histogram, +inf for the saturated one)"""
    rng = np.random.default_rng([7, p])
    gen = pm.sketch_set(p, 6, 8, pm.SEED)[0]
    rows = np.concatenate([pm.edge_rows(p, rng), gen])
    assert int(rows.max()) <= 64 - p + 1
    bins = set()
    for i in range(len(rows)):
        for k in range(i, len(rows)):
            c = pm.union_hist(rows[i], rows[k])
            bins |= set(np.nonzero(c)[0].tolist())
            assert int(c.sum()) == 1 << p and c.shape == (64,)
            assert np.array_equal(c, oracle.union_hist(rows[i], rows[k]))
            for fp in (1, 0):
                oracle.set_fma(fp)
                try:
                    u = oracle.union_size(rows[i], rows[k], p)
                finally:
                    oracle.set_fma(1)
                want = oracle.estimate(c, p, fp)
                assert want == u or (math.isnan(want) and math.isnan(u)), (p, i, k, fp, want, u)
                got = host.selhost_ertl_estimate(c.ctypes.data, p, fp)
                assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (p, i, k, fp, got, want)
    assert oracle.estimate(pm.union_hist(rows[0], rows[0]), p) == 0.0
    assert math.isinf(oracle.estimate(pm.union_hist(rows[1], rows[2]), p))
    assert 0 in bins and 64 - p + 1 in bins and 64 - p in bins


def test_bit_length_is_exact():
    xs = np.array([0, 1, 2, 3, (1 << 53) - 1, 1 << 53, (1 << 60) - 1, 1 << 60, (1 << 64) - 1], dtype=np.uint64)
    assert pm.bit_length(xs).tolist() == [int(x).bit_length() for x in xs.tolist()]
    # a hash whose low q bits are zero has the largest value a register takes, q + 1; one with the top bit of them set has 1
    for p in (4, 14, 20):
        q = 64 - p
        row = pm.registers(np.array([0, (1 << 64) - 1, (3 << q) | 1], dtype=np.uint64), p)
        assert row[0] == q + 1 and row[(1 << p) - 1] == 1 and row[3] == q


def test_drivers_take_p_hll():
    """ooc_select and multi_select pass the main sketches' precision on (default 14) and check the shape of hll, as Selector.upload does"""
    for fn in (pkg.ooc_select, pkg.selection.multi_select):
        assert inspect.signature(fn).parameters["p_hll"].default == 14
    hll = np.zeros((4, 1 << 10), dtype=np.uint8)
    aux = np.zeros((4, 8), dtype=np.uint64)
    cards = np.arange(4, dtype=np.float64)
    with pytest.raises(AssertionError):
        pkg.ooc_select(hll, aux, cards, 0.5, 2, n_rows=1, n_bands=8)                     # rows of 2^10 registers given as p_hll = 14
    with pytest.raises(AssertionError):
        pkg.selection.multi_select([0], hll, aux, cards, 0.5, n_rows=1, n_bands=8, gather=0)


def test_documents_name_the_precision_tests():
    from conftest import ROOT
    for doc in ("include/selection_hip.h", "DESIGN.md"):
        text = (ROOT / doc).read_text()
        for word in ("p_hll != 14", "hll_union_hist_kernel", "test_hll_precision_gpu.py", "test_hll_precision_host.py"):
            assert word in text, (doc, word)
