"""The bit-sliced signature join ("join_form" = 2, sigl_join_kernel FORM 3): the same 16-bit matches as the packed-minimum form 0, so the
same candidates, survivors and pairs -- against the oracle and against form 0 on the same context, over every band count, both modes,
the launch shapes of the LDS-tile join, row ranges, interleaved parts, chunk lanes, the signature cache and the shapes that fall back."""
import sys

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

import cuda_selection_criteria_amd as pkg  # noqa: E402
from cuda_selection_criteria_amd import ALGO_SIG, MODE_CB_SMH, MODE_SMH, Selector  # noqa: E402

sys.path.insert(0, str(GOLDEN))
import make_golden  # noqa: E402

SLICED, PACKED = 3, 0                                   # kernel FORM reported by get_param("join_form_used")


def sorted_set(name, oracle):
    cfg = make_golden.GOLDEN_SYNTH[name]
    hll, aux, _ = pkg.synth_host(cfg)
    cards = oracle.cards(hll)
    perm = pkg.sort_by_card(cards)
    return cfg, hll[perm], aux[perm], cards[perm]


def same_pairs(got, want):
    return (got.shape[0] == want.shape[0] and np.array_equal(got["i"], want["i"]) and np.array_equal(got["k"], want["k"])
            and np.array_equal(got["jaccard"].view(np.uint64), want["jacc"].view(np.uint64)))


def run_form(sel, form, tau, mode, r, b, **kw):
    sel.set_param("join_form", form)
    got = sel.run(tau, mode, r, b, algo=ALGO_SIG, **kw)
    s = sel.stats()
    return got, (s["evaluated"], s["survivors"], s["candidates"]), sel.get_param("join_form_used")


# (set, tau, (rows per band, bands)): nb = 8, 16, 32, 64, 128, every one a shape of the tiled build
SHAPES = [("synth_spread_n600_m64", 0.5, (8, 8)), ("synth_spread_n600_m64", 0.5, (4, 16)), ("synth_flat_n200_m128", 0.5, (8, 16)),
          ("synth_spread_n600_m64", 0.5, (2, 32)), ("synth_flat_n1000_m256", 0.9, (8, 32)), ("synth_flat_n300_m512", 0.5, (8, 64)),
          ("synth_flat_n300_m512", 0.5, (4, 128)), ("synth_flat_n300_m512", 0.8, (16, 32))]
# (waves per block, tile height, candidate groups per wave, triangle grid)
LAUNCH = [(4, 0, 1, 0), (8, 16, 1, 1), (4, 32, 2, 0), (8, 64, 2, 1), (4, 128, 1, 1), (8, 256, 2, 0), (4, 48, 1, 0), (8, 0, 2, 1), (4, 0, 0, 0)]


@pytest.mark.parametrize("name,tau,shape", SHAPES)
def test_sliced_join_matches_oracle_and_packed(oracle, name, tau, shape):
    cfg, hll, aux, cards = sorted_set(name, oracle)
    r, b = shape
    want, st = oracle.select(hll, aux, cards, tau, r, b)
    want_all, st_all = oracle.select(hll, aux, cards, tau, r, b, use_cb=False)
    n = hll.shape[0]
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        ref = {}
        for mode, w, s in ((MODE_CB_SMH, want, st), (MODE_SMH, want_all, st_all)):
            got, stats, used = run_form(sel, 0, tau, mode, r, b)
            assert used == PACKED and same_pairs(got, w) and stats[:2] == (s["evaluated"], s["survivors"])
            ref[mode] = stats
        for wpb, qt, t, tri in LAUNCH:
            sel.set_param("join_wpb", wpb); sel.set_param("join_qt", qt); sel.set_param("join_t", t); sel.set_param("join_tri", tri)
            for mode, w in ((MODE_CB_SMH, want), (MODE_SMH, want_all)):
                got, stats, used = run_form(sel, 2, tau, mode, r, b)
                assert used == SLICED, (wpb, qt, t, tri)
                assert same_pairs(got, w), (mode, wpb, qt, t, tri, len(got), len(w))
                assert stats == ref[mode], (mode, wpb, qt, t, tri, stats, ref[mode])
            # row ranges: the same rows of the whole result, sliced and packed alike
            for lo, hi in ((0, 33), (64, n // 2), (n // 2 - 1, n // 2), (n - 100, n)):
                sub = want_all[(want_all["i"] >= lo) & (want_all["i"] < hi)]
                for form, form_used in ((2, SLICED), (0, PACKED)):
                    got, _, used = run_form(sel, form, tau, MODE_SMH, r, b, rows=(lo, hi))
                    assert used == form_used and same_pairs(got, sub), (form, lo, hi, wpb, qt, t)


def test_sliced_join_interleave_and_chunk_lanes(oracle):
    """interleaved row blocks (the multi-rank partition) and chunk lanes: the parts tile the whole result, under the sliced join"""
    for name, tau, shape in (("synth_flat_n300_m512", 0.5, (8, 64)), ("synth_flat_n1000_m256", 0.9, (8, 32)), ("synth_spread_n600_m64", 0.5, (4, 16))):
        cfg, hll, aux, cards = sorted_set(name, oracle)
        r, b = shape
        want, st = oracle.select(hll, aux, cards, tau, r, b)
        with Selector(0) as sel:
            sel.upload(hll, aux, cards)
            sel.set_param("join_form", 2)
            for lanes in (0, 2, 3):
                sel.set_pipeline(lanes)
                assert same_pairs(sel.run(tau, MODE_CB_SMH, r, b, algo=ALGO_SIG), want)
                assert sel.get_param("join_form_used") == SLICED
                for block, parts in ((32, 3), (64, 2), (96, 4)):
                    got, evaluated = [], 0
                    for part in range(parts):
                        sel.set_row_interleave(block, parts, part)
                        got.append(sel.run(tau, MODE_CB_SMH, r, b, algo=ALGO_SIG))
                        assert sel.get_param("join_form_used") == SLICED
                        evaluated += sel.stats()["evaluated"]
                    sel.set_row_interleave(0, 1, 0)
                    cat = np.concatenate(got)
                    assert same_pairs(cat[np.lexsort((cat["k"], cat["i"]))], want), (lanes, block, parts)
                    assert evaluated == st["evaluated"]
            sel.set_pipeline(-1)


def test_sliced_join_fallbacks_and_parameters(oracle):
    """shapes the tiled build does not take (r = 64, "sig_tile" = 0) run the packed form; 15-bit signatures and the DPP join keep their
    own kernels; join_form and join_t refuse other values"""
    cfg, hll, aux, cards = sorted_set("synth_flat_n300_m512", oracle)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        with pytest.raises(Exception):
            sel.set_param("join_form", 3)
        with pytest.raises(Exception):
            sel.set_param("join_form", -1)
        with pytest.raises(Exception):
            sel.set_param("join_t", 3)
        with pytest.raises(Exception):
            sel.set_param("join_t", -1)
        for tau, (r, b), setting, expect in ((0.5, (64, 8), None, PACKED), (0.5, (8, 64), ("sig_tile", 0), PACKED),
                                             (0.5, (8, 64), ("join_bits", 15), 1), (0.5, (8, 64), ("join_q", 0), -1),
                                             (0.5, (8, 64), None, SLICED)):
            want, st = oracle.select(hll, aux, cards, tau, r, b)
            if setting:
                sel.set_param(*setting)
            sel.set_param("join_form", 2)
            got = sel.run(tau, MODE_CB_SMH, r, b, algo=ALGO_SIG)
            assert sel.get_param("join_form_used") == expect, (r, b, setting)
            assert same_pairs(got, want) and sel.stats()["survivors"] == st["survivors"]
            sel.set_param("sig_tile", 1); sel.set_param("join_bits", 16); sel.set_param("join_q", 1)


def test_sliced_join_signature_cache(oracle):
    """"sig_cache" = 1 while the layout changes between passes: packed, sliced, 15-bit and zero-half joins must each read words written
    for them (the layout is part of the cache key)"""
    cfg, hll, aux, cards = sorted_set("synth_flat_n300_m512", oracle)
    with Selector(0) as sel:
        sel.set_param("sig_cache", 1)
        sel.upload(hll, aux, cards)
        cand = {}
        for tau, shape in ((0.5, (8, 64)), (0.5, (4, 128)), (0.8, (16, 32))):
            r, b = shape
            want, st = oracle.select(hll, aux, cards, tau, r, b)
            want_all, _ = oracle.select(hll, aux, cards, tau, r, b, use_cb=False)
            for form, bits, expect in ((2, 16, SLICED), (0, 16, PACKED), (2, 16, SLICED), (2, 16, SLICED), (2, 15, 1), (2, 16, SLICED),
                                       (1, 16, 2), (2, 16, SLICED), (0, 16, PACKED), (0, 15, 1), (0, 16, PACKED)):
                sel.set_param("join_bits", bits)
                got, stats, used = run_form(sel, form, tau, MODE_CB_SMH, r, b)
                assert used == expect and same_pairs(got, want), (shape, form, bits)
                assert stats[:2] == (st["evaluated"], st["survivors"])
                if bits == 16:
                    assert cand.setdefault(shape, stats[2]) == stats[2], (shape, form)
                got, _, used = run_form(sel, form, tau, MODE_SMH, r, b, rows=(40, 211))
                assert same_pairs(got, want_all[(want_all["i"] >= 40) & (want_all["i"] < 211)]), (shape, form, bits)
        sel.set_param("join_bits", 16)


def test_sliced_join_full_size_cfg3():
    """BASELINE configs[2] at full size (10 000 genomes, m = 512, tau = 0.8): the sliced join against the packed one, bit for bit"""
    cfg = pkg.SYNTH_CONFIGS["cfg3"]
    hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg)
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        sel.attach(hll_t, aux_t, cards_t)
        for mode in (MODE_CB_SMH, MODE_SMH):
            a, sa, ua = run_form(sel, 0, cfg.tau, mode, r, b)
            c, sc, uc = run_form(sel, 2, cfg.tau, mode, r, b)
            assert (ua, uc) == (PACKED, SLICED)
            assert len(a) > 0 and sa == sc, (mode, sa, sc)
            assert a.shape == c.shape and np.array_equal(a["i"], c["i"]) and np.array_equal(a["k"], c["k"])
            assert np.array_equal(a["jaccard"].view(np.uint64), c["jaccard"].view(np.uint64))
