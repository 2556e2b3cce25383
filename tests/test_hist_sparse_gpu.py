"""Stage 2a's sparse lists ("hist_sparse" = 1; the automatic default takes them for sets whose planes fit the cache): the bit-plane kernel decodes only the values below the set's threshold T and takes
every register >= T from the two rows' lists.  Against "hist_sparse" = 0 (every value from the planes) on the same context -- the same
selected pairs, J bit for bit, the same counters -- on sets shaped like BASELINE configs[1] / configs[2], cfg3-spread, harden()ed sets and
the influenza fixtures; and against the oracle on adversarial rows: exactly 128 and 129 registers at the threshold, equal and unequal high
registers in both rows or in one, a whole plane dword of high registers, values up to 63 (six planes), tiny sets (T = 4) and sets whose
threshold would exceed 24 (the feature is off)."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

import cuda_selection_criteria_amd as pkg  # noqa: E402
from cuda_selection_criteria_amd import MODE_CB_SMH, MODE_SMH, Selector  # noqa: E402

sys.path.insert(0, str(GOLDEN))
EXP = GOLDEN / "expected"


def same_pairs(got, want):
    return (got.shape[0] == want.shape[0] and np.array_equal(got["i"], want["i"]) and np.array_equal(got["k"], want["k"])
            and np.array_equal(got["jaccard"].view(np.uint64), want["jaccard"].view(np.uint64)))


def run_both(sel, tau, mode, r, b):
    """(pairs, counters) with hist_sparse 0 and 1 on the same context, and the threshold the second run used"""
    out = []
    for on in (0, 1):
        sel.set_param("hist_sparse", on)
        got = sel.run(tau, mode, r, b)
        s = sel.stats()
        out.append((got, (s["evaluated"], s["survivors"], s["candidates"])))
        if not on:
            assert sel.get_param("hist_sparse_t") == 0
    return out[0], out[1], sel.get_param("hist_sparse_t")


@pytest.mark.parametrize("name,hard", [("cfg2", False), ("cfg3", False), ("cfg3-spread", False), ("cfg3", True), ("cfg2-spread", True)])
def test_synthetic_sets_sparse_equals_full(name, hard):
    cfg = pkg.SYNTH_CONFIGS[name]
    hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg, device=0)
    if hard:
        pkg.harden(aux_t)
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        sel.attach(hll_t, aux_t, cards_t)
        for group in (True, False):
            sel.set_stage2_grouping(group)
            for mode in (MODE_SMH, MODE_CB_SMH):
                (full, st_full), (sparse, st_sparse), t = run_both(sel, cfg.tau, mode, r, b)
                assert 4 <= t <= 24, t
                assert len(full) > 0 and same_pairs(sparse, full), (name, hard, group, mode, len(sparse), len(full))
                assert st_sparse == st_full
        if name == "cfg3" and not hard:
            assert t == 12                                   # 58-68 registers >= 12 per genome, more than 128 >= 8


def test_influenza_fixtures_sparse_equals_full():
    old = dict(Selector.DEFAULT_PARAMS)
    cwd = os.getcwd()
    os.chdir(GOLDEN)
    try:
        for a, h in ((512, 0.01), (2048, 0.9), (8192, 0.01)):
            want = (EXP / f"influenza_smh_a_a{a}_h{h}.fma.txt").read_text()
            for on in (0, 1):
                Selector.DEFAULT_PARAMS = {**old, "hist_sparse": on}
                assert pkg.select_from_filelist("influenza_filelist.txt", h, a) == want, (a, h, on)
    finally:
        Selector.DEFAULT_PARAMS = old
        os.chdir(cwd)


# ---- adversarial rows against the oracle ----------------------------------------------------------------------------------------------
def plane_dword_registers(o, lane):
    """the 32 registers that share one plane dword (hll_bitslice_kernel: register 4 ((8 o + jj) 64 + lane) + s -> bit 8 s + jj)"""
    return np.array([4 * ((8 * o + jj) * 64 + lane) + s for jj in range(8) for s in range(4)])


def adversarial_rows(kind, n=48, seed=0xAD5E):
    rng = np.random.default_rng(seed)
    base = np.minimum(rng.geometric(0.5, 16384) + 1, 11)                # ~256 registers >= 8 (so T > 8), nothing >= 12
    if kind == "tiny":
        base = np.minimum(base - 2, 3)                                  # only the planted registers reach 4
    rows = np.tile(base, (n, 1)).astype(np.int64)
    for g in range(n):                                                  # similar genomes: 2 % of the registers moved a little
        sel = rng.choice(16384, 330, replace=False)
        rows[g, sel] = np.clip(rows[g, sel] + rng.integers(-2, 3, sel.size), 0, 3 if kind == "tiny" else 11)
    hi_lo, hi_hi = (4, 8) if kind == "tiny" else (12, 16)
    # high registers: a shared pool (equal in some rows, larger or smaller in others) and private ones
    pool = rng.choice(16384, 60, replace=False)
    for g in range(n):
        take = pool[rng.random(pool.size) < 0.7]
        rows[g, take] = rng.integers(hi_lo, hi_hi, take.size) if g % 3 else hi_lo + 1
        own = rng.choice(16384, 20, replace=False)
        rows[g, own] = np.maximum(rows[g, own], rng.integers(hi_lo, hi_hi, own.size))
    # a whole plane dword of high registers in rows 0..3, with different values per row
    dw = plane_dword_registers(3, 17)
    for g in range(4):
        rows[g, dw] = hi_lo + (np.arange(32) + g) % 4
    if kind in ("cap128", "cap129"):
        row = rows[5]
        row[row >= 12] = 11
        k = 128 if kind == "cap128" else 129
        row[rng.choice(16384, k, replace=False)] = rng.integers(12, 16, k)
        rows[10:13, rng.choice(16384, 5, replace=False)] = 16 + np.arange(5)    # values >= 16 to take from the lists (T < khi)
    if kind == "six_planes":
        rows[7, rng.choice(16384, 6, replace=False)] = [40, 47, 52, 58, 61, 63]
        rows[8, rng.choice(16384, 3, replace=False)] = [33, 63, 45]
    if kind == "off":
        rows[9, rng.choice(16384, 129, replace=False)] = rng.integers(24, 30, 129)
    return rows.astype(np.uint8)


@pytest.mark.parametrize("kind,t_want", [("plain", 12), ("cap128", 12), ("cap129", 16), ("six_planes", 12), ("tiny", 4), ("off", 0)])
def test_adversarial_rows_vs_oracle(oracle, kind, t_want):
    hll = adversarial_rows(kind)
    n = hll.shape[0]
    if kind == "cap128":
        assert int((hll >= 12).sum(axis=1).max()) == 128
    if kind == "cap129":
        assert int((hll >= 12).sum(axis=1).max()) == 129
    cards = oracle.cards(hll)
    perm = pkg.sort_by_card(cards)
    hll, cards = hll[perm], cards[perm]
    m = 64
    aux = np.tile(np.arange(m, dtype=np.uint64), (n, 1))               # every pair passes every band: all pairs reach stage 2
    r, b = pkg.banding(m, 0.5)
    tau = 0.05
    want, st = oracle.select(hll, aux, cards, tau, r, b, use_cb=False)
    assert st["survivors"] == n * (n - 1) // 2 and len(want) > 0.9 * st["survivors"]
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        for run in (1, 4, 64):
            sel.set_param("hist_run", run)
            (full, st_full), (sparse, st_sparse), t = run_both(sel, tau, MODE_SMH, r, b)
            assert t == t_want, (kind, t)
            for got in (full, sparse):
                assert got.shape[0] == want.shape[0] and np.array_equal(got["i"], want["i"]) and np.array_equal(got["k"], want["k"])
                assert np.array_equal(got["jaccard"].view(np.uint64), want["jacc"].view(np.uint64)), (kind, run)
            assert st_sparse == st_full and st_full[:2] == (st["evaluated"], st["survivors"])
        # the dense walk (every XCD walks the whole list) and a list of single pairs
        sel.set_param("hist_run", 0)
        sel.set_param("hist_dense_degree", 0)
        (full, _), (sparse, _), _ = run_both(sel, tau, MODE_SMH, r, b)
        assert same_pairs(sparse, full)


def test_hist_sparse_param():
    with Selector(0) as sel:
        with pytest.raises(pkg.SelhipError):
            sel.set_param("hist_sparse", 2)
        assert sel.get_param("hist_sparse_t") == 0                     # nothing loaded
        hll = adversarial_rows("plain", n=8)
        aux = np.tile(np.arange(64, dtype=np.uint64), (8, 1))
        sel.upload(hll, aux, None)
        assert sel.get_param("hist_sparse_t") == 12                    # automatic: 8 genomes' planes fit the cache
        sel.set_param("hist_sparse", 0)
        assert sel.get_param("hist_sparse_t") == 0
        sel.set_param("hist_sparse", 1)
        assert sel.get_param("hist_sparse_t") == 12
        sel.set_param("hist_algo", 0)                                  # byte rows: no planes, no lists
        assert sel.get_param("hist_sparse_t") == 0
