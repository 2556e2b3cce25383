"""verify16_batch (csrc/kernel_verify.cuh) issues every load of a half-batch unconditionally, at a clamped index, and applies the lane
conditions to the loaded bits.  These tests pin the places where that could go wrong, on the planted set of tests/sig_model.py
(N = 200 genomes, as in test_sig_collisions_gpu.py) with further pairs planted on the genomes that set leaves alone:

  band position   a pair whose ONLY equal band is the first band, the last band of lane 15's first signature group (63), the first
                  band of the second group (64) or the last band (127 of 128): the clamped group index and the `sub < nq` masks;
                  and a pair whose first flagged band is a collision and whose equal band comes later
  row remainder   bands of 32, 64, 128 buckets equal in all but bucket r - 1, or all but bucket 16, with an equal signature: the
                  batched remainder loop over the buckets sub + 16, sub + 32, ...; candidates, never survivors
  partial batches pair lists of 0 .. 513 entries -- live quarters beside dead ones -- ending in a forged collision and a true pair
  grouping inputs the all-pairs pass at the default settings: verify16_kernel tallies row_cnt / row_lab for stage 2's grouping

Both routes through the shared body run: the all-pairs ALGO_SIG pass (verify16_kernel) and the pair-list signature route
(pairs_verify_kernel), with "verify_fb" 0 and 1.  Expected values: the oracle's pairs and J bits, the oracle's survivor count, the
model's candidate count."""
import copy

import numpy as np
import pytest

import sig_model as S
import test_sig_collisions_gpu as SC
from test_pairlist_gpu import as_dict, in_E, records_of

from cuda_selection_criteria_amd import ALGO_SIG, Selector

pytestmark = pytest.mark.gpu

N = SC.N
BAND_SHAPES = ((128, 8, 16), (512, 8, 64), (512, 4, 128))
ROW_SHAPES = ((512, 32, 16), (512, 64, 8), (1024, 128, 8))
LENGTHS = (0, 1, 3, 4, 5, 63, 64, 65, 511, 512, 513)
_CACHE = {}


def ids(shapes):
    return [f"{r}x{nb}" for _, r, nb in shapes]


def band_positions(nb):
    """the first band, band 63 (4 * 15 + 3: the last band of lane 15's first 16-byte group), 64 (the first of the second group), and
    the last band, as far as the shape has them"""
    return sorted({0, nb - 1} | ({63} if nb >= 64 else set()) | ({64, 127} if nb == 128 else set()))


def forge_at(values, pos, target, rng):
    """uint64[r]: `values` with bucket `pos` solved for so that the band has the 32-bit signature `target` (sig_model.forge_last solves
    the last bucket; the signature is a sum over the buckets, so any one of them can be solved for)"""
    vals = [int(v) for v in values]
    lo_p = hi_p = 0
    for j, v in enumerate(vals):
        if j != pos:
            x = S.mix64((v + S.GOLD * (j + 1)) & S.MASK64)
            lo_p += x & S.MASK32
            hi_p += x >> 32
    lo_t = int(rng.integers(0, 1 << 32))
    hi_t = lo_t ^ (int(target) & S.MASK32)
    x = (((hi_t - hi_p) & S.MASK32) << 32) | ((lo_t - lo_p) & S.MASK32)
    vals[pos] = (S.unmix64(x) - S.GOLD * (pos + 1)) & S.MASK64
    out = np.array(vals, dtype=np.uint64)
    assert S.band_sig(out) == int(target) & S.MASK32
    return out


def plant_bands(aux, r, nb, take, rng):
    """{name: (i, k)}: one pair per band position equal in that band alone; one whose band 1 collides and whose band nb - 2 is equal"""
    mine = {}
    for b in band_positions(nb):
        i, k = take()
        aux[k, b * r:(b + 1) * r] = aux[i, b * r:(b + 1) * r]
        mine[f"only-{b}"] = (i, k)
    i, k = take()
    b0, b1 = 1, nb - 2
    src = aux[i, b0 * r:(b0 + 1) * r].copy()
    src[0] ^= np.uint64(int(rng.integers(1, 1 << 63)))
    aux[k, b0 * r:(b0 + 1) * r] = S.forge_last(src[:-1], S.band_sig(aux[i, b0 * r:(b0 + 1) * r]), rng)
    aux[k, b1 * r:(b1 + 1) * r] = aux[i, b1 * r:(b1 + 1) * r]
    mine["collision-then-equal"] = (i, k)
    return mine


def plant_rows(aux, r, nb, take, rng):
    """{name: (i, k)}: band nb - 1 equal in all but bucket r - 1, band 1 equal in all but bucket 16, signatures equal"""
    mine = {}
    for name, b, pos in (("all-but-last", nb - 1, r - 1), ("all-but-16", 1, 16)):
        i, k = take()
        want = aux[i, b * r:(b + 1) * r]
        while True:
            new = forge_at(want, pos, S.band_sig(want), rng)
            if new[pos] != want[pos]:
                break
        aux[k, b * r:(b + 1) * r] = new
        assert int((new != want).sum()) == 1
        mine[name] = (i, k)
    return mine


def variant(oracle, shape, plant):
    """the shape's Case of test_sig_collisions_gpu with `plant`'s pairs added on genomes of no planted pair; .mine names them"""
    key = (shape, plant.__name__)
    if key not in _CACHE:
        base = SC.case(oracle, *shape)
        good = SC._CACHE["base"][2]                                           # rank pairs that tau = 0 lists once they survive stage 1
        used = {g for p in base.P.pairs for g in p}
        free = [g for g in range(N) if g not in used]
        c = copy.copy(base)
        c.aux = base.aux.copy()

        def take():
            for i in free:
                for k in free:
                    if i < k and good[i, k]:
                        free.remove(i)
                        free.remove(k)
                        return i, k
            raise AssertionError("no free pair left")

        c.mine = plant(c.aux, base.r, base.nb, take, np.random.default_rng(0xBA7C + base.r))
        c.sg = S.band_sigs(c.aux, base.r, base.nb)
        c.lit = S.literal_matrix(c.aux, c.aux, base.r, base.nb)
        c.sig_match = S.sig_match_matrix(c.sg, c.sg)
        c._exp = {}
        _CACHE[key] = c
    return _CACHE[key]


def whole_triangle(seed):
    ii, kk = np.triu_indices(N, 1)
    return np.ascontiguousarray(np.stack([kk, ii], axis=1)[np.random.default_rng(seed).permutation(len(ii))], dtype=np.int32)


def check_both_routes(sel, c, L):
    """the all-pairs ALGO_SIG pass and the pair-list signature route over the whole triangle: the oracle's pairs, J bit for bit, the
    oracle's survivors, the model's candidates; returns the listed pairs of the tau = 0 pass"""
    listed = None
    for run in SC.RUNS:
        tau, mode, _ = SC.RUNS[run]
        want, _, survivors, cand = c.expect(run)
        got = SC.check_pass(sel, c, ALGO_SIG, run)
        st_all = sel.stats()
        lst = sel.run_pairs(L, tau, mode, c.r, c.nb, algo=ALGO_SIG)
        st = sel.stats()
        print(f"{c.r}x{c.nb} {run}: list route listed {len(lst)} / {len(want)} stats {st} all-pairs {st_all} model candidates {cand}")
        assert sel.get_param("pairs_route_used") == 1
        SC.assert_same_pairs(lst, want)
        assert st == st_all and st["survivors"] == survivors and st["candidates"] == cand
        if run == "smh":
            listed = set(zip(got["i"].tolist(), got["k"].tolist()))
    return listed


# ---- band position ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [0, 1])
@pytest.mark.parametrize("m,r,nb", BAND_SHAPES, ids=ids(BAND_SHAPES))
def test_band_position(oracle, m, r, nb, fb):
    c = variant(oracle, (m, r, nb), plant_bands)
    assert len(c.mine) == len(band_positions(nb)) + 1
    for name, (i, k) in c.mine.items():
        equal = (c.aux[i].reshape(nb, r) == c.aux[k].reshape(nb, r)).all(axis=1)
        flagged = c.sg[i] == c.sg[k]
        assert equal.sum() == 1 and c.lit[i, k], name
        if name == "collision-then-equal":
            assert flagged.sum() == 2 and flagged[1] and not equal[1] and equal[nb - 2]
        else:
            assert flagged.sum() == 1 and equal[int(name.split("-")[1])]
    with Selector(0) as sel:
        sel.set_param("verify_fb", fb)
        sel.upload(c.hll, c.aux, c.cards)
        listed = check_both_routes(sel, c, whole_triangle(r + nb))
    assert set(c.mine.values()) <= listed


# ---- row remainder ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [0, 1])
@pytest.mark.parametrize("m,r,nb", ROW_SHAPES, ids=ids(ROW_SHAPES))
def test_row_remainder(oracle, m, r, nb, fb):
    c = variant(oracle, (m, r, nb), plant_rows)
    base = SC.case(oracle, m, r, nb)
    for name, (i, k) in c.mine.items():
        assert c.sig_match[i, k] and not c.lit[i, k], name                    # a candidate, no survivor
        assert not base.lit[i, k] and not S.sig_match_matrix(base.sg[[i]], base.sg[[k]])[0, 0]
    with Selector(0) as sel:
        sel.set_param("verify_fb", fb)
        sel.upload(c.hll, c.aux, c.cards)
        for run in SC.RUNS:                                                   # the two pairs count among the candidates of a pass
            assert c.expect(run)[3] >= base.expect(run)[3]
        assert c.expect("smh")[3] == base.expect("smh")[3] + 2 and c.expect("smh")[2] == base.expect("smh")[2]
        listed = check_both_routes(sel, c, whole_triangle(r + nb))
    assert not set(c.mine.values()) & listed


# ---- partial batches on the pair-list route --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fb", [0, 1])
def test_partial_batches(oracle, fb):
    c = variant(oracle, (512, 8, 64), plant_bands)
    true_pair = c.mine["only-63"]
    collision = c.P.of("C1")[0]
    assert c.lit[true_pair] and c.sig_match[collision] and not c.lit[collision]
    rng = np.random.default_rng(513)
    x = rng.integers(0, N, max(LENGTHS), dtype=np.int32)
    y = ((x + rng.integers(1, N, max(LENGTHS), dtype=np.int32)) % N).astype(np.int32)      # never x
    filler = np.stack([x, y], axis=1)
    with Selector(0) as sel:
        sel.set_param("verify_fb", fb)
        sel.upload(c.hll, c.aux, c.cards)
        for run in SC.RUNS:
            tau, mode, use_cb = SC.RUNS[run]
            S_dict = as_dict(c.expect(run)[0])
            for P in LENGTHS:
                L = filler[:P].copy()
                if P >= 1:
                    L[P - 1] = true_pair[::-1]                                # the last entry: a true pair, larger rank first
                if P >= 2:
                    L[P - 2] = collision                                      # before it: a forged collision
                lo, hi = L.min(axis=1), L.max(axis=1)
                want = records_of(S_dict, lo, hi)
                inE = in_E(oracle, c.cards, tau, use_cb, lo, hi) if P else np.zeros(0, dtype=bool)
                got = sel.run_pairs(L, tau, mode, c.r, c.nb, algo=ALGO_SIG)
                st = sel.stats()
                print(f"fb={fb} {run} P={P}: records {len(got)} / {len(want)} stats {st}")
                assert got.shape[0] == want.shape[0]
                assert np.array_equal(got["i"], want["i"]) and np.array_equal(got["k"], want["k"])
                assert np.array_equal(got["jaccard"].view(np.uint64), want["jaccard"].view(np.uint64))
                assert st == {"evaluated": int(inE.sum()), "survivors": int((inE & c.lit[lo, hi]).sum()), "selected": len(want),
                              "candidates": int((inE & c.sig_match[lo, hi]).sum())}
                if run == "smh" and P >= 1:
                    listed = set(zip(got["i"].tolist(), got["k"].tolist()))
                    assert true_pair in listed and collision not in listed and st["survivors"] >= 1
                    assert P < 2 or st["candidates"] > st["survivors"]


# ---- grouping inputs -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,r,nb", BAND_SHAPES, ids=ids(BAND_SHAPES))
def test_grouping_inputs(oracle, m, r, nb):
    """the default settings of the suite's contexts group the survivors by row for stage 2: verify16_kernel counts them per row
    (row_cnt) and records every row's smallest partner (row_lab) while it appends"""
    c = variant(oracle, (m, r, nb), plant_bands)
    with Selector(0) as sel:
        sel.upload(c.hll, c.aux, c.cards)
        for run in SC.RUNS:
            tau, mode, _ = SC.RUNS[run]
            want, evaluated, survivors, _ = c.expect(run)
            got = sel.run(tau, mode, c.r, c.nb)
            st = sel.stats()
            print(f"{r}x{nb} {run}: default pass listed {len(got)} / {len(want)} stats {st} label_order {sel.get_param('label_order')}")
            SC.assert_same_pairs(got, want)
            assert st["evaluated"] == evaluated and st["survivors"] == survivors and st["selected"] == len(want)
            got = SC.check_pass(sel, c, ALGO_SIG, run)
            if run == "smh":
                assert set(c.mine.values()) <= set(zip(got["i"].tolist(), got["k"].tolist()))
