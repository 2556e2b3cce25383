"""One sketch set whose pair list has more than 2^20 DISTINCT entries, and what passes over prefixes of that list must give -- in numpy and
the oracle, nothing here comes from the library under test.

The pair-list kernels (csrc/kernel_pairs.cuh) and the drop-in launchers (csrc/abi_compat.inc) take their launch shape from the list's
length: gpw = clamp(P / 32 768, 1, 16) groups of four entries per wave and batch (pairs_direct_shape, csrc/host_plan.hpp), a grid of at
most 1 024 blocks -- a second trip of the grid-stride loop beyond 524 288 entries -- and launcher chunks of 2^20 entries.  LENGTHS sit
on those edges.  The list is the whole triangle of N = 1 500 genomes, every entry in a random orientation, shuffled: a record {i, k, J}
names exactly one entry, so a verdict read from the wrong group, quarter, wave, batch or chunk shows up as a wrong set of records.

    main sketches   p_hll = 10 (the oracle's all-pairs pass stays short); the genomes are subsets of eight cores of 20 000 hashes, a
                    few of them twenty times smaller than the rest, so J spreads over (0, 1) and the CB bound cuts some entries
    SuperMinHash    m = 64 as 16 bands of 4 buckets; every band of every genome is one of 32 values of that band's pool, with one of
                    two last buckets: a pair has an equal band with probability 1 - (63/64)^16 = 0.22, and as many bands again are
                    equal in all but their last bucket
    J               the oracle's all-pairs pass (FMA flavour) with bands of ONE bucket and tau = -1: the J of every pair with an equal
                    bucket, which every pair that a band test or a count threshold >= 1 passes has

The per-entry predicates are those of in_E and Ref.literal in test_pairlist_gpu.py: truncated cards, the CB ratio in float64 against
(double)(float)tau (checked against orc_cb on a sample), sig_model.literal_matrix, sig_model.band_sigs."""
import functools

import numpy as np

import precision_model as pm
import sig_model as S
from smh_matrix_model import match_counts

from cuda_selection_criteria_amd import PAIR_DTYPE

N, M, P_HLL = 1500, 64, 10
RB = (4, 16)                                  # rows per band, bands: a shape with band signatures (the signature route takes it)
TAU_CB = 0.5                                  # the "real" tau of the MODE_CB_SMH cases
SEED = 0x5CA1E
TOTAL = N * (N - 1) // 2                      # 1 124 250
CHUNK = 1 << 20                               # kCompatChunk (csrc/abi_compat.inc)
ONE_GRID = 1024 * 512                         # entries of one trip of the lane-per-entry kernels, and of the others at gpw = 16
# length: what it reaches
LENGTHS = {65535: "last length with gpw = 1", 65536: "gpw = 2", 65537: "gpw = 2", 98305: "gpw = 3", 491537: "gpw = 15",
           524288: "gpw = 16, exactly one grid", 524289: "first entry of a second trip", 1048613: "well into the second trip",
           TOTAL: "the whole list"}
BEYOND_ONE_GRID = (524289, 1048613, TOTAL)
N_CORES, CORE_ITEMS = 8, 20000
ODD_M, ODD_RB = 68, (17, 4)                   # bands that straddle the 16-bucket steps of pairs_direct_kernel


def direct_shape(P):
    """(gpw, grid) of pairs_direct_shape (csrc/host_plan.hpp), restated"""
    gpw = min(16, max(1, P // (4 * 1024 * 8)))
    return gpw, min(1024, max(1, -(-P // (32 * gpw))))


def flat_grid(P):
    """the grid of the kernels of one lane per entry (pairs_filter_kernel, pairs_verify_kernel)"""
    return min(1024, max(1, -(-P // 512)))


def trips(P, gpw=None):
    """trips of the grid-stride loop the busiest block makes"""
    per_block = 512 if not gpw else 32 * gpw
    return -(-(-(-P // per_block)) // 1024)


def band_pool_rows(rng, n, r, nb, pool=32):
    """u64 [n, r * nb]: band b of a row is pool value base[b] (r buckets) with one of two last buckets"""
    values = rng.integers(1, 1 << 62, size=(nb, pool, r), dtype=np.uint64)
    other_last = rng.integers(1, 1 << 62, size=(nb, pool), dtype=np.uint64)
    base = rng.integers(0, pool, size=(n, nb))
    variant = rng.integers(0, 2, size=(n, nb))
    band = np.arange(nb)[None, :]
    rows = values[band, base].copy()                                         # [n, nb, r]
    rows[..., r - 1] = np.where(variant == 1, other_last[band, base], rows[..., r - 1])
    return np.ascontiguousarray(rows.reshape(n, r * nb))


def cb_matrix(e, tau):
    """bool [n, n]: (double)e[a] / (double)e[b] >= (double)(float)tau, a over b as indexed"""
    ed = e.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (ed[:, None] / ed[None, :]) >= np.float64(np.float32(tau))


def records(i, k, j):
    rec = np.zeros(len(i), dtype=PAIR_DTYPE)
    rec["i"], rec["k"], rec["jaccard"] = i, k, j
    return rec[np.lexsort((rec["k"], rec["i"]))]


def j_matrix(n, pairs):
    """float64 [n, n], NaN where the oracle's list has no record: J of its pairs at [i, k], i < k"""
    J = np.full((n, n), np.nan)
    J[pairs["i"], pairs["k"]] = pairs["jacc"]
    return J


class Scale:
    def __init__(self, oracle):
        self.oracle = oracle
        rng = np.random.default_rng([SEED, N])
        cores = rng.integers(0, 1 << 64, size=(N_CORES, CORE_ITEMS), dtype=np.uint64)
        hll = np.zeros((N, 1 << P_HLL), dtype=np.uint8)
        for g in range(N):
            share = rng.uniform(0.06, 0.1) if rng.random() < 0.04 else rng.uniform(0.4, 1.0)
            keep = cores[rng.integers(N_CORES)][rng.random(CORE_ITEMS) < share]
            own = rng.integers(0, 1 << 64, size=len(keep) // 20 + 1, dtype=np.uint64)
            hll[g] = pm.registers(np.concatenate([keep, own]), P_HLL)
        aux = band_pool_rows(rng, N, *RB)
        odd = band_pool_rows(rng, N, *ODD_RB)
        cards, perm = pm.rank_order(hll, P_HLL)
        self.hll, self.aux, self.odd_base, self.cards = (np.ascontiguousarray(a[perm]) for a in (hll, aux, odd, cards))
        self.e = S.trunc_cards(self.cards)
        assert np.all(np.diff(self.cards) >= 0) and self.e[0] > 1000
        # the list: the whole triangle, random orientation, shuffled
        ii, kk = np.triu_indices(N, 1)
        L = np.stack([ii, kk], axis=1).astype(np.int32)
        flip = rng.random(len(L)) < 0.5
        L[flip] = L[flip][:, ::-1]
        self.L = np.ascontiguousarray(L[rng.permutation(len(L))])
        assert len(self.L) == TOTAL > CHUNK and 0.4 < flip.mean() < 0.6
        self.lo, self.hi = self.L.min(axis=1).astype(np.int64), self.L.max(axis=1).astype(np.int64)
        # per pair, then per entry
        self.lit = S.literal_matrix(self.aux, self.aux, *RB)[self.lo, self.hi]
        self.cnt = match_counts(self.aux, self.aux)[self.lo, self.hi]
        sg = S.band_sigs(self.aux, *RB)
        self.sig = S.sig_match_matrix(sg, sg)[self.lo, self.hi]
        oracle.set_fma(1)
        pairs, st = oracle.select(self.hll, self.aux, self.cards, -1.0, 1, M, use_cb=False, p=P_HLL)
        assert st["evaluated"] == TOTAL and st["survivors"] == len(pairs) == int((self.cnt >= 1).sum())
        self.J = j_matrix(N, pairs)[self.lo, self.hi]
        assert not np.isnan(self.J[self.cnt >= 1]).any() and np.isnan(self.J[self.cnt == 0]).all()
        self._E = {}
        self._check_inputs()

    # ---- conditions on the inputs (asserted on the reference, before any GPU call) ---------------------------------------------------
    def _check_inputs(self):
        share = float(self.lit.mean())
        assert 0.05 <= share <= 0.5, share
        assert int((self.sig & ~self.lit).sum()) >= 0 and bool((self.lit <= self.sig).all())     # an equal band has an equal signature
        assert int((self.cnt[~self.lit] >= 3).sum()) > 1000                   # bands equal in all but the last bucket
        # both verdicts in every (group t, quarter) slot of a wave at gpw = 16: lane 4 t + quarter of the wave holds entry j, j % 64 = lane
        for slot in range(64):
            v = self.lit[slot::64]
            assert v.any() and not v.all(), slot
        inside = self.in_E(TAU_CB, True)
        assert 0 < int((~inside).sum()) < int(inside.sum()), (int(inside.sum()), TOTAL)
        # the CB predicate of numpy is orc_cb, on a sample of the entries
        for j in range(0, TOTAL, 997):
            assert bool(inside[j]) == self.oracle.cb(TAU_CB, self.e[self.lo[j]], self.e[self.hi[j]]), j
        # the J matrix and the per-entry predicates reproduce the oracle's own smh_a pass under the CB bound
        want, st = self.oracle.select(self.hll, self.aux, self.cards, TAU_CB, *RB, use_cb=True, p=P_HLL)
        rec, wst = self.smh_a(TOTAL, TAU_CB, True)
        assert st["evaluated"] == wst["evaluated"] and st["survivors"] == wst["survivors"] and 100 < len(want) < wst["survivors"]
        assert np.array_equal(rec["i"], want["i"]) and np.array_equal(rec["k"], want["k"])
        assert np.array_equal(rec["jaccard"].view(np.uint64), want["jacc"].view(np.uint64))

    # ---- per-entry predicates -----------------------------------------------------------------------------------------------------------
    def in_E(self, tau, use_cb):
        """bool per entry of the whole list: e_hi != 0 and, under CB, e_lo / e_hi >= tau -- membership of the all-pairs pair space"""
        key = (float(np.float32(tau)), bool(use_cb))
        if key not in self._E:
            out = self.e[self.hi] != 0
            if use_cb:
                out = out & cb_matrix(self.e, tau)[self.lo, self.hi]
            self._E[key] = out
        return self._E[key]

    def _pass(self, P, tau, use_cb, ok, cand):
        inside = self.in_E(tau, use_cb)[:P]
        with np.errstate(invalid="ignore"):
            sel = inside & ok[:P] & (self.J[:P] >= np.float64(np.float32(tau)))
        return records(self.lo[:P][sel], self.hi[:P][sel], self.J[:P][sel]), {
            "evaluated": int(inside.sum()), "survivors": int((inside & ok[:P]).sum()), "selected": int(sel.sum()),
            "candidates": int((inside & cand[:P]).sum())}

    def smh_a(self, P, tau, use_cb, route="direct"):
        """(records, statistics) of a list pass of criterion smh_a over the first P entries"""
        return self._pass(P, tau, use_cb, self.lit, self.sig if route == "sig" else self.lit)

    def smh_c(self, P, tau, use_cb, need):
        """the same of criterion smh_c under the HLL estimator; need: the count every entry needs, int64 per entry of the whole list"""
        ok = self.cnt >= need
        return self._pass(P, tau, use_cb, ok, ok)

    def need(self, c_min=None, gamma=None, floor=0):
        """int64 per entry of the whole list: the count an entry needs -- max(floor, c_min if set, smhcc_model.threshold if gamma is set)"""
        import smhcc_model as CC
        out = np.full(TOTAL, max(int(floor), int(c_min or 0)), dtype=np.int64)
        if gamma is not None:
            e_x, e_y = self.e[self.lo], self.e[self.hi]
            out = np.maximum(out, CC.threshold(M, gamma, np.minimum(e_x, e_y), np.maximum(e_x, e_y)))
        return out

    def smh_v(self, P, tau, use_cb, measure, c_min=None, gamma=None):
        """the same under the SuperMinHash estimator: smhv_model.expected_list on the counts this set already has (the model itself
        gathers both rows of every entry: 1.1 GB for the whole list; the test holds this restatement to it on a prefix)"""
        import smhv_model as V
        inside = self.in_E(tau, use_cb)[:P]
        lo, hi = self.lo[:P], self.hi[:P]
        val = V.value(measure, M, self.cnt[:P], self.e[lo], self.e[hi])
        ok = self.cnt[:P] >= self.need(c_min, gamma, floor=1)[:P]
        with np.errstate(invalid="ignore"):
            sel = inside & ok & (val >= np.float64(np.float32(tau)))
        surv = int((inside & ok).sum())
        return records(lo[sel], hi[sel], val[sel]), {"evaluated": int(inside.sum()), "survivors": surv, "selected": int(sel.sum()),
                                                     "candidates": surv}

    # ---- the odd band shape ---------------------------------------------------------------------------------------------------------------
    @functools.cached_property
    def odd(self):
        """(aux u64 [N, 68], planted pairs, near pairs, literal per entry, J per entry) for 17 x 4: the first, the last and a straddling
        band planted as test_direct_route_any_band_shape plants them"""
        r, nb = ODD_RB
        aux = self.odd_base.copy()
        straddling = [b for b in range(nb) if (b * r) // 16 != (b * r + r - 1) // 16]
        plant = {"first": 0, "last": nb - 1, "straddle": straddling[len(straddling) // 2]}
        fresh = np.random.default_rng([SEED, 68]).integers(1, 1 << 62, size=(12, ODD_M), dtype=np.uint64)
        aux[:12] = fresh                                                      # twelve rows that share nothing with anyone
        planted, near = [], []
        for g, band in zip(range(0, 12, 4), plant.values()):
            aux[g + 1, band * r:(band + 1) * r] = aux[g, band * r:(band + 1) * r]
            planted.append((g, g + 1))
            aux[g + 3, band * r:(band + 1) * r - 1] = aux[g + 2, band * r:(band + 1) * r - 1]
            near.append((g + 2, g + 3))
        for (a, b), (c, d) in zip(planted, near):
            assert self.oracle.smh_a(aux[a], aux[b], r, nb) and not self.oracle.smh_a(aux[c], aux[d], r, nb)
        lit = S.literal_matrix(aux, aux, r, nb)[self.lo, self.hi]
        pairs, st = self.oracle.select(self.hll, aux, self.cards, -1.0, r, nb, use_cb=False, p=P_HLL)
        assert st["survivors"] == len(pairs) == int(lit.sum())
        return aux, planted, near, lit, j_matrix(N, pairs)[self.lo, self.hi]


_SCALE = []


def scale(oracle):
    """the set, built once per session"""
    if not _SCALE:
        _SCALE.append(Scale(oracle))
    return _SCALE[0]
