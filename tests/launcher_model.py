"""The contract of the drop-in launchers on an EXPLICIT pair list (include/selection_hip.h section 1; launch_kernel_smh, launch_kernel_CBsmh
and their 64-bit twins), entry by entry and in the orientation listed -- from the oracle's primitives (orc_cb, orc_smh_a, the J of
orc_select, truncated cards), nothing from the library under test:

    an entry {x, y} is LIVE    iff (size_t)cards[y] != 0 and, for CBsmh, (double)(size_t)cards[x] / (double)(size_t)cards[y] >= tau
                               -- x over y as listed: a reversed entry {larger, smaller} has a ratio >= 1; x empty is cut at tau > 0
    a live entry gives the record {x, y, (float)J}, x and y as listed, once per occurrence,
                               iff some band of the two rows is equal and J = (e_x + e_y - t) / t >= tau

Nothing is deduplicated, no rank is checked, `cards` need not be ascending, and x == y is no special case (every band is equal, t is the
estimate of the sketch's own registers)."""
import numpy as np

import sig_model as S

CB_SAMPLE = 4096                              # entries whose numpy CB verdict is checked against orc_cb on every call


def live(oracle, cards, pairs, tau, use_cb):
    """bool per entry"""
    e = S.trunc_cards(cards)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    ex, ey = e[pairs[:, 0]], e[pairs[:, 1]]
    out = ey != 0
    if use_cb:
        with np.errstate(divide="ignore", invalid="ignore"):
            out = out & ((ex.astype(np.float64) / ey.astype(np.float64)) >= np.float64(np.float32(tau)))
        step = max(1, len(pairs) // CB_SAMPLE)
        for j in range(0, len(pairs), step):
            assert bool(out[j]) == (ey[j] != 0 and oracle.cb(tau, ex[j], ey[j])), j
    return out


def per_entry(oracle, hll, aux, cards, pairs, n_rows, n_bands, p=14):
    """(band_equal bool [P], J float64 [P], NaN where no band is equal or e_y == 0) by one oracle call per entry"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    e = S.trunc_cards(cards)
    eq = np.zeros(len(pairs), dtype=bool)
    J = np.full(len(pairs), np.nan)
    memo = {}
    for j, (x, y) in enumerate(pairs.tolist()):
        key = (min(x, y), max(x, y))                                          # (orc_smh_a and J are symmetric)
        if key not in memo:
            band = oracle.smh_a(aux[x], aux[y], n_rows, n_bands)
            jac = None
            if band and e[x] + e[y] != 0:
                a, b = (x, y) if e[y] != 0 else (y, x)                        # (orc_select skips a pair whose second card is 0)
                jac = oracle.jaccard(hll[a], hll[b], cards[a], cards[b], p)
            memo[key] = (band, np.nan if jac is None else jac)
        eq[j], J[j] = memo[key]
    return eq, J


def expected(oracle, cards, pairs, tau, use_cb, band_equal, J):
    """int32 [R, 3]: the records {x, y, float32 bits of J} of one launcher call, sorted; band_equal and J per entry (per_entry, or
    matrices of the whole set indexed by the entries)"""
    pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        sel = live(oracle, cards, pairs, tau, use_cb) & band_equal & (J >= np.float64(np.float32(tau)))
    rec = np.empty((int(sel.sum()), 3), dtype=np.int32)
    rec[:, :2] = pairs[sel]
    rec[:, 2] = J[sel].astype(np.float32).view(np.int32)
    return sort_records(rec)


def sort_records(rec):
    """the records as a multiset: rows sorted by (x, y, bits)"""
    rec = np.asarray(rec, dtype=np.int32).reshape(-1, 3)
    return rec[np.lexsort((rec[:, 2], rec[:, 1], rec[:, 0]))]


def awkward_set(oracle, p=10, n=48, m=64, seed=137):
    """(hll, aux, cards, empty, twin) in an order in which `cards` is NOT ascending, with one empty sketch (genome `empty`, card 0)
    whose SuperMinHash row is genome `twin`'s -- so entries with it have an equal band"""
    import precision_model as pm
    hll, aux, cards = (a.copy() for a in pm.sketch_set(p, n, m, seed))
    order = np.random.default_rng([seed, 5]).permutation(n)
    hll, aux, cards = hll[order], aux[order], cards[order]
    empty, twin = 7, 23
    hll[empty] = 0
    aux[empty] = aux[twin]
    cards[empty] = oracle.report(hll[empty], p)
    assert cards[empty] == 0 and np.any(np.diff(cards) < 0) and np.all(np.delete(cards, empty) >= 1)
    return hll, aux, cards, empty, twin


def awkward_list(n, empty, seed=11, repeats=1500):
    """every ordered pair of the n genomes, x == y included (so both orientations, the empty sketch as x and as y), plus `repeats`
    entries listed again, shuffled"""
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    L = np.stack([x.ravel(), y.ravel()], axis=1).astype(np.int32)
    L = np.concatenate([L, L[rng.integers(0, len(L), repeats)]])
    return np.ascontiguousarray(L[rng.permutation(len(L))])
