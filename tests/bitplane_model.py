"""Forged HLL-14 register sets that take stage 2a's bit-plane code (csrc/kernel_hllbs.cuh) through every instantiation, and the numpy
model of what decides the instantiation: the plane count NB from the set's largest register, the sparse threshold T (so G1 = T / 4) from
the per-genome counts of high registers, the optional walks of bs_pair_hist from the two rows' largest registers.  No GPU, no library:
numpy alone (the oracle is passed in where a set has to be ranked).

  grid_set(vmax, T)     a set whose largest register is vmax and whose sparse threshold is T: one (NB, G1) cell
  ladder_set(vmax)      genomes whose largest registers run over LADDER (cut at vmax): every walk boundary of bs_pair_hist, with the larger
                        maximum in the first row, the second row and both
  flat_rows()           rows of 16 384 equal registers: one union bin holds 16 384 through each of bs_decode's four count formulas
"""
import numpy as np

CAP = 128                                                   # kBsSparseCap: entries of a genome's sparse list
LADDER = (3, 15, 16, 23, 24, 31, 32, 47, 48, 51)            # gmax values: both sides of kp = 16|17, 24|25, 32|33, 48|49
M_AUX = 64
# the (vmax, T) cells of hll_union_hist_bs_kernel<NB, G1 = T / 4>: NB = 4 with G1 1..3, NB = 5 with 1..5, NB = 6 with 1..6
GRID_ON = [(15, t) for t in (4, 8, 12)] + [(31, t) for t in (4, 8, 12, 16, 20)] + [(51, t) for t in (4, 8, 12, 16, 20, 24)]
GRID_OFF = [(31, 24), (15, 16)]                             # five planes with T > 20; T >= khi
FLAT_VALUES = (24, 29, 34, 51)                              # v mod 4 = 0, 1, 2, 3; one per walk above 24, two in the first
_BASE_SEED = 0xB17B


# ---- the model -------------------------------------------------------------------------------------------------------------------
def khi(hll):
    """largest register value + 1 (registers are taken modulo 64); 0 for no genomes"""
    return int((np.asarray(hll) & 63).max()) + 1 if np.asarray(hll).size else 0


def planes(k):
    return 4 if k <= 16 else 5 if k <= 32 else 6


def sparse_t(hll, k):
    """the threshold the all-pairs stage 2a uses with "hist_sparse" = 1; 0 = every value from the planes"""
    hll = np.asarray(hll) & 63
    for t in range(4, 28, 4):
        if int((hll >= t).sum(axis=1).max()) <= CAP:
            break
    else:
        return 0
    if t >= k or (t > 20 and k <= 32):
        return 0
    return t


def union_hist(a, b):
    return np.bincount(np.maximum(a, b) & 63, minlength=64)[:64].astype(np.uint32)


def kp_class(kp):
    return 0 if kp <= 24 else 1 if kp <= 32 else 2 if kp <= 48 else 3


def walk_cells(gx, gy):
    """{(kp class, side)} of the pairs (gx[j], gy[j]) of largest registers: side 0 = the first row holds the larger maximum, 1 = the
    second, 2 = both the same"""
    gx, gy = np.asarray(gx, dtype=np.int64), np.asarray(gy, dtype=np.int64)
    return {(kp_class(int(max(a, b)) + 1), 0 if a > b else 1 if b > a else 2) for a, b in zip(gx.tolist(), gy.tolist())}


def prefetch_steps(level, step=4):
    """{(kp class of a row's p-th pair, of its (p + step)-th)} over the rows x of a ranked set, whose pairs are (x, x + 1 + p): a wave of
    the one-launch small pass takes every step-th pair of a row's list and asks for the next one's kp while it decodes the current"""
    level = np.asarray(level, dtype=np.int64)
    out = set()
    for x in range(len(level)):
        kp = np.maximum(level[x], level[x + 1:]) + 1
        out |= {(kp_class(int(a)), kp_class(int(b))) for a, b in zip(kp[:-step].tolist(), kp[step:].tolist())}
    return out


def walk_cells_allowed(levels_x, levels_y, same_set):
    """the cells that sets with these gmax levels can reach: every (a, b) of levels_x x levels_y (a set against itself: both orders of
    two different levels, and a level with itself, of which it has two genomes)"""
    out = set()
    for a in levels_x:
        for b in levels_y:
            out |= walk_cells([a], [b])
            if same_set:
                out |= walk_cells([b], [a])
    return out


# ---- forged sets -----------------------------------------------------------------------------------------------------------------
def _base():
    return np.random.default_rng(_BASE_SEED).integers(0, 4, 16384).astype(np.int64)


def _pool(size):
    return np.random.default_rng(_BASE_SEED + 1).choice(16384, size, replace=False)


def _rows(n, rng, redraw):
    """similar genomes with every register in 0..3: one base row, `redraw` registers per genome drawn again"""
    rows = np.tile(_base(), (n, 1))
    for g in range(n):
        sel = rng.choice(16384, redraw, replace=False)
        rows[g, sel] = rng.integers(0, 4, redraw)
    return rows


def grid_set(vmax, t, n=24, seed=0):
    """n genomes (unranked, u8) with largest register vmax and sparse threshold t (t > vmax: no register reaches it).  Every value group
    below t holds registers too: the groups the sparse kernel still decodes from the planes all carry counts"""
    rng = np.random.default_rng([seed, vmax, t])
    rows = _rows(n, rng, 400)
    pool = _pool(90)
    free = np.setdiff1d(np.arange(16384), pool)
    lo = t if t <= vmax else t - 4
    if t > 4:                                                # 129 registers just below t in one genome: t - 4 leaves too many
        sel = rng.choice(free, 129, replace=False)
        rows[1, sel] = rng.integers(t - 4, min(t, vmax + 1), 129)
    mid = free[np.random.default_rng(_BASE_SEED + 3).choice(free.size, 40, replace=False)]
    for g in range(n):                                       # the shared high registers: equal, larger, smaller, absent over the pairs
        take = pool[rng.random(pool.size) < 0.6]
        rows[g, take] = rng.integers(lo, vmax + 1, take.size)
        if t > 4:                                            # and shared registers below t: every group the dense decode keeps holds counts
            take = mid[rng.random(mid.size) < 0.6]
            rows[g, take] = rng.integers(4, min(t, vmax + 1), take.size)
    rows[0, rng.choice(free, 1)] = vmax
    return rows.astype(np.uint8)


def ladder_levels(vmax):
    return [v for v in LADDER if v <= vmax]


def per_level_for(vmax, min_pairs):
    """genomes per level so that the set has at least min_pairs pairs (and two per level)"""
    k, per = len(ladder_levels(vmax)), 2
    while (k * per) * (k * per - 1) // 2 < min_pairs:
        per += 1
    return per


def ladder_per(vmax):
    """genomes per level of the ladder sets that the pair-list and count tests use: at least 60 pairs"""
    return per_level_for(vmax, 60)


def ladder_set(vmax, n_per_level=2, seed=0):
    """(rows u8 unranked, level of every genome): genome g's largest register is its level.  Every genome above level 3 holds about
    60 % of a shared pool of 48 registers at values uniform in [4, level], so that over the pairs a register is high in both rows (larger
    in either, or equal) or in one.  The even copies of a level have few non-zero registers more than the base and the odd copies many
    (fewer with the level): ranked by cardinality, low levels come before and after high ones."""
    assert n_per_level >= 2
    rng = np.random.default_rng([seed, vmax, n_per_level])
    levels = ladder_levels(vmax)
    n = len(levels) * n_per_level
    rows = _rows(n, rng, 300)
    pool = _pool(48)
    level = np.zeros(n, dtype=np.int64)
    for li, lv in enumerate(levels):
        for c in range(n_per_level):
            g = li * n_per_level + c
            level[g] = lv
            extra = 40 * li + 4 * c if c % 2 == 0 else 1500 - 40 * li - 4 * c
            zeros = np.setdiff1d(np.nonzero(rows[g] == 0)[0], pool)
            rows[g, rng.choice(zeros, extra, replace=False)] = 1
            if lv > 3:
                take = pool[1:][rng.random(pool.size - 1) < 0.6]
                rows[g, take] = rng.integers(4, lv + 1, take.size)
                rows[g, pool[0]] = lv
    return rows.astype(np.uint8), level


def flat_rows(values=FLAT_VALUES):
    return np.repeat(np.asarray(values, dtype=np.uint8)[:, None], 16384, axis=1)


def top_row(seed=0):
    """a base-like genome that holds every value 52..63 (registers above 51: six planes, the last group of the last walk)"""
    rng = np.random.default_rng([seed, 63])
    row = _rows(1, rng, 300)[0]
    sel = rng.choice(16384, 36, replace=False)
    row[sel] = np.tile(np.arange(52, 64), 3)
    return row.astype(np.uint8)


def aux_equal(n, m=M_AUX):
    """SuperMinHash sketches that are all equal: every pair passes every band and reaches stage 2"""
    return np.tile(np.arange(m, dtype=np.uint64), (n, 1))


def aux_hll_rows(n, seed=0, p_aux=8):
    """auxiliary HLL sketches of similar genomes of about 20 000 elements: shared registers, a few redrawn per genome"""
    rng = np.random.default_rng([seed, p_aux])
    size = 1 << p_aux
    shift = max(0, 14 - p_aux)
    base = np.minimum(np.random.default_rng(_BASE_SEED + 2).geometric(0.5, size) + shift, 64 - p_aux + 1)
    rows = np.tile(base, (n, 1))
    for g in range(n):
        sel = rng.choice(size, max(1, size // 40), replace=False)
        rows[g, sel] = np.minimum(rng.geometric(0.5, sel.size) + shift, 64 - p_aux + 1)
    return rows.astype(np.uint8)


def query_case(oracle, vmax_q, vmax_d):
    """a query set and a database from ladder sets of their own, each ranked on its own: (hll, aux, cards, level, aux_hll) twice"""
    sides = []
    for vmax, seed in ((vmax_q, 11), (vmax_d, 12)):
        rows, level = ladder_set(vmax, 2, seed=seed)
        hll, cards, _, level, ah = rank_set(oracle, rows, level, aux_hll_rows(rows.shape[0], seed=seed))
        sides.append((hll, aux_equal(hll.shape[0]), cards, level, ah))
    return sides[0], sides[1]


def rank_set(oracle, hll, *more):
    """(hll, cards, perm, *more) in the rank order of the oracle's cardinalities"""
    from cuda_selection_criteria_amd import sort_by_card
    cards = oracle.cards(hll)
    perm = sort_by_card(cards)
    return (hll[perm], cards[perm], perm) + tuple(x[perm] for x in more)
