"""The forged sets of tests/bitplane_model.py are what tests/test_bitplane_instantiations_gpu.py needs them to be: conditions on the
inputs, read from the oracle and the numpy model alone.  Every grid cell has the intended largest register, plane count and sparse
threshold, and all its pairs reach the Jaccard test; every ladder set and every query / database split holds a pair in each cell of
(walks taken) x (which row holds the larger maximum) that its levels allow, with union mass in every value interval a walk decodes.
No GPU."""
import numpy as np
import pytest

import bitplane_model as B
import cuda_selection_criteria_amd as pkg

NB_OF = {15: 4, 31: 5, 51: 6}
# (vmax, genomes per level, pairs the case needs): the query sides, the pair-list and count sets, the one-launch small pass's sets
LADDER_CASES = ([(v, 2, 1) for v in (15, 31, 51)] + [(v, B.ladder_per(v), 60) for v in (15, 31, 51)]
                + [(v, B.per_level_for(v, 130), 130) for v in (15, 23, 24, 31, 32)])


@pytest.mark.parametrize("vmax,t", B.GRID_ON + B.GRID_OFF)
def test_grid_cell_is_the_intended_one(oracle, vmax, t):
    rows = B.grid_set(vmax, t)
    n = rows.shape[0]
    assert n <= 64
    k = B.khi(rows)
    assert k == vmax + 1 and B.planes(k) == NB_OF[vmax]
    assert B.sparse_t(rows, k) == (t if (vmax, t) in B.GRID_ON else 0)
    if t > 4:                                                # the threshold sits on the cap: 129 registers at t - 4 or more in one genome
        assert int((rows >= t - 4).sum(axis=1).max()) > B.CAP >= int((rows >= t).sum(axis=1).max())
    hll, cards, _ = B.rank_set(oracle, rows)
    assert np.all(np.isfinite(cards)) and np.all(cards > 0)
    r, b = pkg.banding(B.M_AUX, 0.5)
    pairs, st = oracle.select(hll, B.aux_equal(n), cards, -1.0, r, b, use_cb=False)
    assert st["evaluated"] == st["survivors"] == len(pairs) == n * (n - 1) // 2
    # every group of four values below the threshold (what the sparse kernel decodes from the planes) holds registers in most genomes,
    # with different counts in different genomes: no input of bs_reduce16<2 G1> is zero throughout
    for g4 in range(1, min(t, vmax + 1) // 4):
        cnt = ((rows >= 4 * g4) & (rows < 4 * g4 + 4)).sum(axis=1)
        assert np.count_nonzero(cnt) > n // 2 and len(set(cnt.tolist())) > 2, (vmax, t, g4)
    # the shared registers: over the pairs a register is high in both rows with either the larger, or equal, and high in one row only
    hi = min(t, vmax - 3)
    kinds = set()
    rng = np.random.default_rng(vmax * 100 + t)
    for x, y in rng.integers(0, n, (60, 2)):
        a, c = hll[x].astype(int), hll[y].astype(int)
        assert np.array_equal(B.union_hist(hll[x], hll[y]), oracle.union_hist(hll[x], hll[y]))
        if x != y:
            both = (a >= hi) & (c >= hi)
            kinds |= {("gt", bool(np.any(both & (a > c)))), ("lt", bool(np.any(both & (a < c)))), ("eq", bool(np.any(both & (a == c)))),
                      ("one", bool(np.any((a >= hi) != (c >= hi))))}
    assert {("gt", True), ("lt", True), ("eq", True), ("one", True)} <= kinds


def all_pairs_cells(level):
    x, y = np.triu_indices(len(level), 1)
    return B.walk_cells(level[x], level[y]), x, y


def interval_mass(hll, x, y):
    mass = np.zeros(64, dtype=np.int64)
    for a, c in zip(x.tolist(), y.tolist()):
        mass += B.union_hist(hll[a], hll[c])
    return mass


def assert_intervals(mass, vmax):
    for lo, hi in ((24, 32), (32, 48), (48, 52)):
        if vmax >= lo:
            assert mass[lo:hi].sum() > 0, (vmax, lo)
    assert mass[vmax + 1:].sum() == 0 and mass[vmax] > 0


@pytest.mark.parametrize("vmax,per,min_pairs", sorted(set(LADDER_CASES)))
def test_ladder_set_reaches_every_walk_cell(oracle, vmax, per, min_pairs):
    rows, level = B.ladder_set(vmax, per)
    n = rows.shape[0]
    assert n <= 64 and np.array_equal(rows.max(axis=1), level) and B.khi(rows) == vmax + 1
    assert all(int((level == lv).sum()) == per >= 2 for lv in B.ladder_levels(vmax))
    hll, cards, _, level = B.rank_set(oracle, rows, level)
    assert np.all(np.isfinite(cards)) and np.all(cards > 0)
    cells, x, y = all_pairs_cells(level)
    assert cells == B.walk_cells_allowed(B.ladder_levels(vmax), B.ladder_levels(vmax), True), (vmax, per, sorted(cells))
    if vmax == 51:
        assert len(cells) == 12                                  # every kp class with the maximum in the first row, the second and both
    assert_intervals(interval_mass(hll, x, y), vmax)
    r, b = pkg.banding(B.M_AUX, 0.5)
    pairs, st = oracle.select(hll, B.aux_equal(n), cards, -1.0, r, b, use_cb=False)
    assert st["evaluated"] == st["survivors"] == len(pairs) == n * (n - 1) // 2
    assert len(pairs) >= min_pairs
    # a shared register high in both rows with a > b, a < b, a = b, and in one row only
    a, c = hll[x].astype(int), hll[y].astype(int)
    both = (a >= 4) & (c >= 4)
    assert np.any(both & (a > c)) and np.any(both & (a < c)) and np.any(both & (a == c)) and np.any((a >= 4) != (c >= 4))
    for j in np.random.default_rng(vmax).integers(0, len(x), 20):
        assert np.array_equal(B.union_hist(hll[x[j]], hll[y[j]]), oracle.union_hist(hll[x[j]], hll[y[j]]))


def test_small_pass_sets_change_kp_class_between_a_waves_pairs(oracle):
    """a wave of the one-launch pass takes pairs p, p + 4, ... of a row and prefetches the next one's kp: in the sets whose registers
    reach 24 (kp = 25 takes the walk) a row's pairs p and p + 4 lie on both sides of it, in both orders.  (With khi <= 24 no pair
    takes a walk, whatever kp is.)"""
    for vmax in (24, 31):
        rows, level = B.ladder_set(vmax, B.per_level_for(vmax, 130))
        _, _, _, level = B.rank_set(oracle, rows, level)
        assert {(0, 1), (1, 0), (0, 0), (1, 1)} <= B.prefetch_steps(level), vmax
    rows, level = B.ladder_set(23, B.per_level_for(23, 130))
    assert B.prefetch_steps(level) == {(0, 0)}


@pytest.mark.parametrize("vmax_q", [15, 31, 51])
@pytest.mark.parametrize("vmax_d", [15, 31, 51])
def test_query_split_reaches_every_walk_cell(oracle, vmax_q, vmax_d):
    Q, D = B.query_case(oracle, vmax_q, vmax_d)
    assert B.khi(Q[0]) == vmax_q + 1 and B.khi(D[0]) == vmax_d + 1
    assert np.array_equal(Q[0].max(axis=1), Q[3]) and np.array_equal(D[0].max(axis=1), D[3])
    for side in (Q, D):
        assert np.all(np.isfinite(side[2])) and np.all(side[2] > 0) and np.all(np.diff(side[2]) >= 0)
    x, y = np.divmod(np.arange(len(Q[3]) * len(D[3])), len(D[3]))
    cells = B.walk_cells(Q[3][x], D[3][y])
    assert cells == B.walk_cells_allowed(B.ladder_levels(vmax_q), B.ladder_levels(vmax_d), False)
    if vmax_q == vmax_d == 51:
        assert len(cells) == 12
    if vmax_q != vmax_d:
        # the larger maximum on one side only: a kernel that read one set's maxima for both rows would decode too few values
        top = (0 if vmax_q > vmax_d else 1)
        assert (B.kp_class(max(vmax_q, vmax_d) + 1), top) in cells and (B.kp_class(max(vmax_q, vmax_d) + 1), 1 - top) not in cells
    mass = np.zeros(64, dtype=np.int64)
    for a, c in zip(x.tolist(), y.tolist()):
        mass += B.union_hist(Q[0][a], D[0][c])
    assert_intervals(mass, max(vmax_q, vmax_d))
    # ranks differ between the sets: the same rank holds different maxima in Q and in D somewhere
    k = min(len(Q[3]), len(D[3]))
    assert np.any(Q[3][:k] != D[3][:k]) or vmax_q == vmax_d == 15


def test_flat_rows_take_every_count_formula(oracle):
    flat = B.flat_rows()
    assert sorted(int(v) % 4 for v in B.FLAT_VALUES) == [0, 1, 2, 3] and min(B.FLAT_VALUES) >= 24
    assert {B.kp_class(v + 1) for v in B.FLAT_VALUES} == {1, 2, 3}
    for i, v in enumerate(B.FLAT_VALUES):
        for j, w in enumerate(B.FLAT_VALUES):
            want = np.zeros(64, dtype=np.uint32)
            want[max(v, w)] = 16384
            assert np.array_equal(B.union_hist(flat[i], flat[j]), want) and np.array_equal(oracle.union_hist(flat[i], flat[j]), want)
    top = B.top_row()
    assert set(range(52, 64)) <= set(top.tolist()) and B.khi(top[None]) == 64 and B.planes(64) == 6


def test_model_rules():
    assert [B.planes(k) for k in (1, 16, 17, 32, 33, 64)] == [4, 4, 5, 5, 6, 6]
    assert [B.kp_class(k) for k in (4, 24, 25, 32, 33, 48, 49, 64)] == [0, 0, 1, 1, 2, 2, 3, 3]
    rows = np.zeros((2, 16384), dtype=np.uint8)
    rows[0, :128] = 30
    assert B.sparse_t(rows, 31) == 4 and B.sparse_t(rows, 4) == 0
    rows[0, 128] = 22
    assert B.sparse_t(rows, 31) == 0 and B.sparse_t(rows, 33) == 24          # T = 24: off with five planes, on with six
    rows[1, :129] = 25
    assert B.sparse_t(rows, 64) == 0                                        # more than 128 registers at 24 or more: no lists
    assert len(B.GRID_ON) == 14 and len({(B.planes(v + 1), t // 4) for v, t in B.GRID_ON}) == 14
