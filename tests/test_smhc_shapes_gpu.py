"""The narrow (m = 32, 64) and the wide (m = 2048 .. 8192 in steps of 1024) kernel of criterion smh_c's count pass (kernel_smhc.cuh, DESIGN.md
section 37).  Every case runs the pass under the estimator smh, where the count itself is the record: the expected records {i, k, c / m}
and statistics come from the numpy counts of smh_matrix_model.py through smhv_model.py, compared with ==; the same call under
"smhc_generic" = 1 must give the same; "smhc_kernel_used" must name the kernel that ran and "smhc_path_used" stay 0."""
import functools

import numpy as np
import pytest

import smh_matrix_model as model
import smhc_model as M
import smhcc_model as CC
import smhv_model as V

from cuda_selection_criteria_amd import CRIT_SMH_C, MODE_SMH, SelhipError, Selector

pytestmark = pytest.mark.gpu

KIND = {32: 2, 64: 2, 2048: 3, 3072: 3}                       # "smhc_kernel_used": 2 narrow (both G), 3 wide (an even and an odd chunk count)
ALL_N = (2, 5, 13, 49, 66, 130, 1030)
QUERY_SHAPES = ((1, 1), (5, 63), (13, 65), (49, 200), (3, 1030))
TAU = 0.3


def zeros_hll(n):
    return np.zeros((n, 1 << 14), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def case(m, n_q, n_d):
    """(Q rows, Q cards, D rows, D cards, counts[Q, D]); n_q = 0: the all-pairs case, Q = D"""
    rows = model.random_rows(n_q + n_d, m, seed=31 * m + n_d)
    D, d_cards = rows[n_q:], V.spread_cards(n_d)
    Q, q_cards = (rows[:n_q], V.spread_cards(n_q)) if n_q else (D, d_cards)
    return Q, q_cards, D, d_cards, model.match_counts(Q, D)


def configure(sel, c_min=1, gamma=None, measure="jaccard", estimator="smh"):
    sel.set_criterion(CRIT_SMH_C)
    sel.set_min_matches(c_min)
    sel.set_min_containment(gamma)
    sel.set_measure(measure)
    sel.set_estimator(estimator)


def both_routes(sel, m, run, what):
    """(records, statistics) of run() on the kernel of m, which the generic kernel must repeat"""
    out = []
    for generic, kind in ((0, KIND[m]), (1, 0)):
        sel.set_param("smhc_generic", generic)
        got, st = run(), sel.stats()
        sel.set_param("smhc_generic", 0)
        assert sel.get_param("smhc_kernel_used") == kind and sel.get_param("smhc_path_used") == 0, (what, generic)
        out.append((M.tuples(got), st))
    assert out[0] == out[1], (what, "generic against new")
    return out[0]


def check(sel, m, run, want, what):
    rec, wst = want
    assert both_routes(sel, m, run, what) == (M.tuples(rec), wst), what


@pytest.mark.parametrize("n", ALL_N)
@pytest.mark.parametrize("m", sorted(KIND))
def test_all_pairs(m, n):
    aux, cards, _, _, counts = case(m, 0, n)
    with Selector(0) as sel:
        sel.upload(zeros_hll(n), aux, cards)
        configure(sel, c_min=m // 4)
        want = V.expected(aux, cards, TAU, c_min=m // 4, counts=counts)
        check(sel, m, lambda: sel.run(TAU, MODE_SMH, 7, 3), want, (m, n))
        if n >= 49:
            assert 0 < want[1]["selected"] < want[1]["survivors"] < want[1]["evaluated"]


@pytest.mark.parametrize("shape", QUERY_SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("m", sorted(KIND))
def test_query(m, shape):
    Q, q_cards, D, d_cards, _ = case(m, *shape)
    with Selector(0) as sel:
        sel.upload(zeros_hll(shape[1]), D, d_cards)
        sel.upload_queries(zeros_hll(shape[0]), Q, q_cards)
        configure(sel, c_min=m // 4)
        check(sel, m, lambda: sel.run_queries(TAU, MODE_SMH, 7, 3), V.expected_cross(Q, q_cards, D, d_cards, TAU, c_min=m // 4), (m, shape))


def planted(m):
    """rows of distinct buckets in which row i + 1 shares with row 0 exactly the buckets plant[i], and the plant"""
    plant = [[0], [m - 1], [2], [3], [m - 2], [m - 3], [5]]    # one bucket: the first, the last, the .x and .y halves of a 16-byte load
    # neighbouring rows of one wave load of the narrow kernel: the last bucket of one lane group, the first bucket of the next
    plant += [[m - 1], [0], [m - 1], [0], [m - 1], [0], [0, m - 1]]
    if m >= 2048:                                              # wide: the last bucket of a 1024-bucket chunk and the first of the next
        plant += [[1023], [1024], [m - 1025], [m - 1024], [1023, 1024]]
    plant += [list(range(m)), [], []]
    idx = np.arange((len(plant) + 1) * m, dtype=np.uint64).reshape(-1, m) + np.uint64(1)
    rows = (idx << np.uint64(32)) | (idx * np.uint64(2654435761) & np.uint64(0xFFFFFFFF))       # all distinct, in both dwords
    for i, buckets in enumerate(plant):
        rows[i + 1, buckets] = rows[0, buckets]
    rows[-2] = rows[0] ^ np.uint64(1 << 32)                     # differs from the base in the high dword only ...
    rows[-1] = rows[0] ^ np.uint64(1)                           # ... and in the low dword only
    return rows, plant


@pytest.mark.parametrize("m", sorted(KIND))
def test_planted_rows(m):
    rows, plant = planted(m)
    n = len(rows)
    cards = V.spread_cards(n)
    counts = model.match_counts(rows, rows)
    assert counts[0, 1:].tolist() == [len(b) for b in plant]
    with Selector(0) as sel:
        sel.upload(zeros_hll(n), rows, cards)
        sel.upload_queries(zeros_hll(2), rows[:2], cards[:2])
        for c_min in (1, 2, 3, m):                              # the planted counts 1 and 2, each of them + 1, and m
            configure(sel, c_min=c_min)
            want = V.expected(rows, cards, 0.0, c_min=c_min, counts=counts)
            assert [int(k) for i, k in zip(want[0]["i"], want[0]["k"]) if i == 0] == [k + 1 for k, b in enumerate(plant) if len(b) >= c_min]
            check(sel, m, lambda: sel.run(0.0, MODE_SMH, 7, 3), want, (m, c_min))
            check(sel, m, lambda: sel.run_queries(0.0, MODE_SMH, 7, 3), V.expected_cross(rows[:2], cards[:2], rows, cards, 0.0, c_min=c_min), (m, c_min, "query"))


@pytest.mark.parametrize("m", sorted(KIND))
def test_windows(m):
    """a row range with candidate_begin set, and genomes of cardinality 0 at the front (z0 = 5)"""
    n = 130
    aux, cards, _, _, counts = case(m, 0, n)
    with Selector(0) as sel:
        sel.upload(zeros_hll(n), aux, cards)
        configure(sel, c_min=m // 4)
        sel.set_candidate_begin(70)
        check(sel, m, lambda: sel.run(TAU, MODE_SMH, 7, 3, rows=(7, 77)), V.expected(aux, cards, TAU, c_min=m // 4, rows=(7, 77), cand_begin=70, counts=counts), (m, "range"))
        zero = cards.copy()
        zero[:5] = 0.0
        sel.upload(zeros_hll(n), aux, zero)
        configure(sel, c_min=m // 4)
        check(sel, m, lambda: sel.run(TAU, MODE_SMH, 7, 3), V.expected(aux, zero, TAU, c_min=m // 4, counts=counts), (m, "z0"))


@pytest.mark.parametrize("m", sorted(KIND))
def test_containment_rule(m):
    """the per-pair threshold of smhcc_model.py, with the maximum containment as the record"""
    aux, cards, _, _, counts = case(m, 0, 130)
    Q, q_cards, D, d_cards, _ = case(m, 13, 65)
    with Selector(0) as sel:
        sel.upload(zeros_hll(130), aux, cards)
        configure(sel, gamma=CC.G08, measure="max_containment")
        want = V.expected(aux, cards, 0.5, measure="max_containment", c_min=1, gamma=CC.G08, counts=counts)
        assert 0 < want[1]["selected"] <= want[1]["survivors"] < want[1]["evaluated"]
        check(sel, m, lambda: sel.run(0.5, MODE_SMH, 7, 3), want, (m, "all"))
        sel.upload(zeros_hll(65), D, d_cards)
        sel.upload_queries(zeros_hll(13), Q, q_cards)
        configure(sel, gamma=CC.G08, measure="max_containment")
        check(sel, m, lambda: sel.run_queries(0.5, MODE_SMH, 7, 3), V.expected_cross(Q, q_cards, D, d_cards, 0.5, measure="max_containment", c_min=1, gamma=CC.G08), (m, "query"))


@pytest.mark.parametrize("m", sorted(KIND))
def test_hll_estimator(oracle, m):
    """the survivor-list form (stage 2 on real HLL rows): the kernel of m against the generic kernel on the same context"""
    n = 130
    hll, aux, cards = M.ranked(oracle, M.hll_pool(n), case(m, 0, n)[0])
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        sel.upload_queries(hll[:13], aux[:13], cards[:13])
        configure(sel, c_min=m // 4, estimator="hll")
        rec, st = both_routes(sel, m, lambda: sel.run(0.0, MODE_SMH, 7, 3), (m, "all"))
        assert st["survivors"] == int(np.triu(model.match_counts(aux, aux) >= m // 4, 1).sum()) >= len(rec) > 0
        rec, st = both_routes(sel, m, lambda: sel.run_queries(0.0, MODE_SMH, 7, 3), (m, "query"))
        assert st["survivors"] == int((model.match_counts(aux[:13], aux) >= m // 4).sum()) >= len(rec) > 0


def test_generic_hook_takes_0_or_1():
    with Selector(0) as sel:
        assert sel.get_param("smhc_kernel_used") == -1 and sel.get_param("smhc_generic") == 0
        with pytest.raises(SelhipError):
            sel.set_param("smhc_generic", 2)
