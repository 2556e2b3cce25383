"""The premises of tests/test_streams_gpu.py, pinned without a GPU: every case there tells a wrong stream from a right one only because
the REAL and the DECOY set (tests/stream_harness.py) have different, non-trivial answers.  For every case id: the expected value of
both sets is non-empty -- a record list holds at least 20 records -- and the two differ -- matrices in more than half their cells."""
import numpy as np
import pytest

import stream_harness as H


@pytest.fixture(scope="module")
def sets(oracle):
    return {name: H.Sets(oracle, name) for name in ("real", "decoy")}


def leaves(value):
    """the arrays of an expected value"""
    if isinstance(value, dict):
        return [np.asarray(v) for _, v in sorted(value.items())]
    return [np.asarray(value)]


def test_shapes_are_the_issue_s(sets):
    for S in sets.values():
        assert S.D.hll.shape == (H.N_D, 1 << 14) and S.D.aux.shape == (H.N_D, H.M) and S.D.aux_hll.shape == (H.N_D, 1 << H.P_AUX)
        assert S.Q.hll.shape == (H.N_Q, 1 << 14) and S.Q.aux.shape == (H.N_Q, H.M)
        assert (np.diff(S.D.cards) >= 0).all() and (np.diff(S.Q.cards) >= 0).all() and S.D.cards[0] > 0 and S.Q.cards[0] > 0
    assert (H.N_D, H.N_Q, H.M, H.TAU, H.P_AUX, H.K) == (300, 40, 128, 0.5, 8, 3)
    assert H.banding() == tuple(sets["real"].oracle.banding(H.M, H.TAU))
    assert H.RUN_A_ONLY <= set(H.CASES)


@pytest.mark.parametrize("case_id", sorted(H.CASES))
def test_real_and_decoy_answers_differ(sets, case_id):
    kind = H.CASES[case_id][1]
    real, decoy = H.expected(sets["real"], case_id), H.expected(sets["decoy"], case_id)
    for value in (real, decoy):
        for leaf in leaves(value):
            assert leaf.size > 0
    if kind == "list":
        assert len(real) >= 20 and len(decoy) >= 20, (len(real), len(decoy))
    if kind == "matrix":
        differ = np.ascontiguousarray(real).view(np.uint64) != np.ascontiguousarray(decoy).view(np.uint64)
        assert real.shape == decoy.shape and differ.mean() > 0.5, differ.mean()
    assert not H.same(real, decoy)


def test_late_inputs_differ(sets):
    """what is written behind run A's second delay differs between the sets too, and the pair lists are valid"""
    a, b = sets["real"], sets["decoy"]
    for name in ("pair_list", "prio", "row_pos", "col_pos", "block_pairs", "edges", "keys", "perm", "forest_values", "linkage_dist"):
        assert not np.array_equal(getattr(a, name), getattr(b, name)), name
    for S in (a, b):
        for p in (S.pair_list, S.block_pairs, S.edges):
            assert p.dtype == np.int32 and p.min() >= 0 and p.max() < H.N_D
        assert (S.pair_list[:, 0] != S.pair_list[:, 1]).all() and len(S.pair_list) == H.N_LIST
        assert sorted(S.row_pos) == list(range(H.N_Q)) and sorted(S.col_pos) == list(range(H.N_D))
        # the smh_c cut is a proper, non-empty part of the exhaustive result, and the estimator's list another one
        assert 20 <= len(S.smh_c) < len(S.none) and 20 <= len(S.smh_c_v)
        # the cuts keep fewer records than the directed lists hold: the top-k really cuts
        assert len(S.topk) < 2 * len(S.smh_a) and len(S.query_topk) < len(S.query)


def test_hierarchy_premises(sets):
    """the capped linkage case really cuts (0 < F < n - 1, at the median height of the whole tree), the SuperMinHash case ends in a
    plateau of equal distances (one pair per round: as many rounds as genomes), the forest is a proper one (0 < F < n - 1: several
    components of several genomes), selhip_linkage's matrix has the harness's size and both layouts are there"""
    assert H.ANSWER_UNDER_BLOCKED_NULL <= H.RUN_A_ONLY and set(H.LINKAGE_CASES) <= set(H.CONTEXT_CASES)
    assert H.LINKAGE_LAYOUTS == {"wide": (0, 0), "narrow": (3, 1)} and (H.N_D + 3) % 2 == 1 and H.N_D % 2 == 0
    for S in sets.values():
        n = S.n_d
        whole, capped = S.linkage_complete_max_containment, S.linkage_complete_max_containment_capped
        assert len(whole["merges"]) == n - 1 and 0 < len(capped["merges"]) < n - 1
        assert np.isfinite(S.linkage_cap) and (capped["merges"]["jaccard"] <= S.linkage_cap).all()
        assert np.sort(whole["merges"]["jaccard"])[(n - 1) // 2] == S.linkage_cap
        for name in ("linkage_average_jaccard", "linkage_single_smh_jaccard"):
            assert len(getattr(S, name)["merges"]) == len(getattr(S, name)["sizes"]) == n - 1
        assert S.linkage_single_smh_jaccard["rounds"] >= n // 2 > 4 * S.linkage_average_jaccard["rounds"] // 3
        for forest in (S.forest, S.block_forest):
            assert 0 < len(forest["edges"]) < n - 1 and len(forest["labels"]) == n
        assert S.linkage_dist.shape == (H.N_D, H.N_D) and len(S.forest_values) == len(S.edges) == H.N_EDGES
        assert len(S.block_linkage) == 6 and len(S.block_linkage["merges-wide"]) == H.N_D - 1


def test_bits_compare_bit_for_bit():
    nan = np.array([np.nan, 0.0])
    assert H.same(nan, nan.copy()) and not H.same(np.array([0.0]), np.array([-0.0]))
    assert H.same({"a": np.arange(3, dtype=np.int32)}, {"a": np.arange(3, dtype=np.int64)})
    assert not H.same(np.zeros(3), np.zeros(4))
