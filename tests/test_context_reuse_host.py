"""The premises of tests/test_context_reuse_gpu.py, pinned without a GPU (tests/context_reuse_model.py).  A
replacement that goes wrong gives the previous set's answer or reads its bytes; the GPU tests see that only if

  * on every step X -> Y the two sets' expected values differ for every operation both admit;
  * the warm-up set BIG holds, under every criterion, records (i, k) with i < 70 <= k < 128: the pairs a join that forgets the pad mask
    adds to PREFIX, whose padded arrays keep BIG's columns 70 .. 127;
  * BIG has at most five bit planes and HIGHREG six, with a sparse threshold;
  * no expected value of a set of two or more genomes is empty."""
import numpy as np
import pytest

import context_reuse_model as R
import stream_harness as H


@pytest.fixture(scope="module")
def lib(oracle):
    return R.Library(oracle)


def test_shapes_are_those_of_the_model_s_docstring(lib):
    shape = lambda S: (S.n_d, S.n_q, S.m, S.p_hll, S.p_aux)          # noqa: E731
    assert shape(lib["BIG"]) == (330, 40, 128, 14, 8) and shape(lib["HIGHREG"]) == (330, 40, 128, 14, 8)
    assert shape(lib["PREFIX"]) == (R.CUT, 40, 128, 14, 8) and (R.CUT, R.PAD) == (70, 128)
    assert shape(lib["NARROW"]) == (200, 40, 64, 14, 6) and shape(lib["WIDE"]) == (130, 40, 512, 14, 8)
    assert shape(lib["LOWP"])[:1] + shape(lib["LOWP"])[2:] == (150, 64, 10, 6)
    assert lib["EMPTY"].n_d == 0 and lib["ONE"].n_d == 1
    for name in R.NAMES:
        S = lib[name]
        assert S.n_d <= 330 and S.D.hll.shape == (S.n_d, 1 << S.p_hll) and S.D.aux.shape == (S.n_d, S.m)
        assert S.D.aux_hll.shape == (S.n_d, 1 << S.p_aux) and (np.diff(S.D.cards) >= 0).all()
    B, P = lib["BIG"], lib["PREFIX"]
    assert np.array_equal(P.D.hll, B.D.hll[:R.CUT]) and np.array_equal(P.D.aux, B.D.aux[:R.CUT]) and P.Q is B.Q
    assert -(-B.n_d // 64) * 64 == 384 and -(-P.n_d // 64) * 64 == R.PAD
    assert {x for t in R.TRANSITIONS for x in t} == set(R.NAMES)


def test_operations_are_the_context_cases():
    assert set(R.OPS) == (set(H.CONTEXT_CASES) - set(R.NOT_HERE)) | {"merge_groups", "cards"}
    assert all(reason for reason in R.NOT_HERE.values())


@pytest.mark.parametrize("step", R.steps(), ids=lambda s: "->".join(s))
def test_every_step_changes_every_answer(lib, step):
    X, Y = lib[step[0]], lib[step[1]]
    for op in R.OPS:
        if R.refusal(X, op) is not None or R.refusal(Y, op) is not None:
            continue
        if (step[0], step[1], op) in R.SAME_ANSWER:
            continue
        assert not H.same(R.expected(X, op), R.expected(Y, op)), f"{op}: {step[0]} and {step[1]} have one answer, the step is blind to it"


NEW_OPS = ("forest",) + tuple(H.LINKAGE_CASES)


def test_the_hierarchy_operations_need_no_exemption(lib):
    """the forest and the three linkages tell every step's two sets apart: none of them stands in SAME_ANSWER, and on every step both
    sets admit they differ (said once more for them alone, beside test_every_step_changes_every_answer)"""
    assert set(NEW_OPS) <= set(R.OPS) and not any(key[2] in NEW_OPS for key in R.SAME_ANSWER)
    assert R.HLL_LINKAGES == {"linkage-average-jaccard", "linkage-complete-max_containment-capped"}
    assert R.HLL_LINKAGES <= R.P14_ONLY and R.HLL_LINKAGES <= R.NEEDS_PLANES
    for x, y in R.steps():
        for op in NEW_OPS:
            if R.refusal(lib[x], op) is None and R.refusal(lib[y], op) is None:
                assert not H.same(R.expected(lib[x], op), R.expected(lib[y], op)), (x, y, op)
    L = lib["LOWP"]
    for op in NEW_OPS:
        assert R.refusal(L, op) == (R.BADARG if op in R.HLL_LINKAGES else None), op
        assert R.refusal(lib["BIG"], op, bit_planes=False) == (R.BADARG if op in R.HLL_LINKAGES else None), op
        assert R.refusal(lib["EMPTY"], op, bit_planes=False) is None
    for name in ("EMPTY", "ONE"):
        n = lib[name].n_d
        for op in R.LINKAGE_OPS:
            want = R.expected(lib[name], op)
            assert len(want["merges"]) == len(want["sizes"]) == 0 and want["rounds"] == n
        want = R.expected(lib[name], "forest")
        assert len(want["edges"]) == 0 and want["labels"].tolist() == list(range(n))
    # the capped case cuts on every set of two or more genomes it runs on
    for name in R.NAMES:
        S = lib[name]
        if not S.trivial and S.p_hll == 14:
            assert 0 < len(S.linkage_complete_max_containment_capped["merges"]) < S.n_d - 1, name


def test_the_image_premises(lib):
    """which sets hold the clamped four-plane image (threshold 4, 8 or 12), and that the steps and sequences are there on which a stale
    image would be read: a step between two sets that are both on the image with other rows at equal ranks, and a sequence on, off, on"""
    on = {name: lib[name].hist_image({}) for name in R.NAMES}
    assert on == {"BIG": 1, "PREFIX": 1, "NARROW": 1, "WIDE": 1, "LOWP": 0, "HIGHREG": 0, "EMPTY": 0, "ONE": 1, "TRIMMED": 1}, on
    B = lib["BIG"]
    for knob in ("hist_image", "hist_sparse", "hist_algo"):
        assert B.hist_image({knob: 0}) == 0 and B.hist_image({knob: 1}) == 1 and B.hist_image({knob: -1}) == 1
    other_rows = []
    for x, y in R.steps():
        X, Y = lib[x], lib[y]
        k = min(X.n_d, Y.n_d)
        if on[x] and on[y] and k >= 2 and (X.D.hll[:k] != Y.D.hll[:k]).any(axis=1).all():
            other_rows.append((x, y))
    assert ("BIG", "NARROW") in other_rows and ("NARROW", "WIDE") in other_rows and ("BIG", "PREFIX") not in other_rows, other_rows
    assert any(tuple(on[s] for s in t[j:j + 3]) == (1, 0, 1) for t in R.TRANSITIONS for j in range(len(t) - 2)), "no sequence on, off, on"
    assert ("BIG", "HIGHREG", "BIG") in R.TRANSITIONS


def test_exemptions_are_few():
    for key, reason in R.SAME_ANSWER.items():
        assert reason and (key[0], key[1]) in R.steps() and key[2] in R.OPS
    for op in R.OPS:
        assert sum(1 for key in R.SAME_ANSWER if key[2] == op) <= 2, op


@pytest.mark.parametrize("attr", ["smh_a", "hll_a", "hll_a_folded", "two_stage", "none", "smh_c", "smh_c_v"])
def test_big_holds_partners_in_the_prefix_s_padding(lib, attr):
    rec = R.pad_partners(getattr(lib["BIG"], attr))
    assert len(rec) >= 5, f"{attr}: {len(rec)} records of BIG with i < {R.CUT} <= k < {R.PAD}"
    # the cut splits a cluster: the genome in the first pad column is a partner of a live row (all a mask that is off by one admits)
    assert (rec["k"] == R.CUT).any(), attr
    # ... and the prefix set's own answer is BIG's cut to the rows and columns below the cut: nothing else tells them apart
    big = getattr(lib["BIG"], attr)
    assert H.same(big[big["k"] < R.CUT], getattr(lib["PREFIX"], attr))


@pytest.mark.parametrize("attr", ["smh_a", "hll_a", "two_stage", "none", "smh_c", "smh_c_v"])
def test_big_holds_partners_in_the_trimmed_set_s_first_pad_column(lib, attr):
    """TRIMMED pads to BIG's 384 columns, so the band-major signature arrays keep their stride and column TRIM of every band is still
    genome TRIM of BIG after BIG -> TRIMMED (behind BIG -> PREFIX the stride changes and the pad columns hold other bands' bytes)"""
    B, T = lib["BIG"], lib["TRIMMED"]
    assert -(-T.n_d // 64) * 64 == -(-B.n_d // 64) * 64 == 384 and T.n_d == R.TRIM
    big = getattr(B, attr)
    assert ((big["k"] == R.TRIM) & (big["i"] < R.TRIM)).sum() >= 5, attr
    assert H.same(big[big["k"] < R.TRIM], getattr(T, attr))


def test_plane_counts_and_sparse_thresholds(lib):
    assert (lib["BIG"].planes, lib["BIG"].sparse_t) == (5, 12) and (lib["PREFIX"].planes, lib["PREFIX"].sparse_t) == (5, 8)
    assert (lib["HIGHREG"].planes, lib["HIGHREG"].sparse_t) == (6, 16)
    # the records a missing or shifted pad mask would add: 43 in PREFIX's padding, 5 of them in its first pad column, 8 in TRIMMED's
    big = lib["BIG"].smh_a
    assert len(R.pad_partners(big)) == 43 and ((big["k"] == R.CUT) & (big["i"] < R.CUT)).sum() == 5
    assert ((big["k"] == R.TRIM) & (big["i"] < R.TRIM)).sum() == 8
    assert lib["LOWP"].planes == 0


@pytest.mark.parametrize("name", [n for n in R.NAMES if n not in ("EMPTY", "ONE")])
def test_no_expected_value_is_empty(lib, name):
    S = lib[name]
    assert not S.trivial
    for op, (_, kind) in R.OPS.items():
        want = R.expected(S, op)
        if R.refusal(S, op) is not None:
            assert want == R.BADARG and S.p_hll != 14
            continue
        for leaf in R.leaves(want):
            assert leaf.size > 0, op
        if kind in ("list", "qlist"):
            assert len(want) >= 10, (op, len(want))
    assert len(S.topk) < 2 * len(S.smh_a) and len(S.smh_c) < len(S.none)
    st = R.stats_expected(S)
    assert st["evaluated"] > st["candidates"] >= st["survivors"] >= st["selected"] > 0


def test_trivial_sets_have_values_too(lib):
    for name in ("EMPTY", "ONE"):
        S = lib[name]
        for op, (_, kind) in R.OPS.items():
            want = R.expected(S, op)
            if kind == "list":
                assert len(want) == 0
        assert not any(R.stats_expected(S).values())
