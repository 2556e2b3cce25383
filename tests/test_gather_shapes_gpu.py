"""The screen's mask stage at m = 32, 64 (narrow kernel) and m = 2048, 3072, 4096 (wide kernel) against tests/gather_model.py, bit for
bit, through both entries; the context entry under "gather_generic" = 0 and = 1, "gather_mask_kernel_used" naming the kernel that ran."""
import numpy as np
import pytest

import gather_model as GM
from test_gather_gpu import forge, raw, same, segments, via_context

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import Selector

pytestmark = pytest.mark.gpu

E = GM.EMPTY
NARROW, WIDE = (32, 64), (2048, 3072, 4096)


def both_routes(Q, D, cases, wants):
    """one context, every (c_min, max_picks) of `cases` under the kernel of m and under the generic one"""
    kind = 2 if Q.shape[1] in NARROW else 3
    with Selector(0) as sel:
        sel.upload(np.zeros((len(D), 1 << 14), np.uint8), D, np.zeros(len(D)))
        sel.upload_queries(np.zeros((len(Q), 1 << 14), np.uint8), Q, np.zeros(len(Q)))
        assert sel.get_param("gather_mask_kernel_used") == -1 and sel.get_param("gather_generic") == 0
        for generic, used in ((0, kind), (1, 0)):
            sel.set_param("gather_generic", generic)
            for (c_min, max_picks), want in zip(cases, wants):
                res = sel.gather(c_min, max_picks)
                assert sel.get_param("gather_mask_kernel_used") == used
                same((res["picks"], res["n_picks"], res["unexplained"]), want, ("context", generic, c_min, max_picks))
        with pytest.raises(pkg.SelhipError, match="gather_generic"):
            sel.set_param("gather_generic", 2)


# (1, 1) a single pair; (2, 3) a partial load of one and of three rows at G = 4; (13, 65) one row past a narrow wave's rows and a wide
# tile, one column past a span; (49, 130) one row past a narrow tile, three spans; (4, 63) one row past a wide wave's rows
@pytest.mark.parametrize("m, n_q, n_d", [(m, q, d) for m in NARROW + WIDE for q, d in ((1, 1), (2, 3), (13, 65), (49, 130), (4, 63)) if m in WIDE or q != 4])
def test_shapes_against_the_model(m, n_q, n_d):
    Q, D = forge(n_q, n_d, m, seed=m + n_q + n_d)
    cases = ((1, 64), (3, 64), (16, 2))
    wants = [GM.gather(Q, D, *c) for c in cases]
    for c, want in zip(cases, wants):
        same(raw(Q, D, *c), want, ("context-free", c))
    both_routes(Q, D, cases, wants)


@pytest.mark.parametrize("m", (32, 64, 2048, 3072))
def test_planted_rows(m):
    """every count known by construction.  Query 0: row 0 shares bucket 1 (the first .y), row 1 bucket m - 2 (the last .x), row 4 the
    last bucket and row 5 the first (neighbours in one wave load: a bit leaking across a ballot field would show), row 6 the last
    bucket of a chunk (of the .x/.y halves of a narrow row) and the first of the next, rows 7 and 8 differ from the query in the high
    and in the low dword only.  Query 1 leaves 3 buckets unfilled; rows 9 and 10 leave them unfilled too and share 2 and 3 filled
    ones: at c_min = 3 both raw counts pass, only row 10's masked one does.  Row 11 is a whole copy of query 2"""
    rng = np.random.default_rng(m)
    Q = rng.integers(1, 1 << 62, (3, m)).astype(np.uint64)
    D = rng.integers(1, 1 << 62, (12, m)).astype(np.uint64)
    b = min(1024, m // 2)
    for d, at in ((0, [1]), (1, [m - 2]), (4, [m - 1]), (5, [0]), (6, [b - 1, b])):
        D[d, at] = Q[0, at]
    D[7], D[8] = Q[0] ^ np.uint64(1 << 40), Q[0] ^ np.uint64(1)
    holes = [5, 6, m - 3]
    Q[1, holes] = E
    for d, at in ((9, [8, 9]), (10, [8, 9, 10])):
        D[d, holes] = E
        D[d, at] = Q[1, at]
    D[11] = Q[2]
    cases = ((1, 64), (3, 64), (m, 64))
    wants = [GM.gather(Q, D, *c) for c in cases]
    assert [tuple(p) for p in wants[0][0].tolist()] == [(0, 6, 2, 2), (0, 0, 1, 1), (0, 1, 1, 1), (0, 4, 1, 1), (0, 5, 1, 1), (1, 10, 3, 3), (2, 11, m, m)]
    assert [tuple(p) for p in wants[1][0].tolist()] == [(1, 10, 3, 3), (2, 11, m, m)] and wants[1][2].tolist() == [m, m - 6, 0]
    assert [tuple(p) for p in wants[2][0].tolist()] == [(2, 11, m, m)]
    for c, want in zip(cases, wants):
        same(raw(Q, D, *c), want, ("context-free", c))
    both_routes(Q, D, cases, wants)


# W = 1, 2 and 96 on the staged and the streamed route.  (segments() asks for 40 distinct buckets, more than a row of 32 has: there the
# long segments are those of 4 mixtures over 700 strains of 5 sources)
@pytest.mark.parametrize("lds_cap", (0, 8))
@pytest.mark.parametrize("m", (32, 64, 3072))
def test_pick_stage_at_the_new_word_counts(m, lds_cap):
    if m == 32:
        Q, D = forge(4, 700, 32, seed=32)
        want, want6 = GM.gather(Q, D, 1, 64), GM.gather(Q, D, 6, 300)
        assert want[1].max() > 1 and want6[1].max() > 1
    else:
        Q, D, want, want6 = segments(m)
    same(via_context(Q, D, 1, 64, lds_cap), want, "c_min 1")
    same(via_context(Q, D, 6, 300, lds_cap), want6, "c_min 6")
    same(raw(Q, D, 6, 300), want6, "context-free")


@pytest.mark.parametrize("m", (64, 2048))
def test_rows_off_the_16_byte_grid_take_the_generic_kernel(m):
    Q, D = forge(13, 65, m, seed=m)
    same(raw(Q, D, 1, 64, shift=1), GM.gather(Q, D, 1, 64), "unaligned")
