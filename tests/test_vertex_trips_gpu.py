"""The kernels that take a lane per vertex, row or slot, past their production grid cap.  cluster_vertex_grid(n) is
at most 4 096 blocks of 256 lanes, so a vertex kernel's grid-stride loop comes round a second time only from vertex 1 048 576 on.  Here
n = 4096 * 256 + 4096 + 71 with both grid hooks at 0: the second trip covers 4 167 vertices in 17 blocks, the last block is partial
and its last wave holds 7 lanes.  Only the free-standing entries run, which need no sketches: selhip_components,
selhip_greedy_representatives, selhip_spanning_forest and selhip_merge_sketches, each compared bit for bit with its Python model.

The models are Python loops over n; they run on the COMPACTED graph: the touched vertices relabelled by their rank.  The relabelling is
monotone, so every smallest-member, pair-order and key-tie rule is preserved; an untouched vertex is its own singleton and, for the
greedy call, its own representative.  test_compaction_is_the_model checks that route against the full models on 5 000 vertices."""
import numpy as np
import pytest
import torch

import cluster_model as CM
import forest_model as FM
import greedy_model as GM
import merge_model as MM
from test_cluster_gpu import clique, components_raw, path, sparse_random
from test_forest_gpu import forest_raw
from test_greedy_gpu import greedy_raw
from test_merge_gpu import S, assert_is_model, raw_merge, to_dev

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import Selector

pytestmark = pytest.mark.gpu

CAP = 4096 * 256               # the vertices one trip of the capped grid covers: the second trip begins here
N = CAP + 4096 + 71            # 1 052 743

TAIL_PATH = (CAP + 300, CAP + 1300)                                  # a path of 1 000 vertices
TAIL_CLIQUES = ((CAP + 1400, 5), (CAP + 1450, 17), (CAP + 1500, 40))
STAR_LEAVES = (CAP + 2000, CAP + 2500)                               # the leaves of the star whose centre is N - 1
TWINS = (CAP + 3000, CAP + 3200)                                     # g of the edges {g, g - CAP}: the same block and lane one trip apart
STRADDLE = (1_048_400, 1_048_800)                                    # a path across the boundary
HEAD_POOL, HEAD_EDGES = 8000, 6000                                   # a sparse random graph on 8 000 vertices below 1 000 000


@pytest.fixture(autouse=True)
def hooks_at_zero():
    """the production grids: both hooks are 0 here, and are 0 again afterwards"""
    with Selector(0) as sel:
        assert (sel.get_param("cluster_blocks"), sel.get_param("vertex_blocks")) == (0, 0)
        yield
        assert (sel.get_param("cluster_blocks"), sel.get_param("vertex_blocks")) == (0, 0)


def big_graph():
    rng = np.random.default_rng(1052743)
    pool = np.sort(rng.choice(1_000_000, HEAD_POOL, replace=False))
    parts = [path(TAIL_PATH[1] - TAIL_PATH[0], "shuffled") + TAIL_PATH[0],
             *[clique(lo, lo + k) for lo, k in TAIL_CLIQUES],
             np.stack([np.full(STAR_LEAVES[1] - STAR_LEAVES[0], N - 1), np.arange(*STAR_LEAVES)], axis=1),
             np.stack([np.arange(*TWINS), np.arange(*TWINS) - CAP], axis=1),
             path(STRADDLE[1] - STRADDLE[0] + 1, "descending") + STRADDLE[0],
             pool[rng.integers(0, HEAD_POOL, size=(HEAD_EDGES, 2))]]
    e = np.concatenate(parts)
    dup = e[rng.integers(0, len(e), 200)][:, ::-1]                    # some rows again, reversed, and self-loops on both sides of the boundary
    loops = np.repeat(np.concatenate([rng.integers(CAP, N - 2, 25), pool[:25]]), 2).reshape(-1, 2)
    e = np.concatenate([e, dup, loops])
    return np.ascontiguousarray(e[rng.permutation(len(e))], dtype=np.int64)


EDGES = big_graph()
_MODEL = {}


# ---- the models on the compacted graph -------------------------------------------------------------------------------------------------------
def compact(edges):
    """(the touched vertices ascending, the edge list in their ranks)"""
    touched = np.unique(edges)
    return touched, np.searchsorted(touched, edges)


def labels_compacted(edges, n):
    touched, e = compact(edges)
    lab = np.arange(n, dtype=np.int32)
    lab[touched] = touched[CM.labels(e, len(touched))]
    return lab


def greedy_compacted(edges, n, keys=None):
    """(uint8 [n] flags by greedy_model.representatives, the rounds of greedy_model.rounds_synchronous)"""
    touched, e = compact(edges)
    kc = None if keys is None else keys[touched]
    rounds, by_rounds = GM.rounds_synchronous(e, len(touched), kc)
    rep_c = GM.representatives(e, len(touched), kc)
    assert np.array_equal(rep_c, by_rounds)
    rep = np.ones(n, dtype=np.uint8)
    rep[touched] = rep_c
    return rep, max(rounds, min(n, 1))                                # (the untouched vertices are decided in round 1)


def forest_compacted(edges, values, n):
    """((a, b, image) edges in BEFORE order by forest_model.kruskal, int32 [n] labels, the rounds of forest_model.boruvka_rounds)"""
    touched, e = compact(edges)
    recs = FM.records_of(e, values)
    k, lab = FM.kruskal(recs, len(touched))
    b, comp, rounds = FM.boruvka_rounds(recs, len(touched))
    assert k == b and lab == comp
    t = touched.tolist()
    full = np.arange(n, dtype=np.int32)
    full[touched] = touched[np.array(lab, dtype=np.int64)]
    return [(t[a], t[b], im) for a, b, im in k], full, rounds


def forest_values(p, which):
    rng = np.random.default_rng(p)
    return {"null": None, "distinct": rng.permutation(p) / p, "levels": rng.integers(0, 3, size=p) / 4.0}[which]


def tied_keys(n, seed):
    """random 64-bit keys; every third vertex has one of three keys instead, so that ties are everywhere, the tail included"""
    rng = np.random.default_rng(seed)
    keys = rng.integers(0, 1 << 64, size=n, dtype=np.uint64)
    keys[::3] = rng.integers(1, 4, size=len(keys[::3])).astype(np.uint64) << np.uint64(62)
    return keys


def test_compaction_is_the_model():
    """on 5 000 vertices of which fewer than half are touched: the compacted route and the full model agree, for all three models"""
    n = 5000
    edges = np.concatenate([sparse_random(4800, 1000, 21), path(60, "shuffled") + 4900, np.array([[n - 1, 0], [7, 7]])])
    assert 1000 < len(np.unique(edges)) < n // 2 and not np.any(edges == n - 2)
    assert np.array_equal(labels_compacted(edges, n), CM.labels(edges, n))
    for keys in (None, tied_keys(n, 5)):
        rep, rounds = greedy_compacted(edges, n, keys)
        full_rounds, full_rep = GM.rounds_synchronous(edges, n, keys)
        assert np.array_equal(rep, GM.representatives(edges, n, keys)) and np.array_equal(rep, full_rep) and rounds == full_rounds
    for which in ("null", "distinct", "levels"):
        values = forest_values(len(edges), which)
        k, lab, rounds = forest_compacted(edges, values, n)
        recs = FM.records_of(edges, values)
        want_k, want_lab = FM.kruskal(recs, n)
        assert k == want_k and lab.tolist() == want_lab and rounds == FM.boruvka_rounds(recs, n)[2]
    none = np.zeros((0, 2), dtype=np.int64)
    assert np.array_equal(labels_compacted(none, 9), np.arange(9)) and greedy_compacted(none, 9)[1] == GM.rounds_synchronous(none, 9)[0] == 1


# ---- the graph holds what makes the second trip matter -----------------------------------------------------------------------------------------
def want_labels():
    if "labels" not in _MODEL:
        _MODEL["labels"] = labels_compacted(EDGES, N)
    return _MODEL["labels"]


def test_the_graph_lies_where_it_should():
    lab = want_labels()
    assert len(EDGES) <= 20000 and EDGES.min() >= 0 and EDGES.max() == N - 1
    size = np.bincount(lab, minlength=N)
    # wholly inside the tail: their roots -- the smallest member -- lie in the second trip
    assert np.all(lab[TAIL_PATH[0]:TAIL_PATH[1]] == TAIL_PATH[0]) and size[TAIL_PATH[0]] == 1000
    for lo, k in TAIL_CLIQUES:
        assert np.all(lab[lo:lo + k] == lo) and size[lo] == k and 5 <= k <= 40
    assert np.all(lab[STAR_LEAVES[0]:STAR_LEAVES[1]] == STAR_LEAVES[0]) and lab[N - 1] == STAR_LEAVES[0] and size[STAR_LEAVES[0]] == 501
    tail_roots = np.flatnonzero((lab == np.arange(N)) & (size > 1))
    assert (tail_roots >= CAP).sum() == 2 + len(TAIL_CLIQUES)
    # straddling the boundary: a root in the head, members in the tail
    g = np.arange(*TWINS)
    assert np.all(lab[g] == lab[g - CAP]) and np.all(lab[g] < CAP) and np.all((g % CAP) == g - CAP)
    assert np.all(lab[STRADDLE[0]:STRADDLE[1] + 1] == STRADDLE[0]) and size[STRADDLE[0]] == 401 and STRADDLE[0] < CAP <= STRADDLE[1]
    # the head: components of mixed size
    head = size[:1_000_000]
    assert head.max() > 20 and (head == 2).sum() > 100 and (head == 3).sum() > 30
    for v in (CAP - 1, CAP, N - 1):
        assert np.any(EDGES == v), v
    assert not np.any(EDGES == N - 2) and lab[N - 2] == N - 2
    # the shape of the second trip
    assert N - CAP == 4167 and -(-(N - CAP) // 256) == 17 and (N - CAP) % 256 % 64 == 7


# ---- the inputs on the device ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev_edges():
    return torch.from_numpy(EDGES.astype(np.int32)).cuda()


@pytest.fixture(scope="module")
def no_edges():
    return torch.zeros((0, 2), dtype=torch.int32, device="cuda")


# ---- the three graph entries at n = 1 052 743 ----------------------------------------------------------------------------------------------------
def test_components(dev_edges):
    want = want_labels()
    first, again = components_raw(dev_edges, N), components_raw(dev_edges, N)
    assert first.dtype == np.int32 and first.tobytes() == again.tobytes()
    assert np.array_equal(first, want), np.flatnonzero(first != want)[:5]


@pytest.mark.parametrize("keyed", [False, True], ids=["null-key", "tied-keys"])
def test_greedy_representatives(dev_edges, keyed):
    keys = tied_keys(N, 9) if keyed else None
    if keyed:
        assert len(np.unique(keys[CAP:])) < N - CAP and len(np.unique(keys[np.unique(EDGES)])) < len(np.unique(EDGES))      # ties in the tail, and on edges
    want, bound = greedy_compacted(EDGES, N, keys)
    if not keyed:
        # the key is the vertex: the tail is visited first, so its picks are made before any of the head's
        assert want[N - 1] == 1 and not want[STAR_LEAVES[0]:STAR_LEAVES[1]].any()
        assert want[CAP + 3000:CAP + 3200].all() and want[TAIL_PATH[1] - 1] == 1
    assert 0 < want[CAP:].sum() < N - CAP and want[N - 2] == 1
    first, rounds = greedy_raw(dev_edges, N, keys)
    again, rounds_again = greedy_raw(dev_edges, N, keys)
    assert first.tobytes() == again.tobytes()
    assert np.array_equal(first, want), np.flatnonzero(first != want)[:5]
    print(f"rounds {rounds}, {rounds_again} of at most {bound}")
    assert 1 <= rounds <= bound and 1 <= rounds_again <= bound


@pytest.mark.parametrize("which", ["null", "distinct", "levels"])
def test_spanning_forest(dev_edges, which):
    values = forest_values(len(EDGES), which)
    k, want_lab, want_rounds = forest_compacted(EDGES, values, N)
    assert np.array_equal(want_lab, want_labels())
    assert sum(a >= CAP for a, _, _ in k) >= 999 + 500 and sum(a < CAP <= b for a, b, _ in k) >= 201       # edges inside the tail, and across the boundary
    dvals = None if values is None else torch.from_numpy(values).cuda()
    first = forest_raw(dev_edges, dvals, N)
    again = forest_raw(dev_edges, dvals, N)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and first[2:] == again[2:]
    got, got_lab, f, rounds = first
    assert f == len(k) and got.tobytes() == FM.as_records(k).tobytes(), (which, f, len(k))
    assert np.array_equal(got_lab, want_lab), which
    assert rounds == want_rounds, (which, rounds, want_rounds)


def test_lists_with_no_entries(no_edges):
    """n_pairs = 0: the three singleton kernels over all n"""
    ident = np.arange(N, dtype=np.int32)
    assert np.array_equal(components_raw(no_edges, N), ident)
    flags, rounds = greedy_raw(no_edges, N)
    assert flags.all() and rounds == 1
    flags, rounds = greedy_raw(no_edges, N, tied_keys(N, 3))
    assert flags.all() and rounds == 1
    for dvals in (None, torch.zeros(1, dtype=torch.float64, device="cuda")):
        got, lab, f, rounds = forest_raw(no_edges, dvals, N)
        assert f == 0 and len(got) == 0 and np.array_equal(lab, ident) and rounds == FM.boruvka_rounds([], 4)[2] == 1


# ---- the merge by group over the same n rows ---------------------------------------------------------------------------------------------------
def test_merge_sketches():
    """p = 4 (16-byte HLL rows), m = 1 (the smallest the entry takes), no auxiliary kind; -1 for most rows; 1 000 groups with members on
    both sides of the boundary, four groups wholly in the tail, one of them longer than two segments"""
    rng = np.random.default_rng(4167)
    mixed, G = 1000, 1004
    groups = np.full(N, -1, dtype=np.int32)
    head = rng.choice(CAP, 6000, replace=False)
    tail = CAP + 1 + rng.permutation(N - CAP - 3)                      # (all but the boundary row and the last two, set below)
    groups[head] = rng.integers(0, mixed, len(head))
    groups[tail[:3000]] = np.concatenate([np.arange(mixed), rng.integers(0, mixed, 2000)])
    at = 3000
    for g, count in zip(range(mixed, G), (1, 2, S + 1, 2 * S + 3)):
        groups[tail[at:at + count]] = g
        at += count
    groups[[CAP - 1, CAP, N - 1]] = (0, 0, 1)                          # the boundary rows and the last row are members
    assert groups[N - 2] == -1 and (groups == -1).sum() > N - 10000
    ids = np.arange(N)
    lo_of = np.full(G, N)
    np.minimum.at(lo_of, groups[groups >= 0], ids[groups >= 0])
    hi_of = np.full(G, -1)
    np.maximum.at(hi_of, groups[groups >= 0], ids[groups >= 0])
    assert ((lo_of[:mixed] < CAP) & (hi_of[:mixed] >= CAP)).sum() > 900 and np.all(lo_of[mixed:] >= CAP) and np.all(hi_of[mixed:] < N)
    hll = rng.integers(0, 256, (N, 16), dtype=np.uint8)
    smh = rng.integers(0, 1 << 64, (N, 1), dtype=np.uint64)
    want = MM.merge_all(hll, smh, None, groups, G)
    assert list(want["sizes"][mixed:]) == [1, 2, S + 1, 2 * S + 3] and want["sizes"][:mixed].min() >= 1
    rc, out = raw_merge(to_dev(hll), to_dev(smh), None, to_dev(groups), N, G)
    assert rc == 0, pkg.hip_lib().selhip_last_error(None).decode()
    assert_is_model(out, want, G, "n = 1 052 743")
