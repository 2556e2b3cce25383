"""Single-linkage clusters on the GPU (selhip_components, selhip_ctx_cluster).  Every output is compared for exact
equality with tests/cluster_model.py -- a sequential union-find in Python -- run on the same edge list, or on the records fetched from
the pass.  The graphs of (1) are built to break a concurrent union-find: long parent chains, every hook on one root, one giant
component, a bridge in the last entry; each runs with the default grid and with the edge kernel's grid forced to 1 and 2 blocks (the
grid-stride loop then runs many times), twice, and the two runs must be byte-equal.  Those record grids are crossed with the vertex
kernels' grid ("vertex_blocks": sized from n, 1 block, 3 blocks), so that the loops over the vertices come round too (DESIGN.md
section 32); test_vertex_trips_of_the_context_call does the same for every kernel of selhip_ctx_cluster at 771 genomes."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import cluster_model as CM
import smhc_model as M
import smhv_model as V
from test_smhv_gpu import case, configure, zeros_hll

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import CRIT_NONE, CRIT_SMH_A, CRIT_SMH_C, MODE_CB_SMH, MODE_SMH, SelhipError, Selector

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
GUARD = 64                     # int32 words of sentinel on both sides of every output array
SENTINEL = -77
OUTPUTS = ("labels", "clusters", "degrees", "sizes", "representatives")


@pytest.fixture
def grid_hook():
    """sets the process-wide grids of the edge kernel and of the vertex kernels (0 = automatic) and puts the defaults back"""
    with Selector(0) as sel:
        def set_hooks(blocks, vertex_blocks=0):
            sel.set_param("cluster_blocks", blocks)
            sel.set_param("vertex_blocks", vertex_blocks)
            assert (sel.get_param("cluster_blocks"), sel.get_param("vertex_blocks")) == (blocks, vertex_blocks)
        yield set_hooks
        set_hooks(0, 0)


VERTEX_BLOCKS = (0, 1, 3)      # the vertex kernels' grid: sized from n, one block, three blocks (strides of 256 and of 768 vertices)


def hook_grid(record_blocks):
    """the ("cluster_blocks", "vertex_blocks") pairs a case runs under: the file's record grids crossed with VERTEX_BLOCKS"""
    return [(b, v) for v in VERTEX_BLOCKS for b in record_blocks]


# ---- 1. + 2. selhip_components on graphs built to break a union-find, every grid, twice ----------------------------------------------------
def path(n, order):
    e = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    if order == "descending":
        e = e[::-1, ::-1]
    elif order == "shuffled":
        rng = np.random.default_rng(7)
        e = e[rng.permutation(len(e))]
        flip = rng.random(len(e)) < 0.5
        e[flip] = e[flip][:, ::-1]
    return np.ascontiguousarray(e)


def star(n, centre):
    leaves = np.array([g for g in range(n) if g != centre])
    return np.stack([np.full(n - 1, centre), leaves], axis=1)


def clique(lo, hi):
    i, k = np.triu_indices(hi - lo, 1)
    return np.stack([i + lo, k + lo], axis=1)


def sparse_random(n, p_edges, seed):
    return np.random.default_rng(seed).integers(0, n, size=(p_edges, 2))


def with_noise(e, n, seed):
    """every entry twice (the second time reversed) and self-loops mixed in, shuffled"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, n, size=max(3, len(e) // 4))
    out = np.concatenate([e, e[:, ::-1], np.stack([v, v], axis=1)])
    return out[rng.permutation(len(out))]


def graphs():
    g = [("n1", 1, np.zeros((0, 2), dtype=np.int64)), ("n1-loop", 1, np.array([[0, 0]])),
         ("n2-apart", 2, np.zeros((0, 2), dtype=np.int64)), ("n2-edge", 2, np.array([[1, 0]])),
         ("path-ascending", 4097, path(4097, "ascending")), ("path-descending", 4097, path(4097, "descending")),
         ("path-shuffled", 4097, path(4097, "shuffled")),
         ("star-centre-highest", 65537, star(65537, 65536)), ("star-centre-0", 65537, star(65537, 0)),
         ("n1000-apart", 1000, np.zeros((0, 2), dtype=np.int64)), ("K300", 300, clique(0, 300)),
         ("two-cliques-bridge-last", 300, np.concatenate([clique(0, 150), clique(150, 300), np.array([[299, 0]])])),
         ("two-cliques-apart", 300, np.concatenate([clique(0, 150), clique(150, 300)])),
         ("sparse-5000", 5000, sparse_random(5000, 2500, 11)),
         ("duplicates-and-loops", 5000, with_noise(sparse_random(5000, 2500, 12), 5000, 13)),
         ("path-with-noise", 1025, with_noise(path(1025, "shuffled"), 1025, 14))]
    for p_edges in (0, 63, 64, 65, 255, 256, 257):
        g.append((f"pairs-{p_edges}", 300, sparse_random(300, p_edges, 100 + p_edges)))
    return g


GRAPHS = graphs()
_WANT = {}


def want_labels(name, n, edges):
    if name not in _WANT:
        _WANT[name] = CM.labels(edges, n)
    return _WANT[name]


def components_raw(dev_pairs, n):
    """selhip_components into a buffer filled with a sentinel, guards on both sides: a vertex the call left unwritten shows (torch.empty
    would hand a second call the block, and the answer, of the first)"""
    lib = pkg.hip_lib()
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    rc = lib.selhip_components(dev_pairs.data_ptr() if dev_pairs.numel() else None, int(dev_pairs.shape[0]), n, buf.data_ptr() + 4 * GUARD, None)
    assert rc == 0, lib.selhip_last_error(None).decode()
    out = buf.cpu().numpy()
    assert np.all(out[:GUARD] == SENTINEL) and np.all(out[GUARD + n:] == SENTINEL)
    return out[GUARD:GUARD + n].copy()


@pytest.mark.parametrize("name,n,edges", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_components(grid_hook, name, n, edges):
    want = want_labels(name, n, edges)
    if name == "K300":
        assert len(edges) == 44850 and np.all(want == 0)
    if name == "two-cliques-bridge-last":
        assert np.all(want == 0) and np.array_equal(np.unique(CM.labels(edges[:-1], 300)), [0, 150])
    if name == "sparse-5000":
        sizes = np.bincount(want)
        assert sizes.max() > 3 and (sizes == 1).sum() > 100                     # many components of mixed size
    dev = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)).cuda()
    for blocks, vblocks in hook_grid((0, 1, 2)):
        grid_hook(blocks, vblocks)
        first = components_raw(dev, n)
        again = components_raw(dev, n)
        assert first.dtype == np.int32 and first.tobytes() == again.tobytes(), (name, blocks, vblocks)
        assert np.array_equal(first, want), (name, blocks, vblocks, np.flatnonzero(first != want)[:5])
    grid_hook(0)
    assert np.array_equal(pkg.components(np.asarray(edges), n), want)            # a host list is copied to the device


@pytest.mark.parametrize("bad", [(-1, 5), (7, 100), (100, 7), (-3, 100), (1 << 30, -(1 << 31))])
def test_components_invalid_entry(grid_hook, bad):
    n = 100
    edges = sparse_random(n, 300, 5).astype(np.int32)
    edges[[17, 230]] = bad                                                         # two such entries
    lib = pkg.hip_lib()
    dev = torch.from_numpy(edges).cuda()
    for blocks, vblocks in hook_grid((0, 1)):
        grid_hook(blocks, vblocks)
        buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        rc = lib.selhip_components(dev.data_ptr(), len(edges), n, buf.data_ptr() + 4 * GUARD, None)
        msg = lib.selhip_last_error(None).decode()
        assert rc == -1, (rc, msg)
        assert "2 invalid entries" in msg and f"[0, {n})" in msg and ("entry 17 is one" in msg or "entry 230 is one" in msg), msg
        out = buf.cpu().numpy()
        assert np.all(out[:GUARD] == SENTINEL) and np.all(out[GUARD + n:] == SENTINEL)
    grid_hook(0)
    # the same list without them is fine, and the guards stay
    edges[[17, 230]] = (0, 0)
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    assert lib.selhip_components(torch.from_numpy(edges).cuda().data_ptr(), len(edges), n, buf.data_ptr() + 4 * GUARD, None) == 0
    out = buf.cpu().numpy()
    assert np.all(out[:GUARD] == SENTINEL) and np.all(out[GUARD + n:] == SENTINEL)
    assert np.array_equal(out[GUARD:GUARD + n], CM.labels(edges, n))
    with pytest.raises(SelhipError, match="invalid entries"):
        pkg.components(np.array([[0, 1], [1, n]]), n)
    with pytest.raises(SelhipError, match=r"outside \[0, 0\)"):
        pkg.components(np.array([[0, 0]]), 0)
    assert len(pkg.components(np.zeros((0, 2), dtype=np.int32), 0)) == 0


# ---- the context entry: raw calls into guarded buffers ------------------------------------------------------------------------------------
def raw_cluster(sel, min_value, rule, null=()):
    """selhip_ctx_cluster into five arrays with sentinel guards; the outputs named in `null` are passed as NULL.  Returns the dict the
    model returns (without the NULL ones), after checking that nothing outside the written entries changed"""
    n = sel.n
    stride = n + 2 * GUARD
    buf = torch.full((5 * stride,), SENTINEL, dtype=torch.int32, device="cuda")
    ptrs = [None if name in null else buf.data_ptr() + 4 * (j * stride + GUARD) for j, name in enumerate(OUTPUTS)]
    out = pkg._lib.Clusters(*ptrs)
    cnt = C.c_int64(-5)
    pkg._lib.check(sel._lib.selhip_ctx_cluster(sel._ctx, float(min_value), int(rule), C.byref(out), C.byref(cnt)), sel._ctx)
    c = cnt.value
    host = buf.cpu().numpy().reshape(5, stride)
    res = {"n_clusters": c}
    for j, name in enumerate(OUTPUTS):
        written = 0 if name in null else c if name in ("sizes", "representatives") else n
        assert np.all(host[j, :GUARD] == SENTINEL) and np.all(host[j, GUARD + written:] == SENTINEL), (name, null, c)
        if name not in null:
            res[name] = host[j, GUARD:GUARD + written].copy()
    assert sel.get_param("clusters_last") == c
    return res


def assert_same(got, want, what=""):
    assert got["n_clusters"] == want["n_clusters"], (what, got["n_clusters"], want["n_clusters"])
    for name in OUTPUTS:
        if name in got:
            assert got[name].dtype == np.int32 and np.array_equal(got[name], want[name]), (what, name)


def snapshot(sel):
    return sel.fetch().tobytes(), sel.stats(), sel.last_attempts(), sel.result_count()


# ---- 3. behind an all-pairs pass: planted groups, every criterion, sizes around the wave and block edges ---------------------------------
@pytest.mark.parametrize("crit", ["smh_a", "smh_c-hll", "smh_c-smh", "none"])
def test_cluster_behind_all_pairs(oracle, grid_hook, crit):
    m = 256
    n_mixed = 0
    with Selector(0) as sel:
        assert sel.get_param("clusters_last") == -1
        for n in (1, 2, 65, 129, 257):
            if crit == "smh_c-smh":
                aux, cards = case(n, m)
                sel.upload(zeros_hll(n), aux, cards)
                configure(sel, c_min=1)
                run = lambda: sel.run(-1.0, MODE_SMH, 7, 3)                      # noqa: E731
            else:
                hll, aux, cards = M.ranked(oracle, M.hll_pool(n), M.planted_groups(n, m, 77 + n))
                sel.upload(hll, aux, cards)
                sel.set_estimator("hll")
                sel.set_measure("jaccard")
                if crit == "smh_a":
                    sel.set_criterion(CRIT_SMH_A)
                    run = lambda: sel.run(0.3, MODE_CB_SMH, 2, 128)              # noqa: E731
                elif crit == "none":
                    sel.set_criterion(CRIT_NONE)
                    run = lambda: sel.run(0.3, MODE_CB_SMH, 1, 1)                # noqa: E731
                else:
                    sel.set_criterion(CRIT_SMH_C)
                    sel.set_min_matches(m // 2)
                    run = lambda: sel.run(0.3, MODE_CB_SMH, 7, 3)                # noqa: E731
            rec = run()
            before = snapshot(sel)
            values = np.unique(rec["jaccard"])
            cuts = [-np.inf] + ([float(values[len(values) // 2]), float(values[-1])] if len(values) else [])
            for min_value in cuts:
                edges = CM.record_edges(rec, min_value)
                want = CM.clusters(edges, n, "max_degree")
                for blocks, vblocks in hook_grid((0, 1)):
                    grid_hook(blocks, vblocks)
                    assert_same(raw_cluster(sel, min_value, 0), want, (crit, n, min_value, blocks, vblocks))
                n_mixed += 1 < want["n_clusters"] < n
            grid_hook(0)
            # every output pointer NULL in turn: the others are still right, nothing else is written
            want = CM.clusters(CM.record_edges(rec), n, "max_degree")
            for name in OUTPUTS:
                assert_same(raw_cluster(sel, -np.inf, 0, null=(name,)), want, (crit, n, "null", name))
            assert raw_cluster(sel, -np.inf, 0, null=OUTPUTS) == {"n_clusters": want["n_clusters"]}
            # the wrapper: numpy arrays, and tensors on the device
            got = sel.cluster()
            assert_same(got, want, (crit, n, "wrapper"))
            dev = sel.cluster(to_host=False)
            assert all(dev[k].is_cuda and np.array_equal(dev[k].cpu().numpy(), want[k]) for k in OUTPUTS) and dev["n_clusters"] == want["n_clusters"]
            assert snapshot(sel) == before, (crit, n)                               # list, statistics, attempts: as they were
    assert n_mixed > 0, crit


def test_cluster_small_pass_default_context(oracle):
    """the one-launch small pass (the default of a context the suite does not configure) leaves a list like any other"""
    n, m = 129, 256
    hll, aux, cards = M.ranked(oracle, M.hll_pool(n), M.planted_groups(n, m, 5))
    with Selector(0) as sel:
        sel.set_param("small_pass", -1)
        sel.upload(hll, aux, cards)
        rec = sel.run(0.3, MODE_CB_SMH, 2, 128)
        assert sel.get_param("small_pass_used") == 1 and len(rec) > 0
        assert_same(raw_cluster(sel, -np.inf, 0), CM.clusters(CM.record_edges(rec), n), "small pass")


# ---- 4. the threshold boundary --------------------------------------------------------------------------------------------------------------
def test_threshold_boundary():
    n, m = 129, 128
    aux, cards = case(n, m)
    with Selector(0) as sel:
        sel.upload(zeros_hll(n), aux, cards)
        configure(sel, c_min=1)
        rec = sel.run(-1.0, MODE_SMH, 7, 3)
        n_at = lambda v: CM.clusters(CM.record_edges(rec, v), n)["n_clusters"]       # noqa: E731
        # a record's value J at which cutting just above it changes the component count: its edge is a bridge at that level
        J = next(float(v) for v in np.unique(rec["jaccard"]) if n_at(v) != n_at(np.nextafter(v, np.inf)))
        above = float(np.nextafter(J, np.inf))
        keep, drop = raw_cluster(sel, J, 0), raw_cluster(sel, above, 0)
        assert_same(keep, CM.clusters(CM.record_edges(rec, J), n), "J")
        assert_same(drop, CM.clusters(CM.record_edges(rec, above), n), "nextafter(J)")
        assert keep["n_clusters"] < drop["n_clusters"]
        assert_same(raw_cluster(sel, -np.inf, 0), CM.clusters(CM.record_edges(rec), n), "-inf")
        assert int(raw_cluster(sel, -np.inf, 0)["degrees"].sum()) == 2 * len(rec)     # -inf takes every record
        alone = raw_cluster(sel, np.inf, 0)
        assert_same(alone, CM.clusters(np.zeros((0, 2), dtype=np.int64), n), "+inf")
        assert alone["n_clusters"] == n and np.array_equal(alone["labels"], np.arange(n)) and np.all(alone["sizes"] == 1)
        last = sel.get_param("clusters_last")
        with pytest.raises(SelhipError, match="NaN") as err:
            raw_cluster(sel, np.nan, 0)
        assert err.value.code == -1 and sel.get_param("clusters_last") == last
        # several levels from the one pass
        for v in (0.25, 0.5, 0.75, 1.0):
            assert_same(raw_cluster(sel, v, 0), CM.clusters(CM.record_edges(rec, v), n), v)


# ---- 5. the representative rules ------------------------------------------------------------------------------------------------------------
def test_representative_rules():
    """a path 3 - 9 - 4 - 12 planted in random rows: degrees 1, 2, 2, 1, so the two middle genomes tie and the smaller rank, 4, wins under
    max_degree; min_rank is the label 3; max_rank is 12.  A triangle 15, 16, 17 with one more leaf on 17; everything else alone"""
    n, m = 20, 128
    rng = np.random.default_rng(3)
    aux = rng.integers(1, 1 << 62, size=(n, m), dtype=np.uint64)
    for a, b, lo in ((3, 9, 0), (9, 4, 10), (4, 12, 20), (15, 16, 30), (16, 17, 40), (15, 17, 50), (17, 19, 60)):
        aux[b, lo:lo + 10] = aux[a, lo:lo + 10]
    aux[17, 30:40] = rng.integers(1, 1 << 62, size=10, dtype=np.uint64)           # (17 copied 16's share with 15: undo)
    aux[17, 50:60] = aux[15, 50:60]
    with Selector(0) as sel:
        sel.upload(zeros_hll(n), aux, V.spread_cards(n))
        configure(sel, c_min=1)
        rec = sel.run(-1.0, MODE_SMH, 7, 3)
        assert sorted(zip(rec["i"].tolist(), rec["k"].tolist())) == [(3, 9), (4, 9), (4, 12), (15, 16), (15, 17), (16, 17), (17, 19)]
        edges = CM.record_edges(rec)
        got = {rule: raw_cluster(sel, -np.inf, code) for rule, code in CM.REP_NAMES.items()}
        for rule in CM.REP_NAMES:
            assert_same(got[rule], CM.clusters(edges, n, rule), rule)
        c_path, c_tri = got["max_degree"]["clusters"][3], got["max_degree"]["clusters"][15]
        assert got["max_degree"]["degrees"][[3, 9, 4, 12]].tolist() == [1, 2, 2, 1]
        assert got["max_degree"]["representatives"][c_path] == 4 and got["max_degree"]["representatives"][c_tri] == 17
        assert got["min_rank"]["representatives"][c_path] == 3 == got["min_rank"]["labels"][12]
        assert np.array_equal(got["min_rank"]["representatives"], np.unique(got["min_rank"]["labels"]))
        assert got["max_rank"]["representatives"][c_path] == 12 and got["max_rank"]["representatives"][c_tri] == 19
        single = got["max_degree"]["clusters"][0]
        assert got["max_degree"]["sizes"][single] == 1 and got["max_degree"]["representatives"][single] == 0 and got["max_degree"]["degrees"][0] == 0
        assert_same(sel.cluster(rep="max_rank"), CM.clusters(edges, n, "max_rank"), "wrapper")
        for code in (3, -1, 100):
            with pytest.raises(SelhipError, match="rep_rule") as err:
                raw_cluster(sel, -np.inf, code)
            assert err.value.code == -1
        with pytest.raises(ValueError, match="rep"):
            sel.cluster(rep="degree")


def test_vertex_trips_of_the_context_call(grid_hook):
    """771 genomes = three blocks of 256 and three lanes: with the vertex kernels in one block every loop of selhip_ctx_cluster comes
    round four times and ends in a wave of three lanes; with three blocks it comes round twice.  Every output, each representative
    rule, two cuts; twice, byte-equal"""
    from test_greedy_gpu import planted_pass, random_weighted                            # (that module imports this one)
    n, m = 771, 256
    with Selector(0) as sel:
        rec = planted_pass(sel, n, m, random_weighted(n, 771), seed=771)                 # a sparse random graph: components across the trips
        for min_value in (-np.inf, 8 / m):
            edges = CM.record_edges(rec, min_value)
            for rule, code in CM.REP_NAMES.items():
                want = CM.clusters(edges, n, rule)
                far = np.flatnonzero(np.arange(n) // 256 != want["labels"] // 256)       # members a trip or more away from their root
                assert 1 < want["n_clusters"] < n and want["sizes"].max() > 50 and (want["sizes"] == 1).sum() > 20 and len(far) > 100
                for blocks, vblocks in hook_grid((0, 1)):
                    grid_hook(blocks, vblocks)
                    first, again = raw_cluster(sel, min_value, code), raw_cluster(sel, min_value, code)
                    assert all(first[k].tobytes() == again[k].tobytes() for k in OUTPUTS), (rule, blocks, vblocks)
                    assert_same(first, want, (min_value, rule, blocks, vblocks))
        grid_hook(0, 3)
        assert len(sel.run(2.0, MODE_SMH, 7, 3)) == 0                                   # no record: cluster_singletons_kernel, two trips
        assert_same(raw_cluster(sel, -np.inf, 0), CM.clusters(np.zeros((0, 2), dtype=np.int64), n), "empty list")


# ---- 6. the kinds of list, the refusals, and what the call leaves alone -------------------------------------------------------------------
def test_list_kinds_and_state():
    n, m = 257, 128
    aux, cards = case(n, m)
    with Selector(0) as sel:
        sel.upload(zeros_hll(n), aux, cards)
        with pytest.raises(SelhipError, match="no result list") as err:              # before any pass
            raw_cluster(sel, -np.inf, 0)
        assert err.value.code == -5
        configure(sel, c_min=1)
        # the directed top-k list, one-shot and in row rounds: records counted, a mutual pair twice
        whole = sel.run(-1.0, MODE_SMH, 7, 3, top_k=0)
        lists = []
        for rounds in (0, 16):
            ranked = sel.run(-1.0, MODE_SMH, 7, 3, top_k=3, rounds=rounds)
            assert sel.get_param("topk_rounds_used") == (17 if rounds else 0)
            lists.append(ranked.tobytes())
            before = snapshot(sel), sel.fetch_ranked().tobytes()
            want = CM.clusters(CM.record_edges(ranked), n)
            assert_same(raw_cluster(sel, -np.inf, 0), want, ("top-k", rounds))
            pairs = set(zip(ranked["i"].tolist(), ranked["k"].tolist()))
            assert any((k, i) in pairs for i, k in pairs)                            # mutual pairs exist ...
            partners = np.array([len({k for i, k in pairs if i == g} | {i for i, k in pairs if k == g}) for g in range(n)])
            assert np.all(want["degrees"] >= partners) and np.any(want["degrees"] > partners)    # ... and count twice
            cut = float(np.median(ranked["jaccard"]))
            assert_same(raw_cluster(sel, cut, 2), CM.clusters(CM.record_edges(ranked, cut), n, "max_rank"), ("top-k cut", rounds))
            assert (snapshot(sel), sel.fetch_ranked().tobytes()) == before
            assert sel.get_param("allpairs_topk") == 3 and sel.get_param("topk_rounds") == rounds
        assert lists[0] == lists[1]
        sel.set_topk_rounds(0)
        sel.set_allpairs_topk(0)
        # a pair list with an entry listed twice
        lst = np.concatenate([np.stack([whole["k"], whole["i"]], axis=1)[:40], np.stack([whole["i"], whole["k"]], axis=1)[:3]]).astype(np.int32)
        rec = sel.run_pairs(lst, -1.0, MODE_SMH, 7, 3)
        assert len(rec) == 43
        want = CM.clusters(CM.record_edges(rec), n)
        assert_same(raw_cluster(sel, -np.inf, 0), want, "pair list")
        assert want["degrees"][whole["i"][0]] >= 2 and int(want["degrees"].sum()) == 86
        # a pass that selected nothing: n singletons
        sel.timing(1)
        assert len(sel.run(2.0, MODE_SMH, 7, 3)) == 0
        assert_same(raw_cluster(sel, -np.inf, 0), CM.clusters(np.zeros((0, 2), dtype=np.int64), n), "empty list")
        assert sel.kernel_ms("cluster") > 0
        # a query pass leaves a list in two index spaces
        sel.upload_queries(zeros_hll(5), aux[:5], cards[:5])
        assert len(sel.run_queries(-1.0, MODE_SMH, 7, 3)) > 0
        last = sel.get_param("clusters_last")
        with pytest.raises(SelhipError, match="query pass") as err:
            raw_cluster(sel, -np.inf, 0)
        assert err.value.code == -5 and sel.get_param("clusters_last") == last
        # between run_async and finish; it works after finish
        sel.run_async(-1.0, MODE_SMH, 7, 3)
        with pytest.raises(SelhipError, match="pending") as err:
            raw_cluster(sel, -np.inf, 0)
        assert err.value.code == -5
        sel.finish()
        rec = sel.fetch()
        assert M.tuples(rec) == M.tuples(whole)
        want = CM.clusters(CM.record_edges(rec), n)
        assert_same(raw_cluster(sel, -np.inf, 0), want, "after finish")
        # a matrix call in between changes nothing
        before = snapshot(sel)
        sel.matrix("smh_jaccard")
        assert_same(raw_cluster(sel, -np.inf, 0), want, "behind a matrix call")
        assert snapshot(sel) == before
        # timing: "cluster" per cluster call, the passes' figures untouched
        sel.timing(1)
        sel.run(-1.0, MODE_SMH, 7, 3)
        names = ("prep", "stage1", "total", "topk", "matrix", "matrix_smh", "hist", "select")
        ms, launches = [sel.kernel_ms(k) for k in names], [sel.kernel_launches(k) for k in names]
        assert sel.kernel_ms("cluster") < 0
        raw_cluster(sel, -np.inf, 0)
        raw_cluster(sel, 0.5, 1)
        assert sel.kernel_ms("cluster") > 0 and sel.kernel_launches("cluster") == 1.0      # one timed scope per call, two calls
        assert [sel.kernel_ms(k) for k in names] == ms and [sel.kernel_launches(k) for k in names] == launches
        sel.timing(0)
        # an upload drops the list: SELHIP_E_STATE again
        sel.upload(zeros_hll(n), aux, cards)
        with pytest.raises(SelhipError) as err:
            raw_cluster(sel, -np.inf, 0)
        assert err.value.code == -5


# ---- 7. the front ends, on the influenza fixtures ------------------------------------------------------------------------------------------
def selection(args):
    out = subprocess.run([str(BIN / "selection")] + args, cwd=GOLDEN, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return out.stdout


CASES = {"smh_a": (["-h", "0.9", "-a", "512"], dict(tau=0.9, aux_bytes=512), None, "max_degree"),
         "smh_a-T0.95": (["-h", "0.9", "-a", "512"], dict(tau=0.9, aux_bytes=512), 0.95, "max_degree"),
         "smh_a-max_rank": (["-h", "0.9", "-a", "512"], dict(tau=0.9, aux_bytes=512), None, "max_rank"),
         "none-T-min_rank": (["-h", "0.5", "-a", "512", "-c", "none", "-n"], dict(tau=0.5, aux_bytes=512, criterion="none", mode=MODE_SMH), 0.9, "min_rank"),
         "knn": (["-c", "none", "-n", "-h", "-1", "-K", "3"], dict(tau=-1.0, aux_bytes=256, criterion="none", mode=MODE_SMH, top_k=3), None, "max_degree")}


@pytest.mark.parametrize("name", list(CASES))
def test_front_ends(monkeypatch, tmp_path, name):
    args, kw, level, rep = CASES[name]
    monkeypatch.chdir(GOLDEN)
    base = ["-l", "influenza_filelist.txt"] + args
    plain = selection(base)
    assert len(plain.splitlines()) > 0
    # the records the text was printed from, with their exact values, and the ranks of the list's lines
    m = kw["aux_bytes"] // 8 if kw.get("criterion", "smh_a") == "smh_a" else 0
    ds = pkg.load_dataset("influenza_filelist.txt", m)
    n = len(ds.names)
    with Selector(0) as sel:
        sel.upload(ds.hll, ds.aux if m else np.zeros((n, 1), dtype=np.uint64), ds.cards)
        sel.set_criterion(CRIT_SMH_A if m else CRIT_NONE)
        rec = sel.run(kw["tau"], kw.get("mode", MODE_CB_SMH), *(pkg.banding(m, kw["tau"]) if m else (1, 1)), top_k=kw.get("top_k") or None)
    assert pkg.format_lines(ds.names, rec) == plain
    f = tmp_path / "clusters.tsv"
    extra = (["-T", repr(level)] if level is not None else []) + (["-Y", rep] if rep != "max_degree" else [])
    assert selection(base + ["-L", str(f)] + extra) == plain                          # stdout: byte for byte what it is without -L
    want = CM.table(ds.names, ds.order, CM.clusters(CM.record_edges(rec, -np.inf if level is None else level), n, rep))
    text = f.read_text()
    assert text == want, name
    assert [ln.split("\t")[0] for ln in text.splitlines()] == (GOLDEN / "influenza_filelist.txt").read_text().split()
    assert pkg.cluster_from_filelist("influenza_filelist.txt", cluster_min=level, rep=rep, **kw) == want, name
