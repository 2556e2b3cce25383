"""Greedy representative clusters on the GPU (selhip_greedy_representatives, selhip_ctx_cluster_greedy).  Every
output is compared for exact equality -- values by their bits -- with tests/greedy_model.py, the sequential greedy in Python, run on
the same edge list or on the records fetched from the pass.  The graphs of (1) are those of test_cluster_gpu.py plus the orders that
stretch the round scheme: a path whose keys ascend along it (one round per vertex), stars with the centre first and last; each runs
with the default grid and with the edge kernel's grid forced to 1 and 2 blocks, twice, and the two runs must be byte-equal.  The device's
round count must lie in [1, rounds of the scheme with every read stale].  The record grids are crossed with the vertex kernels' grid
("vertex_blocks": sized from n, 1 block, 3 blocks); test_vertex_trips_of_the_context_call does the same for
every kernel of selhip_ctx_cluster_greedy at 771 genomes."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import cluster_model as CM
import greedy_model as GM
import smhc_model as M
import smhv_model as V
from test_cluster_gpu import clique, hook_grid, path, sparse_random, star, with_noise
from test_smhv_gpu import case, configure, zeros_hll

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import CRIT_NONE, CRIT_SMH_A, MODE_CB_SMH, MODE_SMH, SelhipError, Selector

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
GUARD = 64                     # words of sentinel on both sides of every output array
SENTINEL = -77
INT_OUTPUTS = ("rep_of", "clusters", "degrees", "sizes", "representatives")
OUTPUTS = INT_OUTPUTS + ("values",)
RULES = {"max_degree": 0, "min_rank": 1, "max_rank": 2, "priority": 3}


@pytest.fixture
def grid_hook():
    """sets the process-wide grids of the edge kernels and of the vertex kernels (0 = automatic) and puts the defaults back"""
    with Selector(0) as sel:
        def set_hooks(blocks, vertex_blocks=0):
            sel.set_param("cluster_blocks", blocks)
            sel.set_param("vertex_blocks", vertex_blocks)
            assert (sel.get_param("cluster_blocks"), sel.get_param("vertex_blocks")) == (blocks, vertex_blocks)
        yield set_hooks
        set_hooks(0, 0)


# ---- 1. selhip_greedy_representatives: the graph shapes, the key orders, every grid, twice ------------------------------------------------
def random_keys(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.uint64)


def graphs():
    none = np.zeros((0, 2), dtype=np.int64)
    rev = lambda n: np.arange(n - 1, -1, -1).astype(np.uint64)                       # noqa: E731
    g = [("n1", 1, none, None), ("n1-loop", 1, np.array([[0, 0]]), None), ("n2-apart", 2, none, None), ("n2-edge", 2, np.array([[1, 0]]), None),
         ("n1000-apart", 1000, none, None),
         ("n2-edge-equal-keys", 2, np.array([[1, 0]]), np.array([9, 9], dtype=np.uint64)),
         ("path-key-vertex", 4097, path(4097, "ascending"), None), ("path-key-reversed", 4097, path(4097, "shuffled"), rev(4097)),
         ("path-key-random", 4097, path(4097, "descending"), random_keys(4097, 3)),
         ("star-centre-first", 65537, star(65537, 65536), None), ("star-centre-last", 65537, star(65537, 0), None),
         ("K300", 300, clique(0, 300), None), ("K300-random-keys", 300, clique(0, 300), random_keys(300, 4)),
         ("two-cliques-bridge-last", 300, np.concatenate([clique(0, 150), clique(150, 300), np.array([[299, 0]])]), None),
         ("two-cliques-bridge-reversed", 300, np.concatenate([clique(0, 150), clique(150, 300), np.array([[299, 0]])]), rev(300)),
         ("sparse-5000", 5000, sparse_random(5000, 2500, 11), None), ("sparse-5000-dense-keys", 5000, sparse_random(5000, 10000, 15), random_keys(5000, 5)),
         ("duplicates-and-loops", 5000, with_noise(sparse_random(5000, 2500, 12), 5000, 13), random_keys(5000, 6)),
         ("path-with-noise", 1025, with_noise(path(1025, "shuffled"), 1025, 14), None),
         ("equal-keys", 5000, sparse_random(5000, 5000, 16), np.full(5000, 1 << 63, dtype=np.uint64)),
         ("few-key-levels", 5000, sparse_random(5000, 5000, 17), np.random.default_rng(8).integers(0, 3, size=5000).astype(np.uint64) << np.uint64(62))]
    for p_edges in (0, 63, 64, 65, 255, 256, 257):
        g.append((f"pairs-{p_edges}", 300, sparse_random(300, p_edges, 100 + p_edges), random_keys(300, p_edges) if p_edges % 2 else None))
    return g


GRAPHS = graphs()
_WANT = {}


def want_reps(name, n, edges, keys):
    if name not in _WANT:
        rounds, rep = GM.rounds_synchronous(edges, n, keys)
        if n <= 5000:
            assert np.array_equal(rep, GM.representatives(edges, n, keys))           # the scheme is the sequential greedy
        _WANT[name] = rep.astype(np.uint8), rounds
    return _WANT[name]


def greedy_raw(dev_pairs, n, keys=None):
    """selhip_greedy_representatives into a buffer filled with 0xAB, guards on both sides: (flags, rounds).  A vertex the call left
    unwritten shows (torch.empty would hand a second call the block, and the answer, of the first)"""
    lib = pkg.hip_lib()
    buf = torch.full((n + 2 * GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    key = None if keys is None else torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64)).cuda()
    rounds = C.c_int64(-9)
    rc = lib.selhip_greedy_representatives(dev_pairs.data_ptr() if dev_pairs.numel() else None, int(dev_pairs.shape[0]), n,
                                           None if key is None else key.data_ptr(), buf.data_ptr() + GUARD, C.byref(rounds), None)
    assert rc == 0, lib.selhip_last_error(None).decode()
    out = buf.cpu().numpy()
    assert np.all(out[:GUARD] == 0xAB) and np.all(out[GUARD + n:] == 0xAB)
    return out[GUARD:GUARD + n].copy(), rounds.value


@pytest.mark.parametrize("name,n,edges,keys", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_representatives(grid_hook, name, n, edges, keys):
    want, bound = want_reps(name, n, edges, keys)
    if name == "path-key-vertex":
        assert bound == 4097 and np.array_equal(want, np.arange(4097) % 2 == 0)       # the worst case: one round per vertex
    if name == "star-centre-first":
        assert want.sum() == 1 and want[65536] == 1
    if name == "star-centre-last":
        assert want.sum() == 65536 and want[0] == 0
    if name.startswith("K300"):
        assert want.sum() == 1 and bound == 2
    if name == "two-cliques-bridge-last":
        assert np.flatnonzero(want).tolist() == [149, 299]
    if name == "two-cliques-bridge-reversed":
        assert np.flatnonzero(want).tolist() == [0, 150]
    if name == "n2-edge-equal-keys":
        assert want.tolist() == [1, 0]                                                # equal keys: the smaller vertex first
    dev = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)).cuda()
    seen = set()
    for blocks, vblocks in hook_grid((0, 1, 2)):
        grid_hook(blocks, vblocks)
        first, rounds = greedy_raw(dev, n, keys)
        again, rounds_again = greedy_raw(dev, n, keys)
        assert first.dtype == np.uint8 and first.tobytes() == again.tobytes(), (name, blocks, vblocks)
        assert np.array_equal(first, want), (name, blocks, vblocks, np.flatnonzero(first != want)[:5])
        for r in (rounds, rounds_again):
            assert 1 <= r <= bound, (name, blocks, vblocks, r, bound)
        seen.add(rounds)
    print(f"{name}: rounds {sorted(seen)} of at most {bound}")
    grid_hook(0)
    got, _ = pkg.greedy_representatives(np.asarray(edges), n, keys)                   # a host list is copied to the device
    assert np.array_equal(got, want)
    on_dev, _ = pkg.greedy_representatives(dev, n, keys, to_host=False)
    assert on_dev.is_cuda and on_dev.dtype == torch.uint8 and np.array_equal(on_dev.cpu().numpy(), want)


@pytest.mark.parametrize("bad", [(-1, 5), (7, 100), (100, 7), (-3, 100), (1 << 30, -(1 << 31))])
def test_representatives_invalid_entry(grid_hook, bad):
    n = 100
    edges = sparse_random(n, 300, 5).astype(np.int32)
    edges[[17, 230]] = bad                                                         # two such entries
    lib = pkg.hip_lib()
    dev = torch.from_numpy(edges).cuda()
    keys = torch.from_numpy(random_keys(n, 2).view(np.int64)).cuda()
    for blocks, vblocks, key_ptr in ((0, 0, None), (1, 0, keys.data_ptr()), (0, 1, keys.data_ptr()), (0, 3, None), (1, 1, None)):
        grid_hook(blocks, vblocks)
        buf = torch.full((n + 2 * GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
        rounds = C.c_int64(-9)
        rc = lib.selhip_greedy_representatives(dev.data_ptr(), len(edges), n, key_ptr, buf.data_ptr() + GUARD, C.byref(rounds), None)
        msg = lib.selhip_last_error(None).decode()
        assert rc == -1 and rounds.value == -9, (rc, msg)
        assert "2 invalid entries" in msg and f"[0, {n})" in msg and ("entry 17 is one" in msg or "entry 230 is one" in msg), msg
        assert np.all(buf.cpu().numpy() == 0xAB)                                      # nothing written, the guards included
    grid_hook(0)
    # the same list without them is fine, and the guards stay
    edges[[17, 230]] = (0, 0)
    buf = torch.full((n + 2 * GUARD,), 0xAB, dtype=torch.uint8, device="cuda")
    assert lib.selhip_greedy_representatives(torch.from_numpy(edges).cuda().data_ptr(), len(edges), n, keys.data_ptr(), buf.data_ptr() + GUARD, None, None) == 0
    out = buf.cpu().numpy()
    assert np.all(out[:GUARD] == 0xAB) and np.all(out[GUARD + n:] == 0xAB)
    assert np.array_equal(out[GUARD:GUARD + n], GM.representatives(edges, n, random_keys(n, 2)).astype(np.uint8))
    with pytest.raises(SelhipError, match="invalid entries"):
        pkg.greedy_representatives(np.array([[0, 1], [1, n]]), n)
    with pytest.raises(SelhipError, match=r"outside \[0, 0\)"):
        pkg.greedy_representatives(np.array([[0, 0]]), 0)
    got, rounds = pkg.greedy_representatives(np.zeros((0, 2), dtype=np.int32), 0)
    assert len(got) == 0 and rounds == 0


# ---- the context entry: raw calls into guarded buffers ------------------------------------------------------------------------------------
def raw_greedy(sel, min_value, rule, priority=None, null=()):
    """selhip_ctx_cluster_greedy into six arrays with sentinel guards; the outputs named in `null` are passed as NULL.  Returns the dict
    the model returns (without the NULL ones) plus "rounds", after checking that nothing outside the written entries changed"""
    n = sel.n
    stride = n + 2 * GUARD
    buf = torch.full((5 * stride,), SENTINEL, dtype=torch.int32, device="cuda")
    val = torch.full((stride,), float(SENTINEL), dtype=torch.float64, device="cuda")
    ptr = {name: buf.data_ptr() + 4 * (j * stride + GUARD) for j, name in enumerate(INT_OUTPUTS)}
    ptr["values"] = val.data_ptr() + 8 * GUARD
    for name in null:
        ptr[name] = None
    out = pkg._lib.Greedy(ptr["rep_of"], ptr["values"], ptr["clusters"], ptr["degrees"], ptr["sizes"], ptr["representatives"])
    prio = None if priority is None else torch.from_numpy(np.asarray(priority, dtype=np.uint32).view(np.int32)).cuda()
    cnt = C.c_int64(-5)
    pkg._lib.check(sel._lib.selhip_ctx_cluster_greedy(sel._ctx, float(min_value), int(rule), None if prio is None else prio.data_ptr(), C.byref(out),
                                                      C.byref(cnt)), sel._ctx)
    c = cnt.value
    host = buf.cpu().numpy().reshape(5, stride)
    res = {"n_clusters": c, "rounds": sel.get_param("greedy_rounds_last")}
    for j, name in enumerate(INT_OUTPUTS):
        written = 0 if name in null else c if name in ("sizes", "representatives") else n
        assert np.all(host[j, :GUARD] == SENTINEL) and np.all(host[j, GUARD + written:] == SENTINEL), (name, null, c)
        if name not in null:
            res[name] = host[j, GUARD:GUARD + written].copy()
    hv = val.cpu().numpy()
    written = 0 if "values" in null else n
    assert np.all(hv[:GUARD] == SENTINEL) and np.all(hv[GUARD + written:] == SENTINEL), ("values", null)
    if "values" not in null:
        res["values"] = hv[GUARD:GUARD + n].copy()
    assert sel.get_param("greedy_clusters_last") == c
    return res


def assert_same(got, want, what=""):
    assert got["n_clusters"] == want["n_clusters"], (what, got["n_clusters"], want["n_clusters"])
    for name in INT_OUTPUTS:
        if name in got:
            assert got[name].dtype == np.int32 and np.array_equal(got[name], want[name]), (what, name)
    if "values" in got:
        assert got["values"].dtype == np.float64 and np.array_equal(got["values"].view(np.uint64), want["values"].view(np.uint64)), (what, "values")
    if "rounds" in got and "rounds_bound" in want:
        assert (got["rounds"] == 0) if want["rounds_bound"] == 0 else 1 <= got["rounds"] <= want["rounds_bound"], (what, got["rounds"], want["rounds_bound"])


def snapshot(sel):
    return sel.fetch().tobytes(), sel.stats(), sel.last_attempts(), sel.result_count(), sel.get_param("clusters_last")


def plant(n, m, edges, seed):
    """n rows of m random SuperMinHash buckets in which the genomes a and b of every (a, b, c) of `edges` share exactly c buckets and no
    other pair shares any: behind a smh_c pass under the SuperMinHash estimator the record of {a, b} has the value c / m exactly"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(1, 1 << 62, size=(n, m), dtype=np.uint64)
    used = np.zeros((n, m), dtype=bool)
    for a, b, c in edges:
        free = np.flatnonzero(~used[a] & ~used[b])[:c]
        assert len(free) == c and a != b, (a, b, c)
        rows[a, free] = rows[b, free] = rng.integers(1 << 62, 1 << 63, size=c, dtype=np.uint64)
        used[a, free] = used[b, free] = True
    return rows


def random_weighted(n, seed, levels=(4, 8, 8, 12, 16)):
    """a sparse random graph with about 1.5 edges per vertex, components of mixed size, and few value levels: ties everywhere"""
    rng = np.random.default_rng(seed)
    pairs = {tuple(sorted(p)) for p in rng.integers(0, n, size=(3 * n // 2, 2)).tolist() if p[0] != p[1]}
    return [(a, b, int(rng.choice(levels))) for a, b in sorted(pairs)]


def planted_pass(sel, n, m, edges, seed=1):
    sel.upload(zeros_hll(n), plant(n, m, edges, seed), V.spread_cards(n))
    configure(sel, c_min=1)
    rec = sel.run(-1.0, MODE_SMH, 7, 3)
    want = sorted((min(a, b), max(a, b), c / m) for a, b, c in edges)
    assert sorted(zip(rec["i"].tolist(), rec["k"].tolist(), rec["jaccard"].tolist())) == want      # the planted graph, values exactly c / m
    return rec


# ---- 2. behind smh_c -V smh passes on hand-built bucket rows: sizes around the wave and block edges, cuts, rules, NULL outputs -------------
def test_greedy_behind_planted_pass(grid_hook):
    m = 256
    n_mixed = 0
    with Selector(0) as sel:
        assert sel.get_param("greedy_clusters_last") == -1 and sel.get_param("greedy_rounds_last") == -1
        for n in (1, 2, 65, 129, 257):
            edges = random_weighted(n, 40 + n) if n > 2 else [(0, 1, 8)][:n - 1]
            rec = planted_pass(sel, n, m, edges, seed=n)
            before = snapshot(sel)
            prio = np.random.default_rng(n).integers(0, 4, size=n).astype(np.uint32)   # four levels: ties, broken by the smaller rank
            prio[n // 2] = 0xFFFFFFFF
            for min_value in (-np.inf, 8 / m, 12 / m):
                for rule, code in RULES.items():
                    p = prio if rule == "priority" else None
                    want = GM.clusters(rec, n, min_value, rule, p)
                    for blocks, vblocks in hook_grid((0, 1)):
                        grid_hook(blocks, vblocks)
                        assert_same(raw_greedy(sel, min_value, code, p), want, (n, min_value, rule, blocks, vblocks))
                    n_mixed += 1 < want["n_clusters"] < n
            grid_hook(0)
            # every output pointer NULL in turn: the others are still right, nothing else is written
            want = GM.clusters(rec, n, -np.inf, "max_degree")
            for name in OUTPUTS:
                assert_same(raw_greedy(sel, -np.inf, 0, null=(name,)), want, (n, "null", name))
            got = raw_greedy(sel, -np.inf, 0, null=OUTPUTS)
            assert got["n_clusters"] == want["n_clusters"] and set(got) == {"n_clusters", "rounds"}
            assert_same(raw_greedy(sel, -np.inf, 2, null=("degrees", "sizes", "values")), GM.clusters(rec, n, -np.inf, "max_rank"), (n, "no degree pass"))
            # the wrapper: numpy arrays, and tensors on the device
            assert_same(sel.cluster_greedy(), want, (n, "wrapper"))
            by_prio = sel.cluster_greedy(8 / m, priority=prio)
            assert_same(by_prio, GM.clusters(rec, n, 8 / m, "priority", prio), (n, "wrapper, priority"))
            dev = sel.cluster_greedy(to_host=False, order="max_rank")
            w_rank = GM.clusters(rec, n, -np.inf, "max_rank")
            assert all(dev[k].is_cuda for k in OUTPUTS) and dev["values"].dtype == torch.float64
            assert_same({k: (v.cpu().numpy() if k in OUTPUTS else v) for k, v in dev.items()}, w_rank, (n, "device tensors"))
            assert snapshot(sel) == before, n                                            # list, statistics, attempts, "clusters_last": as they were
        with pytest.raises(ValueError, match="priority"):
            sel.cluster_greedy(order="priority")
        with pytest.raises(ValueError, match="priority"):
            sel.cluster_greedy(order="max_rank", priority=prio)
        with pytest.raises(ValueError, match="order"):
            sel.cluster_greedy(order="degree")
    assert n_mixed > 0


def test_vertex_trips_of_the_context_call(grid_hook):
    """771 genomes = three blocks of 256 and three lanes: with the vertex kernels in one block every loop of selhip_ctx_cluster_greedy
    comes round four times and ends in a wave of three lanes; with three blocks it comes round twice.  Every output, each order rule
    and a caller's priority, two cuts; twice, byte-equal"""
    n, m = 771, 256
    with Selector(0) as sel:
        rec = planted_pass(sel, n, m, random_weighted(n, 771), seed=771)                 # a sparse random graph: clusters across the trips
        prio = np.random.default_rng(n).integers(0, 4, size=n).astype(np.uint32)         # four levels: ties, broken by the smaller rank
        prio[n - 1] = 0xFFFFFFFF
        for min_value in (-np.inf, 8 / m):
            for rule, code in RULES.items():
                p = prio if rule == "priority" else None
                want = GM.clusters(rec, n, min_value, rule, p)
                far = np.flatnonzero(np.arange(n) // 256 != want["rep_of"] // 256)       # members a trip or more away from their representative
                assert 1 < want["n_clusters"] < n and want["sizes"].max() > 2 and len(far) > 100, (rule, want["n_clusters"], len(far))
                for blocks, vblocks in hook_grid((0, 1)):
                    grid_hook(blocks, vblocks)
                    first, again = raw_greedy(sel, min_value, code, p), raw_greedy(sel, min_value, code, p)
                    assert all(first[k].tobytes() == again[k].tobytes() for k in OUTPUTS), (rule, blocks, vblocks)
                    assert_same(first, want, (min_value, rule, blocks, vblocks))
        grid_hook(0, 3)
        assert len(sel.run(2.0, MODE_SMH, 7, 3)) == 0                                   # no record: greedy_singletons_kernel, two trips
        assert_same(raw_greedy(sel, -np.inf, 0), GM.clusters(rec[:0], n), "empty list")


# ---- 3. the chain A - B - C with A - C below the cut ------------------------------------------------------------------------------------------
def test_chain():
    n, m = 8, 256
    a, b, c = 2, 5, 6
    with Selector(0) as sel:
        rec = planted_pass(sel, n, m, [(a, b, 100), (b, c, 110), (a, c, 10)])
        cut = 50 / m
        single = sel.cluster(cut)
        assert single["n_clusters"] == n - 2 and len({int(single["clusters"][g]) for g in (a, b, c)}) == 1     # single linkage: one cluster
        by_rank = sel.cluster_greedy(cut, order="max_rank")                              # C first, then B (its member), then A: apart from C
        assert_same(by_rank, GM.clusters(rec, n, cut, "max_rank"), "max_rank")
        assert by_rank["n_clusters"] == n - 1 and by_rank["rep_of"][[a, b, c]].tolist() == [a, c, c]
        assert by_rank["values"][[a, b, c]].tolist() == [1.0, 110 / m, 1.0]
        by_degree = sel.cluster_greedy(cut, order="max_degree")                          # B first: both others are its members
        assert_same(by_degree, GM.clusters(rec, n, cut, "max_degree"), "max_degree")
        assert by_degree["n_clusters"] == n - 2 and by_degree["rep_of"][[a, b, c]].tolist() == [b, b, b]
        prio = np.zeros(n, dtype=np.uint32)
        prio[b] = 9
        by_prio = sel.cluster_greedy(cut, priority=prio)
        assert by_prio["rep_of"][[a, b, c]].tolist() == [b, b, b] and by_prio["values"][[a, b, c]].tolist() == [100 / m, 1.0, 110 / m]
        assert sel.cluster_greedy(order="max_rank")["rep_of"][[a, b, c]].tolist() == [c, c, c]      # with A - C an edge, C takes both


# ---- 4. boundaries ---------------------------------------------------------------------------------------------------------------------------
def test_boundaries():
    n, m = 12, 256
    # 0 - 1 at 64 / m decides whether 0 is 1's member (max_rank: 1 first) or a representative of its own
    # 5 has two representatives, 7 and 9, at the same value: the smaller rank;  3 - 4 - 10: 3's best edge leads to 4, a member of 10
    edges = [(0, 1, 64), (5, 7, 32), (5, 9, 32), (3, 4, 128), (4, 10, 16), (3, 10, 8)]
    with Selector(0) as sel:
        rec = planted_pass(sel, n, m, edges)
        J = 64 / m
        above = float(np.nextafter(J, np.inf))
        keep, drop = raw_greedy(sel, J, 2), raw_greedy(sel, above, 2)
        assert_same(keep, GM.clusters(rec, n, J, "max_rank"), "J")
        assert_same(drop, GM.clusters(rec, n, above, "max_rank"), "nextafter(J)")
        assert 0 not in keep["representatives"] and keep["rep_of"][0] == 1 and keep["values"][0] == J
        assert 0 in drop["representatives"] and drop["n_clusters"] == keep["n_clusters"] + 1
        assert drop["degrees"][0] == 0 and keep["degrees"][0] == 1
        whole = raw_greedy(sel, -np.inf, 2)
        assert_same(whole, GM.clusters(rec, n, -np.inf, "max_rank"), "-inf")
        assert int(whole["degrees"].sum()) == 2 * len(rec)                               # -inf takes every record
        assert whole["representatives"].tolist() == [1, 2, 6, 7, 8, 9, 10, 11]
        assert whole["rep_of"][5] == 7 and whole["values"][5] == 32 / m                  # two representatives at one value: the smaller rank
        assert whole["rep_of"][[3, 4]].tolist() == [10, 10] and whole["values"][3] == 8 / m      # not along 3 - 4 at 128 / m: 4 is no representative
        alone = raw_greedy(sel, np.inf, 0)
        assert_same(alone, GM.clusters(rec, n, np.inf), "+inf")
        assert alone["n_clusters"] == n and np.array_equal(alone["rep_of"], np.arange(n)) and np.all(alone["values"] == 1.0) and alone["rounds"] == 1
        last = sel.get_param("greedy_clusters_last"), sel.get_param("greedy_rounds_last")
        with pytest.raises(SelhipError, match="NaN") as err:
            raw_greedy(sel, np.nan, 0)
        assert err.value.code == -1
        for code in (4, -1, 100):
            with pytest.raises(SelhipError, match="order_rule") as err:
                raw_greedy(sel, -np.inf, code)
            assert err.value.code == -1
        with pytest.raises(SelhipError, match="d_priority") as err:                       # the rule without scores
            raw_greedy(sel, -np.inf, 3)
        assert err.value.code == -1
        for code in (0, 1, 2):
            with pytest.raises(SelhipError, match="d_priority") as err:                   # scores without the rule
                raw_greedy(sel, -np.inf, code, priority=np.zeros(n, dtype=np.uint32))
            assert err.value.code == -1
        assert (sel.get_param("greedy_clusters_last"), sel.get_param("greedy_rounds_last")) == last
        with pytest.raises(SelhipError, match="rep_rule"):                                # the single-linkage entry still refuses the new rule
            pkg._lib.check(sel._lib.selhip_ctx_cluster(sel._ctx, 0.0, 3, C.byref(pkg._lib.Clusters()), None), sel._ctx)
        for v in (0.0, -0.0, 8 / m, 16 / m, 0.5, 1.0):
            for rule, code in list(RULES.items())[:3]:
                assert_same(raw_greedy(sel, v, code), GM.clusters(rec, n, v, rule), (v, rule))


# ---- 5. the kinds of list, the refusals, and what the call leaves alone ----------------------------------------------------------------------
@pytest.mark.parametrize("crit", ["smh_a", "none"])
def test_behind_other_criteria(oracle, crit):
    n, m = 129, 256
    hll, aux, cards = M.ranked(oracle, M.hll_pool(n), M.planted_groups(n, m, 77 + n))
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        sel.set_criterion(CRIT_SMH_A if crit == "smh_a" else CRIT_NONE)
        rec = sel.run(0.3, MODE_CB_SMH, *((2, 128) if crit == "smh_a" else (1, 1)))
        assert len(rec) > 0
        before = snapshot(sel)
        cut = float(np.median(rec["jaccard"]))
        for min_value in (-np.inf, cut):
            for rule, code in list(RULES.items())[:3]:
                assert_same(raw_greedy(sel, min_value, code), GM.clusters(rec, n, min_value, rule), (crit, min_value, rule))
        assert snapshot(sel) == before


def test_small_pass_default_context(oracle):
    """the one-launch small pass (the default of a context the suite does not configure) leaves a list like any other"""
    n, m = 129, 256
    hll, aux, cards = M.ranked(oracle, M.hll_pool(n), M.planted_groups(n, m, 5))
    with Selector(0) as sel:
        sel.set_param("small_pass", -1)
        sel.upload(hll, aux, cards)
        rec = sel.run(0.3, MODE_CB_SMH, 2, 128)
        assert sel.get_param("small_pass_used") == 1 and len(rec) > 0
        assert_same(raw_greedy(sel, -np.inf, 0), GM.clusters(rec, n), "small pass")


def test_list_kinds_and_state():
    n, m = 257, 128
    aux, cards = case(n, m)
    with Selector(0) as sel:
        sel.upload(zeros_hll(n), aux, cards)
        with pytest.raises(SelhipError, match="no result list") as err:              # before any pass
            raw_greedy(sel, -np.inf, 0)
        assert err.value.code == -5
        configure(sel, c_min=1)
        # the directed top-k list, one-shot and in row rounds: the two records of a mutual pair are one edge, and count twice in the degrees
        whole = sel.run(-1.0, MODE_SMH, 7, 3, top_k=0)
        for rounds in (0, 16):
            ranked = sel.run(-1.0, MODE_SMH, 7, 3, top_k=3, rounds=rounds)
            before = snapshot(sel), sel.fetch_ranked().tobytes()
            pairs = set(zip(ranked["i"].tolist(), ranked["k"].tolist()))
            assert any((k, i) in pairs for i, k in pairs)
            for rule, code in list(RULES.items())[:3]:
                assert_same(raw_greedy(sel, -np.inf, code), GM.clusters(ranked, n, -np.inf, rule), ("top-k", rounds, rule))
            cut = float(np.median(ranked["jaccard"]))
            assert_same(raw_greedy(sel, cut, 2), GM.clusters(ranked, n, cut, "max_rank"), ("top-k cut", rounds))
            assert (snapshot(sel), sel.fetch_ranked().tobytes()) == before
            assert sel.get_param("allpairs_topk") == 3 and sel.get_param("topk_rounds") == rounds
        sel.set_topk_rounds(0)
        sel.set_allpairs_topk(0)
        # a pair list with entries listed twice, in both directions
        lst = np.concatenate([np.stack([whole["k"], whole["i"]], axis=1)[:40], np.stack([whole["i"], whole["k"]], axis=1)[:3]]).astype(np.int32)
        rec = sel.run_pairs(lst, -1.0, MODE_SMH, 7, 3)
        assert len(rec) == 43
        want = GM.clusters(rec, n)
        assert_same(raw_greedy(sel, -np.inf, 0), want, "pair list")
        assert int(want["degrees"].sum()) == 86
        # a pass that selected nothing: n representatives, one launch, one round
        sel.timing(1)
        assert len(sel.run(2.0, MODE_SMH, 7, 3)) == 0
        empty = raw_greedy(sel, -np.inf, 0)
        assert_same(empty, GM.clusters(rec[:0], n), "empty list")
        assert empty["n_clusters"] == n and empty["rounds"] == 1 and np.all(empty["values"] == 1.0) and np.all(empty["degrees"] == 0)
        assert sel.kernel_ms("greedy") > 0
        # a query pass leaves a list in two index spaces
        sel.upload_queries(zeros_hll(5), aux[:5], cards[:5])
        assert len(sel.run_queries(-1.0, MODE_SMH, 7, 3)) > 0
        last = sel.get_param("greedy_clusters_last")
        with pytest.raises(SelhipError, match="query pass") as err:
            raw_greedy(sel, -np.inf, 0)
        assert err.value.code == -5 and sel.get_param("greedy_clusters_last") == last
        # between run_async and finish; it works after finish
        sel.run_async(-1.0, MODE_SMH, 7, 3)
        with pytest.raises(SelhipError, match="pending") as err:
            raw_greedy(sel, -np.inf, 0)
        assert err.value.code == -5
        sel.finish()
        rec = sel.fetch()
        assert M.tuples(rec) == M.tuples(whole)
        want = GM.clusters(rec, n)
        assert_same(raw_greedy(sel, -np.inf, 0), want, "after finish")
        # a matrix call and a cluster call in between change nothing, and the greedy call leaves "clusters_last" alone
        before = snapshot(sel)
        sel.matrix("smh_jaccard")
        single = sel.cluster()
        assert np.array_equal(single["labels"], CM.labels(CM.record_edges(rec), n))
        before = before[:4] + (single["n_clusters"],)
        assert_same(raw_greedy(sel, -np.inf, 0), want, "behind a matrix and a cluster call")
        assert snapshot(sel) == before
        assert np.array_equal(sel.cluster()["labels"], single["labels"])
        # timing: "greedy" per greedy call, the passes' and the cluster call's figures untouched
        sel.timing(1)
        sel.run(-1.0, MODE_SMH, 7, 3)
        sel.cluster()
        names = ("prep", "stage1", "total", "topk", "matrix", "matrix_smh", "hist", "select", "cluster")
        ms, launches = [sel.kernel_ms(k) for k in names], [sel.kernel_launches(k) for k in names]
        assert sel.kernel_ms("greedy") < 0
        raw_greedy(sel, -np.inf, 0)
        raw_greedy(sel, 0.5, 1)
        assert sel.kernel_ms("greedy") > 0 and sel.kernel_launches("greedy") == 1.0       # one timed scope per call, two calls
        assert [sel.kernel_ms(k) for k in names] == ms and [sel.kernel_launches(k) for k in names] == launches
        sel.timing(0)
        # an upload drops the list: SELHIP_E_STATE again
        sel.upload(zeros_hll(n), aux, cards)
        with pytest.raises(SelhipError) as err:
            raw_greedy(sel, -np.inf, 0)
        assert err.value.code == -5


# ---- 6. the front ends, on the influenza fixtures ------------------------------------------------------------------------------------------
def selection(args):
    out = subprocess.run([str(BIN / "selection")] + args, cwd=GOLDEN, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return out.stdout


NONE_ARGS = (["-h", "0.5", "-a", "512", "-c", "none", "-n"], dict(tau=0.5, aux_bytes=512, criterion="none", mode=MODE_SMH))
KNN_ARGS = (["-c", "none", "-n", "-h", "-1", "-K", "3"], dict(tau=-1.0, aux_bytes=256, criterion="none", mode=MODE_SMH, top_k=3))
CASES = {"none": NONE_ARGS + (None, "max_degree", False), "none-T-max_rank": NONE_ARGS + (0.9, "max_rank", False),
         "none-T-min_rank": NONE_ARGS + (0.95, "min_rank", False), "none-T-W": NONE_ARGS + (0.9, "priority", True),
         "knn": KNN_ARGS + (None, "max_degree", False), "knn-T-max_rank": KNN_ARGS + (0.9, "max_rank", False), "knn-W": KNN_ARGS + (None, "priority", True)}


@pytest.mark.parametrize("name", list(CASES))
def test_front_ends(monkeypatch, tmp_path, name):
    args, kw, level, order, scored = CASES[name]
    monkeypatch.chdir(GOLDEN)
    base = ["-l", "influenza_filelist.txt"] + args
    plain = selection(base)
    assert len(plain.splitlines()) > 0
    ds = pkg.load_dataset("influenza_filelist.txt", 0)
    n = len(ds.names)
    with Selector(0) as sel:
        sel.upload(ds.hll, np.zeros((n, 1), dtype=np.uint64), ds.cards)
        sel.set_criterion(CRIT_NONE)
        rec = sel.run(kw["tau"], kw["mode"], 1, 1, top_k=kw.get("top_k") or None)
    assert pkg.format_lines(ds.names, rec) == plain
    listed = (GOLDEN / "influenza_filelist.txt").read_text().split()
    f = tmp_path / "clusters.tsv"
    extra = ["-Z", "greedy"] + (["-T", repr(level)] if level is not None else [])
    by_line = by_rank = None
    if scored:
        by_line = np.random.default_rng(11).integers(0, 3, size=n).astype(np.uint32)     # three levels: ties; file-list order
        by_line[0] = 0xFFFFFFFF
        scores = tmp_path / "scores.tsv"
        lines = [f"{p}\t{int(s)}\n" for p, s in zip(listed, by_line)]
        scores.write_text("".join(lines[::-1]))                                          # any order of lines
        extra += ["-W", str(scores)]
        by_rank = by_line[np.asarray(ds.order)]
    elif order != "max_degree":
        extra += ["-Y", order]
    assert selection(base + ["-L", str(f)] + extra) == plain                          # stdout: byte for byte what it is without -L
    res = GM.clusters(rec, n, -np.inf if level is None else level, order, by_rank)
    want = GM.table(ds.names, ds.order, res)
    text = f.read_text()
    assert text == want, name
    assert [ln.split("\t")[0] for ln in text.splitlines()] == listed
    assert all(len(ln.split("\t")) == 6 for ln in text.splitlines())
    if name == "none-T-max_rank":
        assert 1 < res["n_clusters"] < n
    assert pkg.greedy_from_filelist("influenza_filelist.txt", cluster_min=level, order=order, priority=by_line, **kw) == want, name
    if name == "none":
        single = tmp_path / "single.tsv"
        assert selection(base + ["-L", str(single), "-Z", "single"]) == plain           # -Z single: the table of -L alone, five columns
        assert single.read_text() == CM.table(ds.names, ds.order, CM.clusters(CM.record_edges(rec), n))


def test_front_end_scores_refused(tmp_path):
    """-W is read and checked on the host: a bad file ends the run with a line naming -W and no table"""
    listed = (GOLDEN / "influenza_filelist.txt").read_text().split()
    good = [f"{p}\t{j}\n" for j, p in enumerate(listed)]
    f = tmp_path / "clusters.tsv"
    for bad in (good[:-1], good + [good[0]], good[:-1] + ["no_such_genome\t3\n"], good[:-1] + [listed[-1] + "\t-3\n"], good[:-1] + [listed[-1] + "\t4294967296\n"],
                good[:-1] + [listed[-1] + " 3\n"], good[:-1] + [listed[-1] + "\t\n"]):
        scores = tmp_path / "scores.tsv"
        scores.write_text("".join(bad))
        out = subprocess.run([str(BIN / "selection"), "-l", "influenza_filelist.txt"] + NONE_ARGS[0] + ["-L", str(f), "-Z", "greedy", "-W", str(scores)],
                             cwd=GOLDEN, capture_output=True, text=True)
        assert out.returncode == 5 and out.stdout == "" and "selection: -W:" in out.stderr and not f.exists(), (bad[-1], out)
