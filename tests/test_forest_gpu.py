"""The maximum spanning forest on the GPU (selhip_spanning_forest, selhip_ctx_spanning_forest).  Every output is
compared bit for bit with tests/forest_model.py -- Kruskal's visit in the BEFORE order, in Python -- run on the same edge list, or on the
records fetched from the pass; the rounds with the model of the synchronous Boruvka scheme.  The graphs of (1) are those that break a
concurrent union-find (tests/test_cluster_gpu.py): hook chains of 4 096, 65 536 picks aimed at one word, one giant component, a bridge
as the worst and as the best edge; each under four value sets, with the default grid and with the record kernels' grid forced to 1 and 2
blocks, twice, and the two runs must be byte-equal.  The record grids are crossed with the vertex kernels' grid ("vertex_blocks": sized
from n, 1 block, 3 blocks), so that the loops of the hook, flatten and emit kernels -- a ballot and a lane-ordered scatter at the end
of every trip -- come round up to 257 times; the round count must equal the model's under every grid."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import cluster_model as CM
import forest_model as FM
import smhc_model as M
from test_cluster_gpu import clique, hook_grid, path, sparse_random, star, with_noise
from test_smhv_gpu import case, configure, zeros_hll

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import CRIT_NONE, CRIT_SMH_A, MODE_CB_SMH, MODE_SMH, PAIR_DTYPE, SelhipError, Selector

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
GUARD = 64                     # 16-byte records / int32 words of sentinel on both sides of every output array
SENTINEL = -77


@pytest.fixture
def grid_hook():
    """sets the process-wide grids of the record kernels and of the vertex kernels (0 = automatic) and puts the defaults back"""
    with Selector(0) as sel:
        def set_hooks(blocks, vertex_blocks=0):
            sel.set_param("cluster_blocks", blocks)
            sel.set_param("vertex_blocks", vertex_blocks)
            assert (sel.get_param("cluster_blocks"), sel.get_param("vertex_blocks")) == (blocks, vertex_blocks)
        yield set_hooks
        set_hooks(0, 0)


# ---- 1. selhip_spanning_forest on graphs built to break a union-find, four value sets, every grid, twice --------------------------------
def graphs():
    p4097 = path(4097, "ascending")
    g = [("n1", 1, np.zeros((0, 2), dtype=np.int64)), ("n1-loop", 1, np.array([[0, 0]])),
         ("n2-apart", 2, np.zeros((0, 2), dtype=np.int64)), ("n2-edge", 2, np.array([[1, 0]])),
         ("n1000-apart", 1000, np.zeros((0, 2), dtype=np.int64)), ("path-4097", 4097, p4097),
         ("star-centre-highest", 65537, star(65537, 65536)), ("star-centre-0", 65537, star(65537, 0)),
         ("K300", 300, clique(0, 300)),
         ("two-cliques-bridge", 300, np.concatenate([clique(0, 150), clique(150, 300), np.array([[299, 0]])])),
         ("sparse-5000", 5000, sparse_random(5000, 2500, 11)),
         ("duplicates-and-loops", 5000, with_noise(sparse_random(5000, 2500, 12), 5000, 13))]
    for p_edges in (0, 63, 64, 65, 255, 256, 257):
        g.append((f"pairs-{p_edges}", 300, sparse_random(300, p_edges, 100 + p_edges)))
    return g


def value_sets(name, n, edges):
    """{set name: float64 [P] or None}: NULL, distinct values, three levels, and NaN / +-0.0 / negatives / +-inf mixed; the paths also
    with values ascending along them (one picking round) and the ruler 1 - ctz(i + 1) / 16 (12 picking rounds); the bridge of the two
    cliques as the worst and as the best edge"""
    p = len(edges)
    rng = np.random.default_rng(p + n)
    specials = np.array([np.nan, 0.0, -0.0, -1.5, -0.25, np.inf, -np.inf, 0.25, 1.0, 5e-324, -5e-324])
    sets = {"null": None, "distinct": rng.permutation(p) / max(p, 1), "levels": rng.integers(0, 3, size=p) / 4.0,
            "specials": specials[rng.integers(0, len(specials), size=p)]}
    if name == "path-4097":
        i = edges.min(axis=1)
        sets["ascending"] = i / n
        sets["ruler"] = 1.0 - np.array([((int(x) + 1) & -(int(x) + 1)).bit_length() - 1 for x in i]) / 16.0
    if name == "two-cliques-bridge":
        for which, v in (("bridge-worst", -1.0), ("bridge-best", 2.0)):
            vals = sets["distinct"].copy()
            vals[-1] = v
            sets[which] = vals
    return sets


GRAPHS = graphs()


def forest_raw(dev_pairs, dev_values, n):
    """selhip_spanning_forest into guarded buffers: (edges PAIR_DTYPE [F], labels, F, rounds)"""
    lib = pkg.hip_lib()
    cap = max(n - 1, 0)
    ebuf = torch.full(((cap + 2 * GUARD) * 4,), SENTINEL, dtype=torch.int32, device="cuda")
    lbuf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    f, rounds = C.c_int64(-5), C.c_int64(-5)
    rc = lib.selhip_spanning_forest(dev_pairs.data_ptr() if dev_pairs.numel() else None, None if dev_values is None else dev_values.data_ptr(),
                                    int(dev_pairs.shape[0]), n, ebuf.data_ptr() + 16 * GUARD, lbuf.data_ptr() + 4 * GUARD, C.byref(f), C.byref(rounds), None)
    assert rc == 0, lib.selhip_last_error(None).decode()
    e, lab = ebuf.cpu().numpy(), lbuf.cpu().numpy()
    assert 0 <= f.value <= cap
    assert np.all(e[:4 * GUARD] == SENTINEL) and np.all(e[4 * (GUARD + f.value):] == SENTINEL)           # entries from F on are not written
    assert np.all(lab[:GUARD] == SENTINEL) and np.all(lab[GUARD + n:] == SENTINEL)
    return e[4 * GUARD:4 * (GUARD + f.value)].copy().view(PAIR_DTYPE), lab[GUARD:GUARD + n].copy(), f.value, rounds.value


@pytest.mark.parametrize("name,n,edges", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_spanning_forest(grid_hook, name, n, edges):
    dev = torch.from_numpy(np.ascontiguousarray(edges, dtype=np.int32).reshape(-1, 2)).cuda()
    for vname, values in value_sets(name, n, edges).items():
        recs = FM.records_of(edges, values)
        k, lab = FM.kruskal(recs, n)
        b, comp, want_rounds = FM.boruvka_rounds(recs, n)
        assert k == b and lab == comp
        want = FM.as_records(k)
        want_lab = np.array(lab, dtype=np.int32)
        live = np.asarray(edges).reshape(-1, 2)[[x == x for _, _, x in recs]] if len(recs) else np.zeros((0, 2), dtype=np.int64)
        assert np.array_equal(want_lab, CM.labels(live, n))
        if vname == "ascending":
            assert want_rounds == 2 and len(k) == n - 1
        if vname == "ruler":
            assert want_rounds == 13
        if vname == "bridge-worst":
            assert (k[-1][0], k[-1][1]) == (0, 299) and len(k) == 299
        if vname == "bridge-best":
            assert (k[0][0], k[0][1]) == (0, 299) and len(k) == 299
        if name.startswith("star") and vname == "null":
            assert len(k) == 65536 and want_rounds == 2
        dvals = None if values is None else torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).cuda()
        for blocks, vblocks in hook_grid((0, 1, 2)):
            grid_hook(blocks, vblocks)
            first = forest_raw(dev, dvals, n)
            again = forest_raw(dev, dvals, n)
            assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and first[2:] == again[2:], (name, vname, blocks, vblocks)
            got, got_lab, f, rounds = first
            assert f == len(k) and got.tobytes() == want.tobytes(), (name, vname, blocks, vblocks, f, len(k))
            assert np.array_equal(got_lab, want_lab), (name, vname, blocks, vblocks)
            assert rounds == want_rounds, (name, vname, blocks, vblocks, rounds, want_rounds)
        grid_hook(0)
    # the wrapper: a host list is copied to the device; tensors on the device
    values = value_sets(name, n, edges)["levels"]
    k, lab = FM.kruskal(FM.records_of(edges, values), n)
    res = pkg.spanning_forest(np.asarray(edges), n, values)
    assert res["edges"].dtype == PAIR_DTYPE and res["edges"].tobytes() == FM.as_records(k).tobytes() and res["labels"].tolist() == lab
    assert res["n_edges"] == len(k) and res["n_clusters"] == n - len(k) == len(set(lab)) and res["rounds"] >= 1
    on_dev = pkg.spanning_forest(dev, n, to_host=False)
    assert on_dev["edges"].is_cuda and on_dev["edges"].shape == (on_dev["n_edges"], 16) and on_dev["labels"].is_cuda


# ---- 2. invalid entries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [(-1, 5), (7, 100), (100, 7), (-3, 100), (1 << 30, -(1 << 31))])
def test_spanning_forest_invalid_entry(grid_hook, bad):
    n = 100
    edges = sparse_random(n, 300, 5).astype(np.int32)
    edges[[17, 230]] = bad                                                         # two such entries
    values = np.random.default_rng(9).random(300)
    values[17] = np.nan                                                            # whatever its value
    lib = pkg.hip_lib()
    dev, dvals = torch.from_numpy(edges).cuda(), torch.from_numpy(values).cuda()
    for blocks, vblocks in hook_grid((0, 1)):
        grid_hook(blocks, vblocks)
        for vals in (dvals, None):
            ebuf = torch.full(((n - 1 + 2 * GUARD) * 4,), SENTINEL, dtype=torch.int32, device="cuda")
            lbuf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
            f, rounds = C.c_int64(-5), C.c_int64(-5)
            rc = lib.selhip_spanning_forest(dev.data_ptr(), None if vals is None else vals.data_ptr(), len(edges), n, ebuf.data_ptr() + 16 * GUARD,
                                            lbuf.data_ptr() + 4 * GUARD, C.byref(f), C.byref(rounds), None)
            msg = lib.selhip_last_error(None).decode()
            assert rc == -1, (rc, msg)
            assert "2 invalid entries" in msg and f"[0, {n})" in msg and ("entry 17 is one" in msg or "entry 230 is one" in msg), msg
            assert np.all(ebuf.cpu().numpy() == SENTINEL) and np.all(lbuf.cpu().numpy() == SENTINEL)     # nothing is written
            assert (f.value, rounds.value) == (-5, -5)
    grid_hook(0)
    # the same list without them is fine
    edges[[17, 230]] = (0, 0)
    got, lab, f, rounds = forest_raw(torch.from_numpy(edges).cuda(), dvals, n)
    k, want_lab = FM.kruskal(FM.records_of(edges, values), n)
    assert got.tobytes() == FM.as_records(k).tobytes() and lab.tolist() == want_lab
    with pytest.raises(SelhipError, match="invalid entries"):
        pkg.spanning_forest(np.array([[0, 1], [1, n]]), n)
    with pytest.raises(SelhipError, match=r"outside \[0, 0\)"):
        pkg.spanning_forest(np.array([[0, 0]]), 0)
    empty = pkg.spanning_forest(np.zeros((0, 2), dtype=np.int32), 0)
    assert len(empty["edges"]) == 0 and len(empty["labels"]) == 0 and empty["rounds"] == 0


# ---- 3. the context entry: raw calls into guarded buffers ------------------------------------------------------------------------------------
def raw_forest(sel, min_value, null=()):
    """selhip_ctx_spanning_forest into guarded arrays; the outputs named in `null` are passed as NULL"""
    n = sel.n
    cap = max(n - 1, 0)
    ebuf = torch.full(((cap + 2 * GUARD) * 4,), SENTINEL, dtype=torch.int32, device="cuda")
    lbuf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    out = pkg._lib.Forest(None if "edges" in null else ebuf.data_ptr() + 16 * GUARD, None if "labels" in null else lbuf.data_ptr() + 4 * GUARD)
    cnt = C.c_int64(-5)
    others = [sel.get_param(k) for k in ("clusters_last", "greedy_clusters_last", "greedy_rounds_last")]
    pkg._lib.check(sel._lib.selhip_ctx_spanning_forest(sel._ctx, float(min_value), C.byref(out), C.byref(cnt)), sel._ctx)
    assert [sel.get_param(k) for k in ("clusters_last", "greedy_clusters_last", "greedy_rounds_last")] == others
    f = cnt.value
    e, lab = ebuf.cpu().numpy(), lbuf.cpu().numpy()
    fw, lw = (0 if "edges" in null else f), (0 if "labels" in null else n)
    assert np.all(e[:4 * GUARD] == SENTINEL) and np.all(e[4 * (GUARD + fw):] == SENTINEL), (null, f)
    assert np.all(lab[:GUARD] == SENTINEL) and np.all(lab[GUARD + lw:] == SENTINEL), (null, f)
    assert sel.get_param("forest_edges_last") == f and sel.get_param("forest_rounds_last") >= (1 if n else 0)
    return {"edges": e[4 * GUARD:4 * (GUARD + fw)].copy().view(PAIR_DTYPE), "labels": lab[GUARD:GUARD + lw].copy(), "n_edges": f,
            "rounds": sel.get_param("forest_rounds_last")}


def snapshot(sel):
    return (sel.fetch().tobytes(), sel.stats(), sel.last_attempts(), sel.result_count(), sel.get_param("clusters_last"),
            sel.get_param("greedy_clusters_last"), sel.get_param("greedy_rounds_last"), sel.get_param("allpairs_topk"), sel.get_param("topk_rounds"))


def check_list(sel, rec, cuts, grid_hook, what, every_value=True):
    """the forest of the list the context holds against the model on the records `rec`, at every cut; forest_cut against Selector.cluster"""
    n = sel.n
    recs = FM.records_of_pass(rec)
    before = snapshot(sel)
    for min_value in cuts:
        k, lab = FM.kruskal(recs, n, min_value)
        b, comp, want_rounds = FM.boruvka_rounds(recs, n, min_value)
        assert k == b
        for blocks, vblocks in hook_grid((0, 1)):
            grid_hook(blocks, vblocks)
            got = raw_forest(sel, min_value)
            assert got["n_edges"] == len(k) and got["edges"].tobytes() == FM.as_records(k).tobytes(), (what, min_value, blocks, vblocks)
            assert got["labels"].tolist() == lab and got["rounds"] == want_rounds, (what, min_value, blocks, vblocks, got["rounds"], want_rounds)
        grid_hook(0)
        clu = sel.cluster(min_value)
        assert np.array_equal(got["labels"], clu["labels"]) and got["n_edges"] == n - clu["n_clusters"], (what, min_value)
    # NULL members in turn
    k, lab = FM.kruskal(recs, n)
    only_edges, only_labels, neither = raw_forest(sel, -np.inf, null=("labels",)), raw_forest(sel, -np.inf, null=("edges",)), raw_forest(sel, -np.inf, null=("edges", "labels"))
    assert only_edges["edges"].tobytes() == FM.as_records(k).tobytes() and only_labels["labels"].tolist() == lab
    assert only_edges["n_edges"] == only_labels["n_edges"] == neither["n_edges"] == len(k)
    # the wrapper, and the cuts of the one forest against a cluster call each
    res = sel.spanning_forest()
    assert res["edges"].tobytes() == FM.as_records(k).tobytes() and res["labels"].tolist() == lab
    assert res["n_edges"] == len(k) and res["n_clusters"] == n - len(k) and res["rounds"] == only_edges["rounds"]
    dev = sel.spanning_forest(to_host=False)
    assert dev["edges"].is_cuda and dev["edges"].cpu().numpy().tobytes() == res["edges"].tobytes() and dev["labels"].cpu().numpy().tolist() == lab
    levels = np.unique(rec["jaccard"]) if every_value else np.unique(np.concatenate([res["edges"]["jaccard"], np.unique(rec["jaccard"])[::97]]))
    counts = pkg.forest_cluster_counts(res["edges"], n, levels)
    for t, c in zip(levels, counts):
        clu = sel.cluster(min_value=float(t))
        assert np.array_equal(pkg.forest_cut(res["edges"], n, float(t)), clu["labels"]) and c == clu["n_clusters"], (what, t)
    after = snapshot(sel)
    assert after[:4] == before[:4] and after[5:] == before[5:], what                    # (clusters_last is selhip_ctx_cluster's to change)
    return len(k)


def test_forest_behind_all_pairs(oracle, grid_hook):
    n, m = 300, 256
    hll, aux, cards = M.ranked(oracle, M.hll_pool(n), M.planted_groups(n, m, 77 + n))
    with Selector(0) as sel:
        assert sel.get_param("forest_rounds_last") == -1 and sel.get_param("forest_edges_last") == -1
        sel.upload(hll, aux, cards)
        sel.set_criterion(CRIT_SMH_A)
        rec = sel.run(0.3, MODE_CB_SMH, 2, 128)
        values = np.unique(rec["jaccard"])
        assert 0 < check_list(sel, rec, [-np.inf, float(values[len(values) // 2])], grid_hook, "smh_a") < n - 1
        sel.set_criterion(CRIT_NONE)
        rec = sel.run(0.05, MODE_SMH, 1, 1)
        values = np.unique(rec["jaccard"])
        cuts = [-np.inf, float(values[len(values) // 4]), float(values[len(values) // 2]), float(values[-1]), float(np.nextafter(values[-1], np.inf))]
        assert check_list(sel, rec, cuts, grid_hook, "none", every_value=False) > 0


def test_forest_list_kinds_and_state(grid_hook):
    n, m = 300, 128
    aux, cards = case(n, m)
    with Selector(0) as sel:
        sel.upload(zeros_hll(n), aux, cards)
        with pytest.raises(SelhipError, match="no result list") as err:              # before any pass
            raw_forest(sel, -np.inf)
        assert err.value.code == -5
        configure(sel, c_min=1)
        whole = sel.run(-1.0, MODE_SMH, 7, 3, top_k=0)
        # the directed top-k list, one-shot and in row rounds: the two records of a mutual pair are one edge
        for rounds in (0, 16):
            ranked = sel.run(-1.0, MODE_SMH, 7, 3, top_k=3, rounds=rounds)
            pairs = set(zip(ranked["i"].tolist(), ranked["k"].tolist()))
            assert any((k, i) in pairs for i, k in pairs)
            kept = sel.fetch_ranked().tobytes()
            check_list(sel, ranked, [-np.inf, float(np.median(ranked["jaccard"]))], grid_hook, ("top-k", rounds))
            assert sel.fetch_ranked().tobytes() == kept
        sel.set_topk_rounds(0)
        sel.set_allpairs_topk(0)
        # a pair list with entries listed twice
        lst = np.concatenate([np.stack([whole["k"], whole["i"]], axis=1)[:40], np.stack([whole["i"], whole["k"]], axis=1)[:3]]).astype(np.int32)
        rec = sel.run_pairs(lst, -1.0, MODE_SMH, 7, 3)
        assert len(rec) == 43
        assert check_list(sel, rec, [-np.inf], grid_hook, "pair list") <= 40
        # argument refusals change nothing
        last = sel.get_param("forest_edges_last"), sel.get_param("forest_rounds_last")
        with pytest.raises(SelhipError, match="NaN") as err:
            raw_forest(sel, np.nan)
        assert err.value.code == -1
        assert sel._lib.selhip_ctx_spanning_forest(sel._ctx, 0.5, None, None) == -1 and "null selhip_forest_t" in sel._lib.selhip_last_error(sel._ctx).decode()
        buf = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
        out = pkg._lib.Forest(buf.data_ptr() + 8, None)
        assert sel._lib.selhip_ctx_spanning_forest(sel._ctx, 0.5, C.byref(out), None) == -1 and "16-byte aligned" in sel._lib.selhip_last_error(sel._ctx).decode()
        assert (sel.get_param("forest_edges_last"), sel.get_param("forest_rounds_last")) == last
        # a pass that selected nothing: the identity labels, no edge, one round
        sel.timing(1)
        assert len(sel.run(2.0, MODE_SMH, 7, 3)) == 0
        assert sel.kernel_ms("forest") < 0
        empty = raw_forest(sel, -np.inf)
        assert empty["n_edges"] == 0 and empty["rounds"] == 1 and np.array_equal(empty["labels"], np.arange(n))
        assert sel.kernel_ms("forest") > 0 and sel.kernel_launches("forest") == 1.0
        # timing: "forest" per forest call, the passes' figures untouched
        sel.timing(1)
        sel.run(-1.0, MODE_SMH, 7, 3)
        names = ("prep", "stage1", "total", "topk", "matrix", "cluster", "greedy", "merge", "hist", "select")
        ms, launches = [sel.kernel_ms(k) for k in names], [sel.kernel_launches(k) for k in names]
        assert sel.kernel_ms("forest") < 0
        raw_forest(sel, -np.inf)
        raw_forest(sel, 0.5)
        assert sel.kernel_ms("forest") > 0 and sel.kernel_launches("forest") == 1.0      # one timed scope per call, two calls
        assert [sel.kernel_ms(k) for k in names] == ms and [sel.kernel_launches(k) for k in names] == launches
        sel.timing(0)
        # a query pass leaves a list in two index spaces
        sel.upload_queries(zeros_hll(5), aux[:5], cards[:5])
        assert len(sel.run_queries(-1.0, MODE_SMH, 7, 3)) > 0
        with pytest.raises(SelhipError, match="query pass") as err:
            raw_forest(sel, -np.inf)
        assert err.value.code == -5
        # between run_async and finish; it works after finish
        sel.run_async(-1.0, MODE_SMH, 7, 3)
        with pytest.raises(SelhipError, match="pending") as err:
            raw_forest(sel, -np.inf)
        assert err.value.code == -5
        sel.finish()
        rec = sel.fetch()
        k, lab = FM.kruskal(FM.records_of_pass(rec), n)
        got = raw_forest(sel, -np.inf)
        assert got["edges"].tobytes() == FM.as_records(k).tobytes() and got["labels"].tolist() == lab
        # an upload drops the list; an empty set writes nothing
        sel.upload(zeros_hll(n), aux, cards)
        with pytest.raises(SelhipError) as err:
            raw_forest(sel, -np.inf)
        assert err.value.code == -5
        sel.upload(zeros_hll(0), aux[:0], cards[:0])
        assert len(sel.run(-1.0, MODE_SMH, 7, 3)) == 0
        none = raw_forest(sel, -np.inf)
        assert none["n_edges"] == 0 and none["rounds"] == 0 and len(none["labels"]) == 0
        res = sel.spanning_forest()
        assert res["n_edges"] == 0 and res["n_clusters"] == 0 and len(res["edges"]) == 0


# ---- 4. the front ends, on the influenza fixtures ------------------------------------------------------------------------------------------
def selection(args):
    out = subprocess.run([str(BIN / "selection")] + args, cwd=GOLDEN, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return out.stdout


CASES = {"smh_a": (["-h", "0.9", "-a", "512"], dict(tau=0.9, aux_bytes=512), None),
         "smh_a-T0.95": (["-h", "0.9", "-a", "512"], dict(tau=0.9, aux_bytes=512), 0.95),
         "none-T": (["-h", "0.5", "-a", "512", "-c", "none", "-n"], dict(tau=0.5, aux_bytes=512, criterion="none", mode=MODE_SMH), 0.9),
         "knn": (["-c", "none", "-n", "-h", "-1", "-K", "3"], dict(tau=-1.0, aux_bytes=256, criterion="none", mode=MODE_SMH, top_k=3), None)}


@pytest.mark.parametrize("name", list(CASES))
def test_front_ends(monkeypatch, tmp_path, name):
    args, kw, level = CASES[name]
    monkeypatch.chdir(GOLDEN)
    base = ["-l", "influenza_filelist.txt"] + args
    plain = selection(base)
    assert len(plain.splitlines()) > 0
    m = kw["aux_bytes"] // 8 if kw.get("criterion", "smh_a") == "smh_a" else 0
    ds = pkg.load_dataset("influenza_filelist.txt", m)
    n = len(ds.names)
    with Selector(0) as sel:
        sel.upload(ds.hll, ds.aux if m else np.zeros((n, 1), dtype=np.uint64), ds.cards)
        sel.set_criterion(CRIT_SMH_A if m else CRIT_NONE)
        rec = sel.run(kw["tau"], kw.get("mode", MODE_CB_SMH), *(pkg.banding(m, kw["tau"]) if m else (1, 1)), top_k=kw.get("top_k") or None)
    assert pkg.format_lines(ds.names, rec) == plain
    k, _ = FM.kruskal(FM.records_of_pass(rec), n, -np.inf if level is None else level)
    want = pkg.forest_table(ds.names, FM.as_records(k))
    assert len(k) > 0 and want.count("\n") == len(k)
    f, g = tmp_path / "forest.tsv", tmp_path / "clusters.tsv"
    extra = ["-T", repr(level)] if level is not None else []
    assert selection(base + ["-H", str(f)] + extra) == plain                          # stdout: byte for byte what it is without -H
    assert f.read_text() == want, name
    f.unlink()
    assert selection(base + ["-H", str(f), "-L", str(g)] + extra) == plain            # beside -L: one -T serves both
    assert f.read_text() == want, name
    assert g.read_text() == CM.table(ds.names, ds.order, CM.clusters(CM.record_edges(rec, -np.inf if level is None else level), n, "max_degree"))
    assert pkg.forest_from_filelist("influenza_filelist.txt", cluster_min=level, **kw) == want, name
