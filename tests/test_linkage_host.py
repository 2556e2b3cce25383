"""The dense-matrix hierarchy without a device (include/selection_hip.h section 2k): the sequential model tests/linkage_model.py --
which defines every output of selhip_linkage bit for bit -- against scipy.cluster.hierarchy.linkage, its rescan branch, its shape
edges, the host helpers of the package, the argument checks and the command line's refusals."""
import subprocess

import numpy as np
import pytest
from scipy.cluster.hierarchy import fcluster, is_valid_linkage
from scipy.cluster.hierarchy import linkage as scipy_linkage
from scipy.spatial.distance import squareform

from conftest import ROOT
import linkage_model as LM

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import PAIR_DTYPE

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
METHODS = ("single", "complete", "average", "weighted")
N = 300


def symmetric(upper):
    d = np.triu(upper, 1)
    return d + d.T


def inputs():
    """tie-free inputs: a random symmetric matrix, points in 8-D, clusters of 10 with noise"""
    rng = np.random.default_rng(20261021)
    out = {"random": symmetric(rng.random((N, N)))}
    pts = rng.random((N, 8))
    out["points"] = np.sqrt(((pts[:, None, :] - pts[None, :, :]) ** 2).sum(axis=2))
    centres = np.repeat(rng.random((N // 10, 8)) * 10.0, 10, axis=0) + 0.05 * rng.standard_normal((N, 8))
    out["clusters"] = symmetric(np.sqrt(((centres[:, None, :] - centres[None, :, :]) ** 2).sum(axis=2)))
    out["points"] = symmetric(out["points"])
    return out


INPUTS = inputs()


def scipy_members(Z, n):
    held = {g: frozenset([g]) for g in range(n)}
    for s, row in enumerate(Z):
        held[n + s] = held[int(row[0])] | held[int(row[1])]
    return [held[n + s] for s in range(len(Z))]


# ---- 1. the model against SciPy ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", list(INPUTS))
def test_model_equals_scipy(name, method):
    """the merged member sets are SciPy's; the sorted heights agree within 4 n 2^-53 relative -- a Lance-Williams step is a convex
    combination with at most four roundings and the tree is at most n - 1 deep --, bit for bit for single and complete linkage.  The
    comparison of the topologies means something because SciPy's consecutive heights lie further apart than that bound"""
    dist = INPUTS[name]
    bound = 4 * N * 2.0 ** -53
    Z = scipy_linkage(squareform(dist, checks=False), method)
    zh = Z[:, 2]
    assert np.all(np.diff(zh) > 2 * bound * zh[1:]), (name, method, float(np.min(np.diff(zh) / zh[1:])))
    got = LM.linkage_model(dist, method)
    assert got["n_merges"] == N - 1 and got["rescans"] == 0
    assert set(LM.members_of(got["merges"], N)) == set(scipy_members(Z, N))
    assert got["sizes"].tolist() == [len(s) for s in LM.members_of(got["merges"], N)]
    h = np.sort(got["merges"]["jaccard"])
    print(name, method, "rounds", got["rounds"], "row scans", got["rowscans"], "max relative height difference", float(np.max(np.abs(h - zh) / zh)))
    if method in ("single", "complete"):
        assert np.array_equal(h.view(np.uint64), zh.view(np.uint64))
    else:
        assert np.all(np.abs(h - zh) <= bound * zh)
    # every merge's height belongs to its member set, not only the sorted lists
    by_set = dict(zip(scipy_members(Z, N), zh))
    for s, e in zip(LM.members_of(got["merges"], N), got["merges"]):
        assert abs(float(e["jaccard"]) - by_set[s]) <= bound * by_set[s]
    # children before parents, ascending a within a round, a < b, the cluster lives in its smallest member
    assert np.all(got["merges"]["i"] < got["merges"]["k"])
    assert all(min(s) == int(e["i"]) for s, e in zip(LM.members_of(got["merges"], N), got["merges"]))
    assert got["rounds"] < N and got["rowscans"] < (40 if method == "single" else 8) * N
    assert sum(got["pairs_per_round"]) == N - 1 and got["pairs_per_round"][-1] == 0


# ---- 2. the rescan branch ------------------------------------------------------------------------------------------------------------------
def three_levels(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(8, 48))
    return rng.choice([0.25, 0.5, 0.75], size=(n, n))


def test_rescan_rounds():
    """matrices of three levels under single linkage: some reach a round without a pair in which not every row was scanned"""
    reached = [seed for seed in range(300) if LM.linkage_model(three_levels(seed), "single")["rescans"] > 0]
    assert len(reached) >= 3 and reached[:3] == [4, 36, 48], reached
    for seed in reached:
        dist = symmetric(three_levels(seed))
        n = dist.shape[0]
        got = LM.linkage_model(dist, "single")
        assert got["rescans"] > 0 and got["n_merges"] == n - 1 and got["rounds"] <= 2 * (n - 1) + 1
        Z = scipy_linkage(squareform(dist, checks=False), "single")
        assert np.array_equal(np.sort(got["merges"]["jaccard"]), Z[:, 2])               # (ties: the heights, not the topology, are unique)


# ---- 3. shape edges ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_shape_edges(method):
    # no slot, one slot
    for n, rounds in ((0, 0), (1, 1)):
        got = LM.linkage_model(np.zeros((n, n)), method)
        assert (got["n_merges"], got["rounds"], got["rowscans"]) == (0, rounds, n)
    # all equal: n - 1 merging rounds of one pair, (0, 1), (0, 2), ...
    n = 40
    got = LM.linkage_model(np.full((n, n), 0.5), method)
    assert got["rounds"] == n and got["pairs_per_round"] == [1] * (n - 1) + [0]
    assert got["merges"]["i"].tolist() == [0] * (n - 1) and got["merges"]["k"].tolist() == list(range(1, n))
    assert got["sizes"].tolist() == list(range(2, n + 1)) and np.all(got["merges"]["jaccard"] == 0.5)
    # the chain p_i = sum 1.5^j: the gaps grow, so single linkage takes one point per round; the tree is SciPy's under every method
    p = np.cumsum(1.5 ** np.arange(n))
    dist = np.abs(p[:, None] - p[None, :])
    got = LM.linkage_model(dist, method)
    assert got["n_merges"] == n - 1 and got["rounds"] <= n and got["rescans"] == 0 and got["rowscans"] <= 4 * n
    if method == "single":
        assert got["merges"]["i"].tolist() == [0] * (n - 1) and got["merges"]["k"].tolist() == list(range(1, n))
        assert got["sizes"].tolist() == list(range(2, n + 1)) and got["rounds"] == n
    Z = scipy_linkage(squareform(dist, checks=False), method)
    assert set(LM.members_of(got["merges"], n)) == set(scipy_members(Z, n))
    assert np.allclose(np.sort(got["merges"]["jaccard"]), Z[:, 2], rtol=4 * n * 2.0 ** -53, atol=0)
    # n / 2 well separated pairs: one round of n / 2 pairs, then the rule for two merged clusters
    rng = np.random.default_rng(5)
    left = np.cumsum(100.0 + 50.0 * rng.random(n // 2))
    p = np.stack([left, left + 0.5 + 0.4 * rng.random(n // 2)], axis=1).reshape(-1)
    dist = np.abs(p[:, None] - p[None, :])
    got = LM.linkage_model(dist, method)
    assert got["pairs_per_round"][0] == n // 2 and got["merges"]["i"][:n // 2].tolist() == list(range(0, n, 2))
    assert got["sizes"][:n // 2].tolist() == [2] * (n // 2) and got["n_merges"] == n - 1
    Z = scipy_linkage(squareform(dist, checks=False), method)
    assert set(LM.members_of(got["merges"], n)) == set(scipy_members(Z, n))
    assert np.allclose(np.sort(got["merges"]["jaccard"]), Z[:, 2], rtol=4 * n * 2.0 ** -53, atol=0)
    # a cap
    h = np.sort(got["merges"]["jaccard"])
    capped = LM.linkage_model(dist, method, float(h[n // 2 - 1]))
    assert capped["n_merges"] == n // 2 and capped["merges"].tobytes() == got["merges"][:n // 2].tobytes()
    with pytest.raises(LM.BadCells, match=r"2 cells .* cell \(1, 3\)"):
        bad = dist.copy()
        bad[1, 3] = np.nan
        bad[2, 5] = -np.inf
        bad[3, 1] = np.nan                                         # (below the diagonal: not read)
        LM.linkage_model(bad, method)


def test_zero_signs_and_infinity():
    """-0.0 against +0.0 goes to the smaller slot; +inf is data and merges last"""
    dist = symmetric(np.array([[0, 1.0, 0.0, np.inf], [0, 0, -0.0, np.inf], [0, 0, 0, np.inf], [0, 0, 0, 0]]))
    got = LM.linkage_model(dist, "average")
    assert got["merges"]["i"].tolist() == [0, 0, 0] and got["merges"]["k"].tolist() == [2, 1, 3]
    assert got["merges"]["jaccard"].tolist() == [0.0, 0.5, np.inf] and not np.isnan(got["merges"]["jaccard"]).any()


# ---- 4. the helpers of the package -------------------------------------------------------------------------------------------------------------
def as_records(rows):
    out = np.zeros(len(rows), dtype=PAIR_DTYPE)
    for j, row in enumerate(rows):
        out[j] = row
    return out


def test_linkage_matrix_and_cut():
    for name, dist in INPUTS.items():
        for method in METHODS:
            got = LM.linkage_model(dist, method)
            Z = pkg.linkage_matrix(got["merges"], got["sizes"], N)
            assert Z.shape == (N - 1, 4) and is_valid_linkage(Z)
            assert np.array_equal(np.sort(Z[:, 2]), np.sort(got["merges"]["jaccard"])) and Z[-1, 3] == N
            assert set(scipy_members(Z, N)) == set(LM.members_of(got["merges"], N))
            h = np.sort(got["merges"]["jaccard"])
            for t in (float(h[5]), float((h[100] + h[101]) / 2), float(h[-1])):
                keep = got["merges"][got["merges"]["jaccard"] <= t]            # what linkage_cut hands to `components`
                mine, theirs = LM.labels_of(keep, N), fcluster(Z, t, criterion="distance")
                assert len(set(zip(mine.tolist(), theirs.tolist()))) == len(set(mine.tolist())) == len(set(theirs.tolist())), (name, method, t)
    # a parent an ulp below its child keeps its place behind the child
    merges = as_records([(0, 1, 0.5), (2, 3, 0.25), (0, 2, np.nextafter(0.5, 0))])
    Z = pkg.linkage_matrix(merges, [2, 2, 4], 4)
    assert Z.tolist() == [[2.0, 3.0, 0.25, 2.0], [0.0, 1.0, 0.5, 2.0], [4.0, 5.0, np.nextafter(0.5, 0), 4.0]] and is_valid_linkage(Z)
    # a capped hierarchy: fill joins the remaining roots in ascending slot order
    with pytest.raises(ValueError, match="3 roots"):
        pkg.linkage_matrix(merges[:1], [2], 4)
    Z = pkg.linkage_matrix(merges[:1], [2], 4, fill=9.0)
    assert Z.tolist() == [[0.0, 1.0, 0.5, 2.0], [2.0, 4.0, 9.0, 3.0], [3.0, 5.0, 9.0, 4.0]] and is_valid_linkage(Z)
    assert pkg.linkage_matrix(as_records([]), [], 1).shape == (0, 4)


def test_newick_by_hand():
    merges = as_records([(0, 1, 0.2), (2, 3, 0.4), (0, 2, 1.0)])
    assert pkg.linkage_newick(merges, [2, 2, 4], ["A", "B", "C", "D"]) == "((A:0.1,B:0.1):0.4,(C:0.2,D:0.2):0.3);\n"
    # a parent below its child: no negative branch; names that need quotes
    merges = as_records([(0, 1, 0.5), (0, 2, 0.25)])
    assert pkg.linkage_newick(merges, [2, 3], ["a b", "it's", "x/y.fa"]) == "(('a b':0.25,'it''s':0.25):0,x/y.fa:0.125);\n"
    with pytest.raises(ValueError, match="2 roots"):
        pkg.linkage_newick(merges[:1], [2], ["A", "B", "C"])
    assert pkg.linkage_newick(merges[:1], [2], ["A", "B", "C"], fill=2.0) == "((A:0.25,B:0.25):0.75,C:1);\n"
    assert pkg.linkage_newick(as_records([]), [], ["A"]) == "A;\n" and pkg.linkage_newick(as_records([]), [], []) == ";\n"
    # a chain as deep as its leaves: no recursion
    n = 5000
    chain = as_records([(0, k, float(k)) for k in range(1, n)])
    text = pkg.linkage_newick(chain, list(range(2, n + 1)), [f"g{k}" for k in range(n)])
    assert text.count("(") == n - 1 and text.endswith(f",g{n - 1}:{(n - 1) / 2:g});\n")
    table = pkg.linkage_table(["p/a", "p/b", "p/c"], {"merges": merges, "sizes": [2, 3]})
    assert table == "p/a\tp/b\t0.500000\t2\np/a\tp/c\t0.250000\t3\n"


# ---- 5. arguments and the command line, without a device -----------------------------------------------------------------------------------------
def test_arguments():
    assert [pkg.linkage_code(m) for m in METHODS] == [pkg.LINKAGE_SINGLE, pkg.LINKAGE_COMPLETE, pkg.LINKAGE_AVERAGE, pkg.LINKAGE_WEIGHTED] == [0, 1, 2, 3]
    assert pkg.linkage_code(2) == 2
    for bad in ("ward", "centroid", 4, -1, True, None, 2.0):
        with pytest.raises(ValueError, match="'single', 'complete', 'average' or 'weighted'"):
            pkg.linkage_code(bad)
    for measure in ("union", "containment", "intersection", "smh_matches"):
        with pytest.raises(ValueError, match="symmetric"):
            pkg.linkage_from_filelist("/nonexistent/list.txt", 512, measure=measure)
    with pytest.raises(ValueError, match="method"):
        pkg.linkage_from_filelist("/nonexistent/list.txt", method="ward")
    with pytest.raises(ValueError, match="aux_bytes"):
        pkg.linkage_from_filelist("/nonexistent/list.txt", 0, measure="smh_jaccard")
    # the context-free entry checks its arguments before it touches a device
    lib = pkg.hip_lib()
    for args, text in (((None, 1, 1, 7, 1.0, None, None), "bad method 7"), ((None, 1, 1, 2, float("nan"), None, None), "max_height is NaN"),
                       ((None, 4, 3, 2, 1.0, None, None), "ld >= n"), ((None, -1, 4, 2, 1.0, None, None), "0 <= n"), ((None, 4, 4, 2, 1.0, None, None), "non-null"),
                       ((8, 1, 1, 2, 1.0, 24, None), "16-byte aligned"), ((12, 1, 1, 2, 1.0, None, None), "8-byte aligned")):
        assert lib.selhip_linkage(*args, None, None, None) == -1 and text in lib.selhip_last_error(None).decode(), text
    import ctypes as C
    f, rounds = C.c_int64(-5), C.c_int64(-5)
    assert lib.selhip_linkage(None, 0, 0, 2, 1.0, None, None, C.byref(f), C.byref(rounds), None) == 0 and (f.value, rounds.value) == (0, 0)
    assert lib.selhip_linkage(None, 1, 1, 0, float("inf"), None, None, C.byref(f), C.byref(rounds), None) == 0 and (f.value, rounds.value) == (0, 1)
    assert lib.selhip_ctx_linkage(None, 0, 2, 1.0, None, None) == -1


def test_cli_refusals():
    sel = str(BIN / "selection")
    run = lambda args: subprocess.run([sel] + args, capture_output=True, text=True)
    lst = ["-l", "/nonexistent/list.txt"]
    tree = ["-N", "/nonexistent/dir/tree.nwk"]
    for args, word in ((lst + ["-X", "average"], "-X (the linkage method) is an option of -N / -J"),
                       (lst + tree + ["-X", "ward"], "-X (the linkage method): average, complete, weighted or single, not 'ward'"),
                       (lst + tree + ["-q", "/nonexistent/q.txt"], "cannot be combined with -q"), (lst + tree + ["-p", "/nonexistent/p.txt"], "cannot be combined with -p"),
                       (lst + ["-J", "/nonexistent/dir/m.tsv", "-g", "2"], "cannot be combined with -g"), (lst + tree + ["-B", "100"], "cannot be combined with -B"),
                       (tree + ["-r", "/nonexistent/in.selr"], "cannot be combined with -r"), (lst + tree + ["-h", "0.9"], "cannot be combined with -h"),
                       (lst + tree + ["-L", "/nonexistent/dir/c.tsv"], "cannot be combined with -L"), (lst + tree + ["-K", "3"], "cannot be combined with -K"),
                       (lst + tree + ["-U"], "symmetric similarity"), (lst + tree + ["-E", "smh_matches", "-a", "512"], "symmetric similarity"),
                       (lst + tree + ["-S", "containment"], "symmetric similarity"), (lst + tree + ["-E", "smh"], "give their size with -a"),
                       (lst + ["-N", ""], "need the name of the file to write"), (tree, "need the list of genomes (-l)")):
        out = run(args)
        assert out.returncode == 2 and out.stdout == "" and word in out.stderr, (args, out)
    # legal combinations get as far as reading the list
    for args in (lst + tree, lst + tree + ["-J", "/nonexistent/dir/m.tsv", "-X", "single"], lst + tree + ["-E", "smh", "-a", "512"],
                 lst + tree + ["-S", "max_containment", "-X", "weighted"]):
        out = run(args)
        assert out.returncode == 1 and out.stdout == "" and "-N / -J: " in out.stderr and "cannot" not in out.stderr, (args, out)
    usage = run(["-x"]).stdout
    assert "-N tree.nwk" in usage and "-J merges.tsv" in usage and "-X average|complete|weighted|single" in usage
