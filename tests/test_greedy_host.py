"""Greedy representative clusters of a result list (selhip_ctx_cluster_greedy, selhip_greedy_representatives), what
needs no GPU: the numpy model (tests/greedy_model.py) against brute-force invariants and an independent greedy, the round scheme of the
device against the sequential greedy, the header's contract, the symbols, the Python names and defaults, and every refusal of the front
ends."""
import ctypes as C
import inspect
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import greedy_model as GM

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import Selector

SEL = str(ROOT / "cuda_selection_criteria_amd" / "bin" / "selection")
LIB = ROOT / "cuda_selection_criteria_amd" / "lib" / "libselhip.so"
CSRC = ROOT / "cuda_selection_criteria_amd" / "csrc"


def random_edges(n, p_edges, seed, loops=0, duplicate=False):
    rng = np.random.default_rng(seed)
    e = rng.integers(0, max(n, 1), size=(p_edges if n else 0, 2))
    if loops and n:
        v = rng.integers(0, n, size=loops)
        e = np.concatenate([e, np.stack([v, v], axis=1)])
    if duplicate:
        e = np.concatenate([e, e[:, ::-1]])
    return e[rng.permutation(len(e))]


def complete(n):
    i, k = np.triu_indices(n, 1)
    return np.stack([i, k], axis=1)


def path(n):
    return np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)


NONE = np.zeros((0, 2), dtype=np.int64)
GRAPHS = [("empty-0", 0, NONE), ("empty-1", 1, NONE), ("empty-50", 50, NONE), ("loop-1", 1, np.array([[0, 0]])),
          ("complete-2", 2, complete(2)), ("complete-40", 40, complete(40)), ("path-2", 2, path(2)), ("path-3", 3, path(3)),
          ("path-64", 64, path(64)), ("path-257", 257, path(257)[::-1, ::-1]),
          ("star-high", 33, np.stack([np.full(32, 32), np.arange(32)], axis=1)), ("star-low", 33, np.stack([np.zeros(32, dtype=np.int64), np.arange(1, 33)], axis=1)),
          ("sparse-300", 300, random_edges(300, 150, 1)), ("mean-degree-2", 300, random_edges(300, 300, 2)),
          ("dense-200", 200, random_edges(200, 2000, 3)), ("loops", 120, random_edges(120, 60, 4, loops=40)),
          ("duplicates", 250, random_edges(250, 120, 5, duplicate=True)), ("loops+duplicates", 97, random_edges(97, 50, 6, loops=20, duplicate=True))]


def keys_of(n, kind):
    if kind == "vertex":
        return None
    if kind == "reversed":
        return [n - 1 - g for g in range(n)]
    if kind == "random":
        return np.random.default_rng(n + 3).permutation(n).tolist()
    if kind == "equal":
        return [7] * n
    if kind == "ties":
        return np.random.default_rng(n + 4).integers(0, 3, size=n).tolist()
    return [(1 << 64) - 1 - 5 * g for g in range(n)]                                 # "wide": keys that need all 64 bits


@pytest.mark.parametrize("kind", ["vertex", "reversed", "random", "equal", "ties", "wide"])
@pytest.mark.parametrize("name,n,edges", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_model_representatives(name, n, edges, kind):
    key = keys_of(n, kind)
    rep = GM.representatives(edges, n, key)
    assert rep.dtype == bool and rep.shape == (n,)
    assert np.array_equal(rep, GM.representatives_by_lists(edges, n, key))           # the independent adjacency-list greedy
    e = np.asarray(edges).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    assert not np.any(rep[e[:, 0]] & rep[e[:, 1]])                                   # no edge between two representatives
    has_rep_neighbour = np.zeros(n, dtype=bool)
    has_rep_neighbour[e[rep[e[:, 1]], 0]] = True
    has_rep_neighbour[e[rep[e[:, 0]], 1]] = True
    assert np.array_equal(has_rep_neighbour, ~rep)                                   # maximal: every other vertex has one for a neighbour
    # lexicographically first: the first vertex of the order is one, and each one has no representative among its EARLIER neighbours only
    order = GM.visiting_order(n, key)
    if n:
        assert rep[order[0]]
        pos = np.empty(n, dtype=np.int64)
        pos[order] = np.arange(n)
        for g in np.flatnonzero(~rep).tolist():
            nb = np.concatenate([e[e[:, 0] == g, 1], e[e[:, 1] == g, 0]])
            assert np.any(rep[nb] & (pos[nb] < pos[g])), (name, kind, g)
    rounds, rep_rounds = GM.rounds_synchronous(edges, n, key)                        # the device's scheme, every read stale
    assert np.array_equal(rep_rounds, rep)
    assert (rounds == 0) if n == 0 else 1 <= rounds <= n
    if kind == "equal":
        assert np.array_equal(rep, GM.representatives(edges, n, [n - g for g in range(n)]))     # equal keys: the smaller vertex first
    if name.startswith("empty") or name == "loop-1":
        assert np.all(rep) and rounds == min(n, 1)
    if name.startswith("complete"):
        assert rep.sum() == 1 and rep[order[0]] and rounds == 2
    if name == "star-high" and kind == "vertex":
        assert rep.tolist() == [False] * 32 + [True] and rounds == 2
    if name == "star-low" and kind == "vertex":
        assert rep.tolist() == [False] + [True] * 32 and rounds == 2
    if name == "path-257" and kind == "vertex":
        assert rounds == 257 and np.array_equal(rep, np.arange(257) % 2 == 0)        # the monotone path: one round per vertex


def records(edges, values):
    rec = np.zeros(len(edges), dtype=pkg.PAIR_DTYPE)
    e = np.asarray(edges).reshape(-1, 2)
    rec["i"], rec["k"], rec["jaccard"] = e[:, 0], e[:, 1], values
    return rec


@pytest.mark.parametrize("rule", ["max_degree", "min_rank", "max_rank", "priority"])
@pytest.mark.parametrize("name,n,edges", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_model_assignment(name, n, edges, rule):
    rng = np.random.default_rng(len(edges) + n)
    values = rng.integers(0, 5, size=len(edges)) / 4.0                               # few levels: ties everywhere
    rec = records(edges, values)
    prio = rng.integers(0, 4, size=n) if rule == "priority" else None
    for cut in (-np.inf, 0.5, 1.0):
        res = GM.clusters(rec, n, cut, rule, prio)
        rep = np.zeros(n, dtype=bool)
        rep[res["representatives"]] = True
        kept = GM.keep(rec, cut)
        assert int(res["degrees"].sum()) == 2 * len(kept)                             # records, self-records twice
        live = kept[kept["i"] != kept["k"]]
        pairs = np.stack([live["i"], live["k"]], axis=1).reshape(-1, 2)
        assert np.array_equal(rep, GM.representatives(pairs, n, GM.order_keys(rule, n, res["degrees"], prio)))
        weight = {}
        for i, k, v in zip(live["i"].tolist(), live["k"].tolist(), live["jaccard"].tolist()):
            weight[(i, k)] = weight[(k, i)] = max(v, weight.get((i, k), -np.inf))      # repeats: one edge, the greatest value
        assert not any(rep[i] and rep[k] for i, k in weight)
        for g in range(n):
            r = int(res["rep_of"][g])
            if rep[g]:
                assert r == g and res["values"][g] == 1.0
                continue
            assert rep[r] and (g, r) in weight and weight[(g, r)] == res["values"][g]  # an edge to its representative, with its value
            to_reps = {x: v for (a, x), v in weight.items() if a == g and rep[x]}
            assert weight[(g, r)] == max(to_reps.values())                            # its best edge to ANY representative ...
            assert r == min(x for x, v in to_reps.items() if v == weight[(g, r)])     # ... ties to the smaller rank
        c = res["n_clusters"]
        assert c == rep.sum() and np.array_equal(res["representatives"], np.flatnonzero(rep))       # numbered by ascending representative
        assert np.array_equal(res["representatives"][res["clusters"]], res["rep_of"])
        assert np.array_equal(res["sizes"], np.bincount(res["clusters"], minlength=c)) and int(res["sizes"].sum()) == n
        assert res["rep_of"].dtype == np.int32 and res["values"].dtype == np.float64 and res["clusters"].dtype == np.int32
        assert res["rounds_bound"] == (0 if n == 0 else 1 if len(rec) == 0 else GM.rounds_synchronous(pairs, n, GM.order_keys(rule, n, res["degrees"], prio))[0])


def test_model_chain_zero_and_table():
    # the chain A - B - C without A - C: single linkage has one cluster; the greedy two under max_rank, one where B goes first
    rec = records([[0, 1], [1, 2]], [0.96, 0.97])
    by_rank = GM.clusters(rec, 3, 0.95, "max_rank")
    assert by_rank["n_clusters"] == 2 and by_rank["representatives"].tolist() == [0, 2] and by_rank["rep_of"].tolist() == [0, 2, 2]
    assert by_rank["values"].tolist() == [1.0, 0.97, 1.0]
    by_degree = GM.clusters(rec, 3, 0.95, "max_degree")
    assert by_degree["n_clusters"] == 1 and by_degree["rep_of"].tolist() == [1, 1, 1] and by_degree["values"].tolist() == [0.96, 1.0, 0.97]
    assert GM.clusters(rec, 3, 0.95, "priority", [0, 5, 0])["rep_of"].tolist() == [1, 1, 1]
    assert GM.clusters(rec, 3, 0.965, "max_rank")["rep_of"].tolist() == [0, 2, 2]
    # a member's best edge leads to a non-representative: it is not assigned along it
    rec = records([[0, 3], [1, 3], [0, 1]], [0.5, 0.6, 0.9])                          # max_rank: 3 first; 0 and 1 are its members
    res = GM.clusters(rec, 4, -np.inf, "max_rank")
    assert res["representatives"].tolist() == [2, 3] and res["rep_of"].tolist() == [3, 3, 2, 3] and res["values"].tolist() == [0.5, 0.6, 1.0, 1.0]
    # -0.0 and +0.0 tie (the smaller rank wins) and a zero is written +0.0; NaN is never an edge; a directed pair is one edge
    rec = records([[2, 0], [2, 1], [0, 2], [3, 2], [3, 3]], [0.0, -0.0, -0.0, np.nan, 0.25])
    res = GM.clusters(rec, 4, -np.inf, "min_rank")
    assert res["representatives"].tolist() == [0, 1, 3] and res["rep_of"].tolist() == [0, 1, 0, 3]
    assert res["values"].view(np.uint64).tolist() == np.array([1.0, 1.0, 0.0, 1.0]).view(np.uint64).tolist()
    assert res["degrees"].tolist() == [2, 1, 3, 2]                                    # the NaN record counts for nobody, the self-record twice
    assert GM.clusters(rec, 4, np.inf)["n_clusters"] == 4
    text = GM.table(["a", "b", "c", "d"], np.array([3, 2, 1, 0]), res)
    assert text == "d\t2\t1\t2\td\t1.000000\nc\t0\t2\t3\ta\t0.000000\nb\t1\t1\t1\tb\t1.000000\na\t0\t2\t2\ta\t1.000000\n"
    from cuda_selection_criteria_amd.selection import greedy_table
    assert greedy_table(["a", "b", "c", "d"], np.array([3, 2, 1, 0]), res) == text


def test_header_words():
    header = (ROOT / "include" / "selection_hip.h").read_text()
    for word in ("int selhip_ctx_cluster_greedy(selhip_ctx* ctx, double min_value, int order_rule, const uint32_t* d_priority,",
                 "const selhip_greedy_t* out, int64_t* n_clusters_out);", "} selhip_greedy_t;", "int32_t* d_rep_of;", "double*  d_value;",
                 "int selhip_greedy_representatives(const selhip_int2_t* d_pairs, int64_t n_pairs, int64_t n, const uint64_t* d_key /* [n] or NULL */,",
                 "uint8_t* d_is_rep /* [n] */, int64_t* rounds_out /* may be NULL */, void* hip_stream);",
                 "#define SELHIP_REP_PRIORITY 3", "2h. Greedy representative clusters", "lexicographically first maximal independent set",
                 "ties go to the smaller rank r", "-0.0 equals +0.0", "any of the six pointers may be NULL", '"greedy_clusters_last"', '"greedy_rounds_last"',
                 '"greedy"', "the greatest of theirs", "accepted by this entry only", "equal keys: the smaller vertex goes first"):
        assert word in header, word
    kernels = (CSRC / "kernel_greedy.cuh").read_text()
    for word in ("WHY ANY INTERLEAVING GIVES THE SEQUENTIAL ANSWER", "a stale read can delay a decision, never change", "at most n rounds",
                 "No loop waits", "kernel boundary alone", "greedy_edges_kernel", "greedy_vertices_kernel", "cl_degree_add", "cluster_rep_key"):
        assert word in kernels, word
    code = "\n".join(ln.split("//")[0] for ln in kernels.splitlines())
    assert "asm" not in code and "cooperative" not in code and "while" not in code      # no loop but the grid-stride ones
    assert "__hip_atomic_load" not in code and "volatile" not in code                  # nothing polls
    unit = (CSRC / "selection_kernels.hip").read_text()
    assert unit.index('#include "kernel_cluster.cuh"') < unit.index('#include "kernel_greedy.cuh"')
    assert unit.index('#include "host_cluster.hpp"') < unit.index('#include "host_greedy.hpp"')
    assert unit.index('#include "abi_cluster.inc"') < unit.index('#include "abi_greedy.inc"')


def test_symbols_and_wrappers():
    assert pkg.REP_PRIORITY == 3 == pkg._lib.REP_PRIORITY
    for name in ("greedy_representatives", "greedy_from_filelist", "REP_PRIORITY", "order_code"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    for sym in ("selhip_ctx_cluster_greedy", "selhip_greedy_representatives"):
        assert sym in pkg._lib.HIP_SYMBOLS and getattr(pkg.hip_lib(), sym) is not None
        assert f" T {sym}\n" in exported, sym
    assert C.sizeof(pkg._lib.Greedy) == 6 * C.sizeof(C.c_void_p)
    assert [f[0] for f in pkg._lib.Greedy._fields_] == ["d_rep_of", "d_value", "d_cluster", "d_degree", "d_cluster_size", "d_cluster_rep"]
    sig = inspect.signature(Selector.cluster_greedy).parameters
    assert list(sig) == ["self", "min_value", "order", "priority", "to_host"]
    assert sig["min_value"].default is None and sig["order"].default == "max_degree" and sig["priority"].default is None and sig["to_host"].default is True
    sig = inspect.signature(pkg.greedy_representatives).parameters
    assert list(sig) == ["pairs", "n", "keys", "device", "to_host"]
    assert sig["keys"].default is None and sig["device"].default == 0 and sig["to_host"].default is True
    sel_sig, gr_sig = inspect.signature(pkg.select_from_filelist).parameters, inspect.signature(pkg.greedy_from_filelist).parameters
    assert list(gr_sig) == list(sel_sig) + ["cluster_min", "order", "priority"]         # the arguments of select_from_filelist, then its own
    assert all(gr_sig[k].default == sel_sig[k].default for k in sel_sig)
    assert gr_sig["cluster_min"].default is None and gr_sig["order"].default == "max_degree" and gr_sig["priority"].default is None
    # the single-linkage names keep their signatures and refusals
    assert list(inspect.signature(Selector.cluster).parameters) == ["self", "min_value", "rep", "to_host"]
    assert pkg.selection.REPS == {"max_degree": 0, "min_rank": 1, "max_rank": 2}
    with pytest.raises(ValueError, match="rep"):
        pkg.rep_code(3)


def test_order_names(tmp_path):
    assert [pkg.order_code(r) for r in ("max_degree", "min_rank", "max_rank", "priority", 0, 1, 2, 3, np.int32(3))] == [0, 1, 2, 3, 0, 1, 2, 3, 3]
    missing = str(tmp_path / "no_such_list.txt")
    for bad in ("degree", "Priority", "", 4, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="order"):
            pkg.order_code(bad)
        with pytest.raises(ValueError, match="order"):                                # before any file is read
            pkg.greedy_from_filelist(missing, 0.9, 512, order=bad)
    with pytest.raises(ValueError, match="cluster_min"):
        pkg.greedy_from_filelist(missing, 0.9, 512, cluster_min=float("nan"))
    with pytest.raises(ValueError, match="priority"):
        pkg.greedy_from_filelist(missing, 0.9, 512, order="priority")
    with pytest.raises(ValueError, match="priority"):
        pkg.greedy_from_filelist(missing, 0.9, 512, order="max_rank", priority=[1, 2])
    for ok in (dict(), dict(order="min_rank"), dict(cluster_min=0.95, order="max_rank"), dict(priority=[3, 1]), dict(order="priority", priority=[3, 1])):
        with pytest.raises(RuntimeError, match="selhost error"):                      # accepted: gets as far as reading the list
            pkg.greedy_from_filelist(missing, 0.9, 512, **ok)


def test_null_context_and_arguments():
    lib = pkg.hip_lib()
    out = pkg._lib.Greedy()
    cnt = C.c_int64(-7)
    for rule in (0, 1, 2, 3, 4, -1):
        for value in (0.5, float("-inf"), float("nan")):
            assert lib.selhip_ctx_cluster_greedy(None, value, rule, None, C.byref(out), C.byref(cnt)) == -1
    assert lib.selhip_ctx_cluster_greedy(None, 0.5, 0, None, None, None) == -1
    assert cnt.value == -7
    # the building block's argument checks come before any device call, with the message form of selhip_components
    rounds = C.c_int64(-7)
    for args in ((None, 1, 5, None, None), (None, -1, 5, None, None), (None, 0, -1, None, None), (None, 0, 1 << 31, None, None), (None, 0, 3, None, None)):
        assert lib.selhip_greedy_representatives(args[0], args[1], args[2], args[3], args[4], C.byref(rounds), None) == -1, args
        msg = lib.selhip_last_error(None).decode()
        assert msg.startswith("selhip_greedy_representatives: 0 <= n <= 2^31 - 1, n_pairs >= 0, and non-null arrays"), msg
        assert rounds.value == -7
    assert lib.selhip_greedy_representatives(None, 0, 0, None, None, C.byref(rounds), None) == 0 and rounds.value == 0     # nothing to do is legal
    assert lib.selhip_greedy_representatives(None, 0, 0, None, None, None, None) == 0


def run(args):
    return subprocess.run([SEL] + args, capture_output=True, text=True)


def test_cli_refusals():
    lst = ["-l", "/nonexistent/list.txt", "-h", "0.9", "-a", "512"]
    L = ["-L", "/nonexistent/clusters.tsv"]
    W = ["-W", "/nonexistent/scores.tsv"]
    for args, word in ((lst + ["-Z", "greedy"], "-Z (single or greedy clusters) is an option of -L"),
                       (lst + ["-Z", "single"], "-Z (single or greedy clusters) is an option of -L"),
                       (lst + W, "-W (the scores that order the greedy clusters) is an option of -L"),
                       (lst + ["-Z", "greedy"] + W, "-Z (single or greedy clusters) is an option of -L"),
                       (lst + L + ["-Z", "average"], "-Z (with -L: how the selected pairs are clustered): single or greedy, not 'average'"),
                       (lst + L + ["-Z", ""], "-Z (with -L: how the selected pairs are clustered): single or greedy"),
                       (lst + L + ["-Z", "Greedy"], "-Z (with -L: how the selected pairs are clustered): single or greedy"),
                       (lst + L + W, "-W (the scores that order the greedy clusters) is an option of -L ... -Z greedy"),
                       (lst + L + ["-Z", "single"] + W, "-W (the scores that order the greedy clusters) is an option of -L ... -Z greedy"),
                       (lst + L + ["-Z", "greedy", "-Y", "max_rank"] + W, "-W (the scores that order the greedy clusters of -L) cannot be combined with -Y"),
                       (lst + L + ["-Z", "greedy", "-W", ""], "-W (with -L -Z greedy) needs the name of the file of scores"),
                       (lst + L + ["-Z", "greedy", "-Y", "priority"], "-Y (with -L: the representative of a cluster): max_degree, min_rank or max_rank"),
                       (lst + L + ["-Z", "greedy", "-T", "nan"], "-T (with -L: the smallest value of an edge) must be a number"),
                       (["-q", "/nonexistent/q.txt"] + lst + L + ["-Z", "greedy"], "-L (the clusters of the selected pairs) cannot be combined with -q"),
                       (lst + L + ["-Z", "greedy", "-g", "2"], "-L (the clusters of the selected pairs) cannot be combined with -g")):
        out = run(args)
        assert out.returncode == 2 and out.stdout == "" and word in out.stderr, (args, out)
        assert "nonexistent/list" not in out.stderr and "input file" not in out.stderr, (args, out.stderr)
    # accepted: the run gets as far as the list, before the scores are opened
    Z = L + ["-Z", "greedy"]
    for extra in (Z, L + ["-Z", "single"], L + ["-Z", "single", "-Y", "max_rank"], Z + ["-T", "0.95"], Z + ["-Y", "max_rank"], Z + W, Z + W + ["-T", "-inf"],
                  Z + ["-c", "none", "-n", "-h", "-1", "-K", "3"], Z + W + ["-c", "none", "-n", "-h", "-1", "-K", "3"], Z + ["-p", "/nonexistent/pairs.txt"]):
        out = run(lst + extra)
        assert out.returncode not in (0, 2) and "No valid input file provided" in out.stderr, (extra, out)
    usage = run(["-x"]).stdout
    assert "-L clusters.tsv [-T min_value] [-Y max_degree|min_rank|max_rank]" in usage                 # the line of -L stays
    assert "-L clusters.tsv -Z single|greedy [-T min_value] [-Y max_degree|min_rank|max_rank | -W scores.tsv]" in usage
