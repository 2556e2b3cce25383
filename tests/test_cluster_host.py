"""Single-linkage clusters of a result list (selhip_ctx_cluster, selhip_components), what needs no GPU: the numpy
model (tests/cluster_model.py) against a breadth-first search, the header's contract, the symbols, the Python names and defaults, and
every refusal of the front ends."""
import ctypes as C
import inspect
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import cluster_model as CM

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import Selector

SEL = str(ROOT / "cuda_selection_criteria_amd" / "bin" / "selection")
LIB = ROOT / "cuda_selection_criteria_amd" / "lib" / "libselhip.so"


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


GRAPHS = [("empty-0", 0, np.zeros((0, 2), dtype=np.int64)), ("empty-1", 1, np.zeros((0, 2), dtype=np.int64)),
          ("empty-50", 50, np.zeros((0, 2), dtype=np.int64)), ("loop-1", 1, np.array([[0, 0]])), ("complete-2", 2, complete(2)),
          ("complete-40", 40, complete(40)), ("complete-150", 150, complete(150)),
          ("sparse-300", 300, random_edges(300, 150, 1)), ("mean-degree-2", 300, random_edges(300, 300, 2)),
          ("dense-200", 200, random_edges(200, 2000, 3)), ("loops", 120, random_edges(120, 60, 4, loops=40)),
          ("duplicates", 250, random_edges(250, 120, 5, duplicate=True)), ("loops+duplicates", 97, random_edges(97, 50, 6, loops=20, duplicate=True)),
          ("path-desc", 64, np.stack([np.arange(63, 0, -1), np.arange(62, -1, -1)], axis=1)),
          ("star-high", 33, np.stack([np.full(32, 32), np.arange(32)], axis=1))]


@pytest.mark.parametrize("name,n,edges", GRAPHS, ids=[g[0] for g in GRAPHS])
def test_model_against_bfs(name, n, edges):
    lab = CM.labels(edges, n)
    assert np.array_equal(lab, CM.bfs_labels(edges, n)) and lab.dtype == np.int32
    assert np.all(lab <= np.arange(n)) and np.array_equal(lab[lab], lab)          # a label is the smallest member, and its own label
    cl, c = CM.dense_ids(lab)
    roots = np.flatnonzero(lab == np.arange(n))
    assert c == len(roots) and np.array_equal(cl[roots], np.arange(c))            # numbered by ascending label
    assert np.array_equal(roots[cl], lab)
    deg = CM.degrees(edges, n)
    assert int(deg.sum()) == 2 * len(edges)
    sz = CM.sizes(cl, c)
    assert int(sz.sum()) == n and np.all(sz >= 1)
    res = CM.clusters(edges, n)
    assert res["n_clusters"] == c and np.array_equal(res["labels"], lab)
    for rule in ("max_degree", "min_rank", "max_rank"):
        rep = CM.representatives(cl, c, deg, rule)
        assert np.array_equal(cl[rep], np.arange(c))                              # a member of its cluster
        for k in range(c):
            members = np.flatnonzero(cl == k)
            if rule == "min_rank":
                assert rep[k] == members.min() == roots[k]
            elif rule == "max_rank":
                assert rep[k] == members.max()
            else:
                best = deg[members].max()
                assert rep[k] == members[deg[members] == best].min()
    if "complete" in name:
        assert c == 1 and np.all(deg == n - 1) and sz[0] == n
    if name.startswith("empty"):
        assert c == n and np.all(deg == 0) and np.array_equal(res["representatives"], np.arange(n))


def test_model_record_edges_and_table():
    rec = np.zeros(5, dtype=pkg.PAIR_DTYPE)
    rec["i"], rec["k"] = [0, 1, 2, 0, 3], [1, 2, 3, 3, 4]
    rec["jaccard"] = [0.5, np.nextafter(0.5, 1.0), np.nextafter(0.5, 0.0), np.nan, -0.25]
    assert CM.record_edges(rec).tolist() == [[0, 1], [1, 2], [2, 3], [3, 4]]      # -inf takes everything but the NaN
    assert CM.record_edges(rec, 0.5).tolist() == [[0, 1], [1, 2]]
    assert CM.record_edges(rec, np.inf).shape == (0, 2)
    res = CM.clusters(CM.record_edges(rec, 0.5), 5)
    assert res["labels"].tolist() == [0, 0, 0, 3, 4] and res["n_clusters"] == 3 and res["representatives"].tolist() == [1, 3, 4]
    text = CM.table(["a", "b", "c", "d", "e"], np.array([4, 3, 2, 1, 0]), res)
    assert text == "e\t2\t1\t0\te\nd\t1\t1\t0\td\nc\t0\t3\t1\tb\nb\t0\t3\t2\tb\na\t0\t3\t1\tb\n"
    from cuda_selection_criteria_amd.selection import cluster_table
    assert cluster_table(["a", "b", "c", "d", "e"], np.array([4, 3, 2, 1, 0]), res) == text


def test_header_words():
    header = (ROOT / "include" / "selection_hip.h").read_text()
    for word in ("int selhip_components(const selhip_int2_t* d_pairs, int64_t n_pairs, int64_t n, int32_t* d_label /*[n]*/, void* hip_stream);",
                 "int selhip_ctx_cluster(selhip_ctx* ctx, double min_value, int rep_rule,", "const selhip_clusters_t* out, int64_t* n_clusters_out);",
                 "} selhip_clusters_t;", "int32_t* d_label;", "int32_t* d_cluster;", "int32_t* d_degree;", "int32_t* d_cluster_size;", "int32_t* d_cluster_rep;",
                 "#define SELHIP_REP_MAX_DEGREE 0", "#define SELHIP_REP_MIN_RANK   1", "#define SELHIP_REP_MAX_RANK   2",
                 "2g. Single-linkage clusters", "records, not distinct partners", "a mutual pair counts twice", "an entry listed twice counts twice",
                 "ties go to the smaller rank", "two index spaces", '"clusters_last"', '"cluster"', "-INFINITY", "any of the five pointers may be NULL"):
        assert word in header, word
    kernels = "".join((ROOT / "cuda_selection_criteria_amd" / "csrc" / name).read_text() for name in ("kernel_graph.cuh", "kernel_cluster.cuh"))
    for word in ("__HIP_MEMORY_SCOPE_AGENT", "__hip_atomic_fetch_min", "__hip_atomic_load", "at most n steps", "No loop waits"):
        assert word in kernels, word
    assert "asm" not in kernels and "cooperative" not in kernels.replace("no cooperative launch", "")


def test_symbols_and_wrappers():
    assert (pkg.REP_MAX_DEGREE, pkg.REP_MIN_RANK, pkg.REP_MAX_RANK) == (0, 1, 2)
    assert (pkg._lib.REP_MAX_DEGREE, pkg._lib.REP_MIN_RANK, pkg._lib.REP_MAX_RANK) == (0, 1, 2)
    for name in ("components", "cluster_from_filelist", "REP_MAX_DEGREE", "REP_MIN_RANK", "REP_MAX_RANK"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    for sym in ("selhip_ctx_cluster", "selhip_components"):
        assert sym in pkg._lib.HIP_SYMBOLS and getattr(pkg.hip_lib(), sym) is not None
        assert f" T {sym}\n" in exported, sym
    assert C.sizeof(pkg._lib.Clusters) == 5 * C.sizeof(C.c_void_p)
    assert [f[0] for f in pkg._lib.Clusters._fields_] == ["d_label", "d_cluster", "d_degree", "d_cluster_size", "d_cluster_rep"]
    sig = inspect.signature(Selector.cluster).parameters
    assert sig["min_value"].default is None and sig["rep"].default == "max_degree" and sig["to_host"].default is True
    sig = inspect.signature(pkg.components).parameters
    assert list(sig)[:2] == ["pairs", "n"]
    sel_sig, cl_sig = inspect.signature(pkg.select_from_filelist).parameters, inspect.signature(pkg.cluster_from_filelist).parameters
    assert list(cl_sig) == list(sel_sig) + ["cluster_min", "rep"]                  # the arguments of select_from_filelist, then its own
    assert all(cl_sig[k].default == sel_sig[k].default for k in sel_sig)
    assert cl_sig["cluster_min"].default is None and cl_sig["rep"].default == "max_degree"


def test_rep_names(tmp_path):
    from cuda_selection_criteria_amd.selection import rep_code
    assert [rep_code(r) for r in ("max_degree", "min_rank", "max_rank", 0, 1, 2, np.int32(2))] == [0, 1, 2, 0, 1, 2, 2]
    missing = str(tmp_path / "no_such_list.txt")
    for bad in ("degree", "Max_degree", "", "min", 3, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="rep"):
            rep_code(bad)
        with pytest.raises(ValueError, match="rep"):                              # before any file is read
            pkg.cluster_from_filelist(missing, 0.9, 512, rep=bad)
    with pytest.raises(ValueError, match="cluster_min"):
        pkg.cluster_from_filelist(missing, 0.9, 512, cluster_min=float("nan"))
    for ok in (dict(), dict(rep="min_rank"), dict(cluster_min=0.95, rep="max_rank"), dict(cluster_min=-np.inf)):
        with pytest.raises(RuntimeError, match="selhost error"):                  # accepted: gets as far as reading the list
            pkg.cluster_from_filelist(missing, 0.9, 512, **ok)


def test_null_context():
    lib = pkg.hip_lib()
    out = pkg._lib.Clusters()
    cnt = C.c_int64(-7)
    for rule in (0, 1, 2, 3):
        for value in (0.5, float("-inf"), float("nan")):
            assert lib.selhip_ctx_cluster(None, value, rule, C.byref(out), C.byref(cnt)) == -1
    assert lib.selhip_ctx_cluster(None, 0.5, 0, None, None) == -1
    assert cnt.value == -7
    # the building block's argument checks come before any device call
    for args in ((None, 1, 5, None), (None, -1, 5, None), (None, 0, -1, None), (None, 0, 1 << 31, None), (None, 0, 3, None)):
        assert lib.selhip_components(args[0], args[1], args[2], args[3], None) == -1, args
    assert lib.selhip_components(None, 0, 0, None, None) == 0                     # nothing to do is legal


def run(args):
    return subprocess.run([SEL] + args, capture_output=True, text=True)


def test_cli_refusals():
    lst = ["-l", "/nonexistent/list.txt", "-h", "0.9", "-a", "512"]
    L = ["-L", "/nonexistent/clusters.tsv"]
    for args, word in ((["-q", "/nonexistent/q.txt"] + lst + L, "-L (the clusters of the selected pairs) cannot be combined with -q"),
                       (["-l", "/nonexistent/list.txt", "-M", "/nonexistent/m.tsv"] + L, "-L (the clusters of the selected pairs) cannot be combined with -M"),
                       (lst + L + ["-g", "2"], "-L (the clusters of the selected pairs) cannot be combined with -g"),
                       (lst + L + ["-B", "100"], "-L (the clusters of the selected pairs) cannot be combined with -B"),
                       (L + ["-r", "/nonexistent/x.selr"], "-L (the clusters of the selected pairs) cannot be combined with -r"),
                       (lst + ["-T", "0.95"], "-T (the smallest value of an edge) is an option of -L"),
                       (lst + ["-Y", "max_rank"], "-Y (the representative of a cluster) is an option of -L"),
                       (lst + ["-T", "0.95", "-Y", "max_rank"], "is an option of -L"),
                       (lst + L + ["-Y", "degree"], "-Y (with -L: the representative of a cluster): max_degree, min_rank or max_rank"),
                       (lst + L + ["-T", "x"], "-T (with -L: the smallest value of an edge) must be a number"),
                       (lst + L + ["-T", "nan"], "-T (with -L: the smallest value of an edge) must be a number"),
                       (lst + L + ["-T", ""], "-T (with -L: the smallest value of an edge) must be a number"),
                       (lst + ["-L", ""], "-L needs the name of the file to write")):
        out = run(args)
        assert out.returncode == 2 and out.stdout == "" and word in out.stderr, (args, out)
        assert "-L" in out.stderr
        assert "nonexistent/list" not in out.stderr and "input file" not in out.stderr, (args, out.stderr)
    # accepted: the run gets as far as the list
    for extra in (L, L + ["-T", "0.95"], L + ["-T", "-inf"], L + ["-Y", "min_rank"], L + ["-c", "none", "-n", "-h", "-1", "-K", "3"],
                  L + ["-p", "/nonexistent/pairs.txt"], L + ["-c", "hll_a"], L + ["-c", "smh_c", "-C", "1", "-V", "smh", "-K", "3", "-R", "2"]):
        out = run(lst + extra)
        assert out.returncode not in (0, 2) and "No valid input file provided" in out.stderr, (extra, out)
    usage = run(["-x"]).stdout
    assert "-L clusters.tsv [-T min_value] [-Y max_degree|min_rank|max_rank]" in usage
