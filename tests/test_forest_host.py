"""The maximum spanning forest (include/selection_hip.h section 2j) without a GPU: the two models of
tests/forest_model.py against each other, the host helpers over an edges array (forest_linkage against SciPy, forest_cluster_counts, the
defining property of the forest), the declarations, constants and exports, and the refusals of `selection -H`."""
import ctypes as C
import inspect
import math
import subprocess

import numpy as np
import pytest
from scipy.cluster.hierarchy import linkage
from scipy.spatial.distance import squareform

from conftest import ROOT
import cluster_model as CM
import forest_model as FM

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import Selector

SEL = str(ROOT / "cuda_selection_criteria_amd" / "bin" / "selection")
LIB = ROOT / "cuda_selection_criteria_amd" / "lib" / "libselhip.so"
CSRC = ROOT / "cuda_selection_criteria_amd" / "csrc"


def random_records(rng):
    """a random multigraph: duplicates, reversed entries, NaN, +-0.0, two- and three-level ties or distinct values"""
    n = int(rng.integers(1, 60))
    p = int(rng.integers(0, 4 * n))
    levels = int(rng.choice([2, 3, 1000000]))
    vals = rng.integers(0, levels, size=p) / levels - 0.25
    vals[rng.random(p) < 0.05] = float("nan")
    vals[rng.random(p) < 0.05] = -0.0
    recs = [(int(rng.integers(0, n)), int(rng.integers(0, n)), float(x)) for x in vals]
    recs += [(v, u, x) for u, v, x in recs[: p // 3]]
    return n, recs


def test_image_order():
    xs = [-math.inf, -1.5, -1e-300, -0.0, 0.0, 5e-324, 0.25, 1.0, math.inf]
    ims = [FM.image(x) for x in xs]
    assert ims[3] == ims[4] and all(a <= b for a, b in zip(ims, ims[1:])) and len(set(ims)) == len(xs) - 1 and min(ims) > 0
    assert all(FM.value_of(FM.image(x)) == x for x in xs)
    assert math.copysign(1.0, FM.value_of(FM.image(-0.0))) == 1.0                     # written +0.0


def test_models_agree():
    rng = np.random.default_rng(1)
    most = 0
    for trial in range(400):
        n, recs = random_records(rng)
        cut = float(rng.choice([-math.inf, 0.0, 0.3]))
        k, lab = FM.kruskal(recs, n, cut)
        b, comp, rounds = FM.boruvka_rounds(recs, n, cut)
        assert k == b and lab == comp, trial
        assert len(k) == n - len(set(lab))
        assert all(a < c for a, c, _ in k)
        assert rounds <= max(1, math.ceil(math.log2(max(n, 2)))) + 1, (n, rounds)
        edges = np.array([(u, v) for u, v, x in recs if x >= cut], dtype=np.int64).reshape(-1, 2)
        assert lab == CM.labels(edges, n).tolist()
        most = max(most, rounds)
    assert most >= 4


def test_model_round_counts():
    n = 4097
    asc = [(i, i + 1, i / n) for i in range(n - 1)]
    k, lab = FM.kruskal(asc, n)
    b, comp, rounds = FM.boruvka_rounds(asc, n)
    assert b == k and len(k) == n - 1 and rounds == 2 and set(comp) == {0}             # ONE picking round: a hook chain of 4 096
    assert [(a, c) for a, c, _ in k[:3]] == [(4095, 4096), (4094, 4095), (4093, 4094)]
    for n in (4096, 4097):
        ruler = [(i, i + 1, 1.0 - ((i + 1) & -(i + 1)).bit_length() / 16 + 1 / 16) for i in range(n - 1)]     # 1 - ctz(i + 1) / 16
        assert ruler[0][2] == 1.0 and ruler[1][2] == 1.0 - 1 / 16 and ruler[3][2] == 1.0 - 2 / 16
        b, comp, rounds = FM.boruvka_rounds(ruler, n)
        assert b == FM.kruskal(ruler, n)[0] and rounds == 13, (n, rounds)


def test_linkage_against_scipy():
    rng = np.random.default_rng(2)
    for n in (2, 3, 17, 40):
        J = np.zeros((n, n))
        iu = np.triu_indices(n, 1)
        J[iu] = rng.permutation(len(iu[0])) / len(iu[0])
        J = J + J.T
        recs = [(int(i), int(k), float(J[i, k])) for i, k in zip(*iu)]
        edges, _ = FM.kruskal(recs, n)
        D = 1.0 - J
        np.fill_diagonal(D, 0.0)
        want = linkage(squareform(D, checks=False), "single")
        assert np.array_equal(FM.linkage(edges, n), want), n
        got = pkg.forest_linkage(FM.as_records(edges), n)
        assert got.dtype == np.float64 and got.shape == (n - 1, 4) and np.array_equal(got, want), n
        assert np.array_equal(pkg.forest_linkage(FM.as_records(edges), n, distance=lambda v: -v)[:, 2], -FM.as_records(edges)["jaccard"])   # best first


def test_linkage_fill_rules():
    # components {0, 3}, {1, 2, 5}, {4}
    edges = FM.as_records(FM.kruskal([(3, 0, 0.9), (2, 1, 0.8), (5, 2, 0.7)], 6)[0])
    with pytest.raises(ValueError, match="3 components"):
        pkg.forest_linkage(edges, 6)
    z = pkg.forest_linkage(edges, 6, fill=2.0)
    want = [[0, 3, 1.0 - 0.9, 2], [1, 2, 1.0 - 0.8, 2], [5, 7, 1.0 - 0.7, 3], [6, 8, 2.0, 5], [4, 9, 2.0, 6]]    # then by ascending label: 1, 4
    assert np.array_equal(z, np.array(want, dtype=np.float64))
    assert pkg.forest_linkage(edges[:0], 1).shape == (0, 4) and pkg.forest_linkage(edges[:0], 0).shape == (0, 4)
    assert np.array_equal(pkg.forest_linkage(edges[:0], 2, fill=1.0), [[0, 1, 1.0, 2]])
    with pytest.raises(ValueError, match="cycle"):
        pkg.forest_linkage(FM.as_records([(0, 1, FM.image(0.5)), (0, 1, FM.image(0.4))]), 2)


def test_cluster_counts_and_defining_property():
    rng = np.random.default_rng(3)
    for trial in range(40):
        n, recs = random_records(rng)
        k, lab = FM.kruskal(recs, n)
        edges = FM.as_records(k)
        values = sorted({x for _, _, x in recs if x == x}) + [math.inf]
        counts = pkg.forest_cluster_counts(edges, n, values)
        assert counts.dtype == np.int64 and len(counts) == len(values)
        for t, c in zip(values, counts):
            # the defining property: the forest edges with value >= t connect exactly what ALL records with value >= t connect
            prefix = np.array([(a, b) for a, b, im in k if FM.value_of(im) >= t], dtype=np.int64).reshape(-1, 2)
            whole = np.array([(u, v) for u, v, x in recs if x >= t], dtype=np.int64).reshape(-1, 2)
            want = CM.labels(whole, n)
            assert np.array_equal(CM.labels(prefix, n), want), (trial, t)
            assert c == len(set(want.tolist())) == n - len(prefix), (trial, t)
            assert FM.kruskal(recs, n, t)[0] == k[:len(prefix)]                         # a cut keeps a prefix of the forest
    assert pkg.forest_cluster_counts(edges[:0], 5, 0.5).tolist() == [5]


def test_header_words():
    header = (ROOT / "include" / "selection_hip.h").read_text()
    for word in ("int selhip_ctx_spanning_forest(selhip_ctx* ctx, double min_value, const selhip_forest_t* out, int64_t* n_edges_out);",
                 "} selhip_forest_t;", "selhip_pair_t* d_edges;", "int32_t*       d_label;",
                 "int selhip_spanning_forest(const selhip_int2_t* d_pairs, const double* d_values, int64_t n_pairs, int64_t n,",
                 "2j. Single-linkage hierarchy of the result list", "goes BEFORE", "strict total order", "written +0.0", "F = n - C",
                 '"forest_rounds_last"', '"forest_edges_last"', '"forest"', "Newick", "average or complete linkage"):
        assert word in header, word
    kernels = (CSRC / "kernel_forest.cuh").read_text()
    for word in ("forest_best_kernel", "forest_pick_kernel", "forest_hook_kernel", "forest_flatten_kernel", "cut property", "HOT WORDS",
                 "never skip one that would", "No loop waits", "kernel boundary alone", "cl_unite", "greedy_image"):
        assert word in kernels, word
    code = "\n".join(ln.split("//")[0] for ln in kernels.splitlines())
    assert "asm" not in code and "cooperative" not in code and "volatile" not in code and "__syncthreads" not in code
    unit = (CSRC / "selection_kernels.hip").read_text()
    assert unit.index('#include "kernel_greedy.cuh"') < unit.index('#include "kernel_forest.cuh"')
    assert unit.index('#include "host_greedy.hpp"') < unit.index('#include "host_forest.hpp"')
    assert unit.index('#include "abi_greedy.inc"') < unit.index('#include "abi_forest.inc"')


def test_symbols_and_wrappers():
    for name in ("spanning_forest", "forest_cluster_counts", "forest_cut", "forest_linkage", "forest_from_filelist"):
        assert name in pkg.__all__ and hasattr(pkg, name), name
    exported = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    for sym in ("selhip_ctx_spanning_forest", "selhip_spanning_forest"):
        assert sym in pkg._lib.HIP_SYMBOLS and getattr(pkg.hip_lib(), sym) is not None
        assert f" T {sym}\n" in exported, sym
    assert C.sizeof(pkg._lib.Forest) == 2 * C.sizeof(C.c_void_p) and [f[0] for f in pkg._lib.Forest._fields_] == ["d_edges", "d_label"]
    assert pkg.PAIR_DTYPE.itemsize == 16 and FM.PAIR_DTYPE == pkg.PAIR_DTYPE
    sig = inspect.signature(Selector.spanning_forest).parameters
    assert list(sig) == ["self", "min_value", "to_host"] and sig["min_value"].default is None and sig["to_host"].default is True
    sig = inspect.signature(pkg.spanning_forest).parameters
    assert list(sig) == ["pairs", "n", "values", "device", "to_host"] and sig["values"].default is None and sig["device"].default == 0
    assert list(inspect.signature(pkg.forest_cut).parameters) == ["edges", "n", "t", "device"]
    assert list(inspect.signature(pkg.forest_linkage).parameters) == ["edges", "n", "distance", "fill"]
    sel_sig, fo_sig = inspect.signature(pkg.select_from_filelist).parameters, inspect.signature(pkg.forest_from_filelist).parameters
    assert list(fo_sig) == list(sel_sig) + ["cluster_min"] and all(fo_sig[k].default == sel_sig[k].default for k in sel_sig)
    with pytest.raises(ValueError, match="cluster_min"):                                # before any file is read
        pkg.forest_from_filelist("/nonexistent/list.txt", 0.9, 512, cluster_min=float("nan"))
    with pytest.raises(RuntimeError, match="selhost error"):                            # accepted: gets as far as reading the list
        pkg.forest_from_filelist("/nonexistent/list.txt", 0.9, 512, cluster_min=0.95)
    rec = FM.as_records([(0, 2, FM.image(0.5)), (1, 2, FM.image(-0.0))])
    assert pkg.forest_table(["a", "b", "c"], rec) == "a\tc\t0.500000\nb\tc\t0.000000\n"


def test_null_context_and_arguments():
    lib = pkg.hip_lib()
    out = pkg._lib.Forest()
    cnt = C.c_int64(-7)
    for value in (0.5, float("-inf"), float("nan")):
        assert lib.selhip_ctx_spanning_forest(None, value, C.byref(out), C.byref(cnt)) == -1
    assert lib.selhip_ctx_spanning_forest(None, 0.5, None, None) == -1 and cnt.value == -7
    # the building block's argument checks come before any device call
    f, rounds = C.c_int64(-7), C.c_int64(-7)
    for args in ((None, None, 1, 5, None, None), (None, None, -1, 5, None, None), (None, None, 0, -1, None, None), (None, None, 0, 1 << 31, None, None),
                 (None, None, 0, 5, 8, None)):
        assert lib.selhip_spanning_forest(*args, C.byref(f), C.byref(rounds), None) == -1, args
        assert lib.selhip_last_error(None).decode().startswith("selhip_spanning_forest: 0 <= n <= 2^31 - 1, n_pairs >= 0")
        assert f.value == -7 and rounds.value == -7
    assert lib.selhip_spanning_forest(None, None, 0, 0, None, None, C.byref(f), C.byref(rounds), None) == 0 and (f.value, rounds.value) == (0, 0)
    assert lib.selhip_spanning_forest(None, None, 0, 0, None, None, None, None, None) == 0


def run(args):
    return subprocess.run([SEL] + args, capture_output=True, text=True)


def test_cli_refusals():
    lst = ["-l", "/nonexistent/list.txt", "-h", "0.9", "-a", "512"]
    H = ["-H", "/nonexistent/forest.tsv"]
    L = ["-L", "/nonexistent/clusters.tsv"]
    for args, word in ((["-q", "/nonexistent/q.txt"] + lst + H, "-H (the spanning forest of the selected pairs) cannot be combined with -q"),
                       (lst + H + ["-M", "/nonexistent/m.tsv"], "-H (the spanning forest of the selected pairs) cannot be combined with -M"),
                       (lst + H + ["-g", "2"], "-H (the spanning forest of the selected pairs) cannot be combined with -g"),
                       (lst + H + ["-B", "64"], "-H (the spanning forest of the selected pairs) cannot be combined with -B"),
                       (H + ["-r", "/nonexistent/results.bin"], "-H (the spanning forest of the selected pairs) cannot be combined with -r"),
                       (lst + ["-H", ""], "-H needs the name of the file to write"),
                       (lst + H + ["-T", "nan"], "-T (with -H: the smallest value of an edge) must be a number"),
                       (lst + H + ["-T", "0.9x"], "-T (with -H: the smallest value of an edge) must be a number"),
                       (lst + H + L + ["-T", "nan"], "-T (with -L: the smallest value of an edge) must be a number"),
                       (lst + H + ["-Y", "max_rank"], "-Y (the representative of a cluster) is an option of -L"),
                       (lst + H + ["-T", "0.9", "-Y", "max_rank"], "-Y (the representative of a cluster) is an option of -L"),
                       (lst + H + ["-Z", "greedy"], "-Z (single or greedy clusters) is an option of -L"),
                       (lst + ["-T", "0.9"], "-T (the smallest value of an edge) is an option of -L")):
        out = run(args)
        assert out.returncode == 2 and out.stdout == "" and word in out.stderr, (args, out)
        assert "nonexistent/list" not in out.stderr and "input file" not in out.stderr, (args, out.stderr)
    # accepted wherever -L is: the run gets as far as the list
    for extra in (H, H + ["-T", "0.95"], H + ["-T", "-inf"], H + L, H + L + ["-T", "0.95", "-Z", "greedy"], H + L + ["-P", "/nonexistent/dir"],
                  H + ["-c", "none", "-n", "-h", "-1", "-K", "3"], H + ["-p", "/nonexistent/pairs.txt"], H + ["-c", "smh_c", "-C", "8"]):
        out = run(lst + extra)
        assert out.returncode not in (0, 2) and "No valid input file provided" in out.stderr, (extra, out)
    usage = run(["-x"]).stdout
    assert "-H forest.tsv [-T min_value]" in usage
    assert "-L clusters.tsv [-T min_value] [-Y max_degree|min_rank|max_rank]" in usage                 # the line of -L stays
