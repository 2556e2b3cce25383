"""The neighbour-joining tree without a device (include/selection_hip.h section 2l): the model tests/nj_model.py on additive dyadic
trees -- where every operation of the definition is exact, so the truth does not depend on the model --, the declarations, the
host helpers of the package, the argument checks and the command line's refusals."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import nj_model as NM

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import _lib

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"


@pytest.mark.parametrize("n", (3, 4, 5, 17, 64, 130))
def test_model_recovers_additive_trees(n):
    """edge lengths that are multiples of 2^-6 below 4: no operation rounds, so the splits are the tree's and the recorded lengths
    sum to the tree's total edge length, exactly"""
    for seed in (1, 2, 3):
        dist, total, splits = NM.dyadic_tree(n, seed)
        joins = NM.neighbor_joining(dist)
        assert len(joins) == n - 1 and np.all(joins["a"] < joins["b"])
        assert NM.join_splits(joins, n) == splits
        assert float(np.sum(joins["len_a"]) + np.sum(joins["len_b"])) == total
        assert np.all(joins["len_a"] > 0) and np.all(joins["len_b"] > 0)
    assert len(NM.neighbor_joining(np.zeros((1, 1)))) == 0 and len(NM.neighbor_joining(np.zeros((0, 0)))) == 0
    assert NM.neighbor_joining(np.array([[0.0, 3.0], [9.0, 0.0]])).tolist() == [(0, 1, 1.5, 1.5)]      # only the upper triangle is input


def test_declarations_and_dtype():
    header = (ROOT / "include" / "selection_hip.h").read_text()
    for name in ("selhip_neighbor_joining", "selhip_ctx_neighbor_joining"):
        assert name in _lib.HIP_SYMBOLS and f"int {name}(" in header
        assert hasattr(pkg.hip_lib(), name)
    assert "selhip_nj_join_t" in header and " 2l. " in header
    assert pkg.NJ_DTYPE == NM.NJ_DTYPE and pkg.NJ_DTYPE.itemsize == 24
    assert [pkg.NJ_DTYPE.fields[f][1] for f in ("a", "b", "len_a", "len_b")] == [0, 4, 8, 16]
    for name in ("neighbor_joining", "nj_newick", "nj_table", "nj_from_filelist", "NJ_DTYPE"):
        assert name in pkg.__all__
    assert hasattr(pkg.Selector, "neighbor_joining")


def test_newick_and_table():
    # ((A:1,B:2):3,C:4) joined with (D, E): records in slot space; slot 0 holds (A, B), then ((A, B), C); slot 3 holds (D, E)
    joins = np.array([(0, 1, 1.0, 2.0), (3, 4, 0.5, -0.25), (0, 2, 3.0, 4.0), (0, 3, 0.125, 0.125)], dtype=pkg.NJ_DTYPE)
    names = ["A", "B", "C c", "D", "E'"]
    assert pkg.nj_newick(joins, names) == "(((A:1,B:2):3,'C c':4):0.125,(D:0.5,'E''':-0.25):0.125);\n"
    assert pkg.nj_newick(joins[:0], ["only"]) == "only;\n" and pkg.nj_newick(joins[:0], []) == ";\n"
    assert pkg.nj_newick(joins[:1], ["x", "y"]) == "(x:1,y:2);\n"
    assert pkg.nj_table(names, joins[:2]) == "A\tB\t1.000000\t2.000000\nD\tE'\t0.500000\t-0.250000\n"
    deep = np.array([(0, s + 1, 1.0, 1.0) for s in range(3000)], dtype=pkg.NJ_DTYPE)      # a chain: no recursion
    assert pkg.nj_newick(deep, [str(g) for g in range(3001)]).count("(") == 3000


def test_argument_checks():
    for measure in ("union", "containment", "intersection", "smh_matches"):
        with pytest.raises(ValueError, match="symmetric"):
            pkg.nj_from_filelist("/nonexistent/list.txt", 512, measure=measure)
    with pytest.raises(ValueError, match="aux_bytes"):
        pkg.nj_from_filelist("/nonexistent/list.txt", 0, measure="smh_jaccard")
    lib = pkg.hip_lib()                                                       # checked before a device is touched
    for args, text in (((None, 4, 3, None), "ld >= n"), ((None, -1, 4, None), "0 <= n"), ((None, 4, 4, None), "non-null"),
                       ((12, 1, 1, None), "8-byte aligned"), ((8, 1, 1, 20), "8-byte aligned records")):
        assert lib.selhip_neighbor_joining(*args, None, None) == -1 and text in lib.selhip_last_error(None).decode(), text
    f = C.c_int64(-5)
    for n in (0, 1):
        assert lib.selhip_neighbor_joining(None, n, n, None, C.byref(f), None) == 0 and f.value == 0
    assert lib.selhip_ctx_neighbor_joining(None, 0, None, None) == -1


def test_cli_refusals():
    sel = str(BIN / "selection")
    run = lambda args: subprocess.run([sel] + args, capture_output=True, text=True)
    lst, tree, nj = ["-l", "/nonexistent/list.txt"], ["-N", "/nonexistent/dir/tree.nwk"], ["-X", "nj"]
    for args, word in ((lst + nj, "-X (the linkage method) is an option of -N / -J"), (lst + tree + ["-X", "bionj"], "not 'bionj' (or nj: the neighbour-joining tree)"),
                       (lst + tree + nj + ["-q", "/nonexistent/q.txt"], "cannot be combined with -q"), (lst + tree + nj + ["-K", "3"], "cannot be combined with -K"),
                       (lst + tree + nj + ["-h", "0.9"], "cannot be combined with -h"), (lst + tree + nj + ["-U"], "symmetric similarity"),
                       (lst + tree + nj + ["-S", "containment"], "symmetric similarity"), (lst + tree + nj + ["-E", "smh"], "give their size with -a"),
                       (tree + nj, "need the list of genomes (-l)")):
        out = run(args)
        assert out.returncode == 2 and out.stdout == "" and word in out.stderr, (args, out)
    for args in (lst + tree + nj, lst + ["-J", "/nonexistent/dir/j.tsv"] + nj + ["-E", "smh", "-a", "512"], lst + tree + nj + ["-S", "max_containment"]):
        out = run(args)                                                       # legal: they get as far as reading the list
        assert out.returncode == 1 and out.stdout == "" and "-N / -J: " in out.stderr and "cannot" not in out.stderr, (args, out)
    assert "-X average|complete|weighted|single|nj" in run(["-x"]).stdout
