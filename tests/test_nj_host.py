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


def bits(x):
    return np.array(x, dtype=np.float64).view(np.uint64).tolist()


@pytest.mark.parametrize("n", (5, 64, 130))
def test_first_k_is_the_prefix_of_the_full_run(n):
    for vname in ("distinct", "levels"):
        dist = NM.value_sets(n)[vname]
        full = NM.neighbor_joining(dist)
        for k in (0, 1, 3, NM.PREFIX, n - 2, n - 1, n + 5):
            part = NM.neighbor_joining(dist, first=k)
            assert len(part) == min(k, n - 1) and part.tobytes() == full[:k].tobytes(), (vname, k)
    for tiny in (0, 1):
        assert len(NM.neighbor_joining(np.zeros((tiny, tiny)), first=4)) == 0


def test_signed_zeros_are_mirrored_by_copy():
    """section 2l evaluated by hand, not by the model.  n = 2: len_a = len_b = 0.5 * -0.0 = -0.0.  Five slots with -0.0 in every cell of
    the upper triangle: R is +0.0 (a sum onto +0.0), every q is ((3 * -0.0) - 0.0) - 0.0 = -0.0, the first pair is (0, 1), len_a =
    0.5 * -0.0 + (0.0 - 0.0) / 6 = -0.0 + 0.0 = +0.0 and len_b = -0.0 - (+0.0) = -0.0"""
    two = NM.neighbor_joining(np.array([[0.0, -0.0], [0.0, 0.0]]))
    assert (int(two["a"][0]), int(two["b"][0])) == (0, 1) and bits([two["len_a"][0], two["len_b"][0]]) == bits([-0.0, -0.0])
    five = NM.neighbor_joining(np.triu(np.full((5, 5), -0.0), 1))
    assert (int(five["a"][0]), int(five["b"][0])) == (0, 1) and bits([five["len_a"][0], five["len_b"][0]]) == bits([0.0, -0.0])
    assert bits([0.0]) != bits([-0.0])
    m = NM.mirrored(np.array([[7.0, -0.0, 1.0], [5.0, 7.0, 0.0], [5.0, 5.0, 7.0]]))
    assert bits(m) == bits([[0.0, -0.0, 1.0], [-0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    for n in NM.ZERO_SIZES:                                                   # the sets of the device test do hold negative zeros in the triangle
        for vname, dist in NM.zero_sets(n).items():
            negative = np.signbit(dist[np.triu_indices(n, 1)][dist[np.triu_indices(n, 1)] == 0.0])
            assert negative.all() if vname == "all" else n < 5 or (negative.any() and not negative.all()), (n, vname)


def test_overflow_sets_end_with_ordered_pairs():
    """finite cells, sums that are not: NaN q counts as +inf, and where every q is +inf the first two active slots are joined"""
    seen = {"nan": 0, "inf": 0, "finite": 0}
    for n in NM.OVERFLOW_SIZES:
        for vname, dist in NM.overflow_sets(n).items():
            assert np.isfinite(dist).all()
            joins = NM.neighbor_joining(dist)
            assert len(joins) == n - 1 and np.all(joins["a"] < joins["b"]) and np.all(joins["a"] >= 0) and np.all(joins["b"] < n), (n, vname)
            assert NM.join_splits(joins, n) is not None                      # every b was still active: the records describe a tree
            if vname == "huge" and n >= 65:
                assert np.isnan(joins["len_a"]).all() and np.isnan(joins["len_b"]).all()
            if vname == "mixed":
                for x in np.concatenate([joins["len_a"], joins["len_b"]]):
                    seen["nan" if np.isnan(x) else "inf" if np.isinf(x) else "finite"] += 1
    assert min(seen.values()) > 0, seen
    assert sorted(NM.overflow_sets(65)) == ["huge", "mixed"] and sorted(NM.overflow_sets(130)) == ["huge"]


@pytest.mark.parametrize("n", NM.TRIP_SIZES)
def test_premises_of_the_trip_cases(n):
    """what tests/test_nj_gpu.py rests on at n = 1 024 j + 7: the forged pair is record 0 and its row lies in the last trip of the pick's
    walk over the list; on "equal" every q of the first join ties and the records are (0, 1), (0, 2), ...; on "twins" the smallest q is
    shared by TWIN and the forged pair alone, which the pick meets in different waves and trips, and TWIN is record 0"""
    p, q = NM.forged_pair(n)
    trips = -(-n // NM.LANES)
    assert n % NM.LANES == 7 and trips == NM.TRIP_SIZES.index(n) + 2 and p // NM.LANES == trips - 1 and (p, q) == (n - 4, n - 2)
    first = NM.neighbor_joining(NM.forged(n), first=NM.PREFIX)
    assert len(first) == NM.PREFIX and (int(first["a"][0]), int(first["b"][0])) == (p, q)
    sets = NM.tie_sets(n)
    upper = np.triu_indices(n, 1)
    assert len(np.unique(NM.first_q(sets["equal"])[upper])) == 1
    equal = NM.neighbor_joining(sets["equal"], first=NM.PREFIX)
    assert np.all(equal["a"] == 0) and np.array_equal(equal["b"], np.arange(1, NM.PREFIX + 1))
    fq = NM.first_q(sets["twins"])
    at = sorted(zip(*(x.tolist() for x in np.nonzero(fq == fq.min()))))
    assert at == [NM.TWIN, (p, q)], at
    assert NM.TWIN[0] // NM.WAVE == 1 and (p % NM.LANES) // NM.WAVE == 0      # wave 1 in the first trip, wave 0 in the last
    twins = NM.neighbor_joining(sets["twins"], first=NM.PREFIX)
    assert (int(twins["a"][0]), int(twins["b"][0])) == NM.TWIN and (int(twins["a"][1]), int(twins["b"][1])) == (p, q)
    assert len(np.unique(sets["levels"])) == 3


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
