"""Top-k of the all-pairs passes (selhip_ctx_set_allpairs_topk, include/selection_hip.h section 2), the parts that need no GPU: the new
symbol and wrappers, the header's words, the CLI's -K usage errors, and nbr_reference -- the numpy restatement of the contract that
the GPU tests (test_allpairs_topk_gpu.py) compare the device's reduced list with -- on hand-made record lists."""
import inspect
import subprocess

import numpy as np

from conftest import ROOT
from test_query_topk_host import records, topk_reference, triples

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import PAIR_DTYPE, Selector

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"


def swapped(S):
    """every record {i, k, J} as {k, i, J}"""
    out = np.ascontiguousarray(S, dtype=PAIR_DTYPE).copy()
    out["i"], out["k"] = S["k"], S["i"]
    return out


def nbr_reference(S, K):
    """nbr(S, K) in ranked order: the directed list (every record once per member, {i = owner, k = partner, J}), every owner's
    first min(L_g, K) records by (key(J) descending, partner ascending), owners ascending"""
    S = np.ascontiguousarray(S, dtype=PAIR_DTYPE)
    return topk_reference(np.concatenate([S, swapped(S)]), K)


def test_symbols_and_wrappers():
    lib = pkg.hip_lib()
    assert lib.selhip_ctx_set_allpairs_topk is not None                    # (fails before this entry point existed)
    assert "selhip_ctx_set_allpairs_topk" in pkg._lib.HIP_SYMBOLS
    assert callable(Selector.set_allpairs_topk)
    run = inspect.signature(Selector.run).parameters
    assert run["top_k"].default is None and run["fetch"].default is True
    assert inspect.signature(pkg.select_from_filelist).parameters["top_k"].default == 0
    src = (ROOT / "cuda_selection_criteria_amd" / "csrc" / "abi_context.inc").read_text()
    assert '"allpairs_topk"' in src


def test_header_words():
    header = (ROOT / "include" / "selection_hip.h").read_text()
    for word in ("int selhip_ctx_set_allpairs_topk(selhip_ctx* ctx, int k);", '"allpairs_topk"', "DIRECTED LIST", "{owner k, partner i, J}",
                 "a.partner < b.partner", "LARGER than |S|", "12 bytes per directed record", "2^31 - 1 directed records",
                 "selhip_ctx_copy_results_framed / _framed_async return SELHIP_E_STATE", "stats[2] stays |S|",
                 # the query top-k's sentences stay
                 "not an unconditional k-nearest-neighbour search", "For exact nearest neighbours use SELHIP_CRIT_NONE",
                 "all-pairs passes, selhip_multi_select and selhip_ooc_select never cut"):
        assert word in header, word


def test_reference_owner_from_both_sides():
    """genome 2 is the larger member of two records and the smaller member of two"""
    S = records([(0, 2, 0.5), (1, 2, 0.9), (2, 3, 0.7), (2, 5, 0.1), (0, 1, 0.3)])
    got = nbr_reference(S, 3)
    assert triples(got[got["i"] == 2]) == [(2, 1, 0.9), (2, 3, 0.7), (2, 0, 0.5)]
    assert triples(nbr_reference(S, 1)) == [(0, 2, 0.5), (1, 2, 0.9), (2, 1, 0.9), (3, 2, 0.7), (5, 2, 0.1)]
    assert 4 not in got["i"]                                               # a genome that owns nothing
    # (1, 2) is kept by both members, (2, 5) by genome 5 only, (0, 1) by nobody at K = 1
    one = triples(nbr_reference(S, 1))
    assert (1, 2, 0.9) in one and (2, 1, 0.9) in one and (5, 2, 0.1) in one and (2, 5, 0.1) not in one
    assert (0, 1, 0.3) not in one and (1, 0, 0.3) not in one


def test_reference_tie_across_the_cut():
    S = records([(1, 4, 0.5), (4, 9, 0.5), (4, 6, 0.5), (0, 4, 0.25), (4, 7, 0.75)])
    own4 = lambda K: triples(nbr_reference(S, K)[nbr_reference(S, K)["i"] == 4])
    assert own4(1) == [(4, 7, 0.75)]
    assert own4(2) == [(4, 7, 0.75), (4, 1, 0.5)]                          # the smaller partner wins, whichever side it came from
    assert own4(3) == [(4, 7, 0.75), (4, 1, 0.5), (4, 6, 0.5)]
    assert own4(4) == [(4, 7, 0.75), (4, 1, 0.5), (4, 6, 0.5), (4, 9, 0.5)]


def test_reference_whole_list_and_empty():
    S = records([(0, 1, 0.1), (0, 2, 0.2), (1, 2, 0.3), (2, 3, -0.5)])
    full = nbr_reference(S, 1024)                                          # K beyond every segment: both directions of everything
    assert len(full) == 2 * len(S)
    assert sorted(triples(full)) == sorted(triples(S) + triples(swapped(S)))
    assert np.array_equal(full["i"], np.sort(full["i"]))
    assert triples(full[full["i"] == 2]) == [(2, 1, 0.3), (2, 0, 0.2), (2, 3, -0.5)]
    assert np.array_equal(nbr_reference(S[np.random.default_rng(2).permutation(len(S))], 2), nbr_reference(S, 2))
    empty = nbr_reference(S[:0], 5)
    assert len(empty) == 0 and empty.dtype == PAIR_DTYPE


def test_cli_allpairs_topk_usage_errors():
    sel = str(BIN / "selection")
    base = [sel, "-l", "/nonexistent/list.txt", "-K", "3"]
    for flag, arg in (("-q", "/nonexistent/q.txt"), ("-g", "2"), ("-B", "100"), ("-o", "/nonexistent/out.selr"), ("-r", "/nonexistent/in.selr")):
        out = subprocess.run(base + [flag, arg], capture_output=True, text=True)
        assert out.returncode == 2 and out.stdout == "" and "-K" in out.stderr and flag in out.stderr, (flag, out.stderr)
        if flag == "-q":
            assert "-k" in out.stderr                                      # the per-query cut is the other option
    for bad in ("0", "1025", "x"):
        out = subprocess.run([sel, "-l", "/nonexistent/list.txt", "-K", bad], capture_output=True, text=True)
        assert out.returncode == 2 and out.stdout == "" and "-K must be in 1..1024" in out.stderr, bad
    # a legal -K gets as far as reading the list
    out = subprocess.run([sel, "-l", "/nonexistent/list.txt", "-K", "1024"], capture_output=True, text=True)
    assert out.returncode == 1 and out.stdout == "" and "-K" not in out.stderr
    assert "-K" in subprocess.run([sel, "-x"], capture_output=True, text=True).stdout
    # -k keeps its meaning and its message
    out = subprocess.run([sel, "-l", "/nonexistent/list.txt", "-k", "3"], capture_output=True, text=True)
    assert out.returncode == 2 and out.stdout == "" and "needs -q" in out.stderr
