"""Top-k of the query passes (selhip_ctx_set_query_topk, include/selection_hip.h section 2b), the parts that need no GPU: the new
symbols and wrappers, the CLI's -k usage errors, and topk_reference -- the numpy restatement of the contract that the GPU tests
(test_query_topk_gpu.py) compare the device's reduced list with -- on hand-made record lists."""
import inspect
import subprocess

import numpy as np

from conftest import ROOT

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import PAIR_DTYPE, Selector

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
SIGN = np.uint64(1 << 63)


def sort_key(jaccard):
    """u64 whose unsigned order is the IEEE total order of the doubles: bits ^ 2^63 for a clear sign bit, ~bits for a set one"""
    b = np.ascontiguousarray(jaccard, dtype=np.float64).view(np.uint64)
    return np.where((b & SIGN) != 0, ~b, b ^ SIGN)


def topk_reference(S, K):
    """topk(S, K) in ranked order: query rank ascending; within a query key(J) descending, ties by ascending database rank; the first
    min(L_i, K) records of every query"""
    S = np.ascontiguousarray(S, dtype=PAIR_DTYPE)
    R = S[np.lexsort((S["k"], ~sort_key(S["jaccard"]), S["i"]))]
    at = np.arange(len(R))
    first = np.ones(len(R), dtype=bool)
    first[1:] = R["i"][1:] != R["i"][:-1]
    pos = at - np.maximum.accumulate(np.where(first, at, 0))             # position inside the query's segment
    return R[pos < K]


def records(rows):
    out = np.zeros(len(rows), dtype=PAIR_DTYPE)
    for n, (i, k, j) in enumerate(rows):
        out[n] = (i, k, j)
    return out


def triples(recs):
    return [(int(r["i"]), int(r["k"]), float(r["jaccard"])) for r in recs]


def test_symbols_and_wrappers():
    lib = pkg.hip_lib()
    assert lib.selhip_ctx_set_query_topk is not None and lib.selhip_ctx_fetch_ranked is not None
    header = (ROOT / "include" / "selection_hip.h").read_text()
    assert "#define SELHIP_TOPK_MAX 1024" in header and pkg.TOPK_MAX == 1024
    for word in ("selhip_ctx_set_query_topk", "selhip_ctx_fetch_ranked", '"query_topk"', '"query_topk_lds_cap"', '"topk"',
                 "not an unconditional k-nearest-neighbour search", "For exact nearest neighbours use SELHIP_CRIT_NONE"):
        assert word in header, word
    assert callable(Selector.set_query_topk) and callable(Selector.fetch_ranked)
    assert inspect.signature(Selector.run_queries).parameters["top_k"].default is None
    assert inspect.signature(pkg.query_from_filelists).parameters["top_k"].default == 0


def test_sort_key_is_the_total_order():
    vals = np.array([-np.inf, -1.0, -0.5, -1e-300, -0.0, 0.0, 1e-300, 0.25, 0.5, 1.0, np.inf])
    keys = sort_key(vals)
    assert np.all(keys[1:] > keys[:-1])                                  # strictly ascending, -0.0 below +0.0
    back = np.where((keys & SIGN) != 0, keys ^ SIGN, ~keys)              # the inverse: the same two cases, told apart by the key's top bit
    assert np.array_equal(back, vals.view(np.uint64))


def test_reference_negative_and_infinite():
    S = records([(0, 4, -0.25), (0, 1, 0.5), (0, 7, np.inf), (0, 2, -0.75), (0, 9, 0.0), (0, 3, -0.0)])
    assert triples(topk_reference(S, 6)) == [(0, 7, np.inf), (0, 1, 0.5), (0, 9, 0.0), (0, 3, -0.0), (0, 4, -0.25), (0, 2, -0.75)]
    got = topk_reference(S, 4)
    assert [int(k) for k in got["k"]] == [7, 1, 9, 3]
    assert np.signbit(got["jaccard"][3]) and not np.signbit(got["jaccard"][2])      # +0.0 ranks before -0.0, bits kept


def test_reference_ties_take_the_smaller_rank():
    S = records([(2, 8, 0.5), (2, 3, 0.5), (2, 5, 0.5), (2, 1, 0.25), (2, 9, 0.75)])
    assert triples(topk_reference(S, 1)) == [(2, 9, 0.75)]
    assert triples(topk_reference(S, 2)) == [(2, 9, 0.75), (2, 3, 0.5)]
    assert triples(topk_reference(S, 3)) == [(2, 9, 0.75), (2, 3, 0.5), (2, 5, 0.5)]
    assert triples(topk_reference(S, 4)) == [(2, 9, 0.75), (2, 3, 0.5), (2, 5, 0.5), (2, 8, 0.5)]


def test_reference_segment_lengths():
    """L < K, L = K and L = K + 1, with an empty segment (query 1) between two others; the input order does not matter"""
    K = 3
    S = records([(0, 1, 0.1), (0, 2, 0.2),                               # L = 2 < K
                 (2, 5, 0.3), (2, 6, 0.1), (2, 7, 0.2),                  # L = 3 = K
                 (3, 1, 0.4), (3, 2, 0.1), (3, 3, 0.3), (3, 4, 0.2)])    # L = 4 = K + 1
    want = [(0, 2, 0.2), (0, 1, 0.1), (2, 5, 0.3), (2, 7, 0.2), (2, 6, 0.1), (3, 1, 0.4), (3, 3, 0.3), (3, 4, 0.2)]
    assert triples(topk_reference(S, K)) == want
    assert triples(topk_reference(S[np.random.default_rng(1).permutation(len(S))], K)) == want
    assert 1 not in topk_reference(S, K)["i"]
    assert len(topk_reference(S[:0], K)) == 0
    assert triples(topk_reference(S, 1024)) == triples(topk_reference(S, 4))


def test_cli_topk_usage_errors():
    sel = str(BIN / "selection")
    out = subprocess.run([sel, "-l", "/nonexistent/list.txt", "-k", "3"], capture_output=True, text=True)
    assert out.returncode == 2 and out.stdout == "" and "-k" in out.stderr and "needs -q" in out.stderr
    for bad in ("0", "1025", "-1", "many"):
        out = subprocess.run([sel, "-l", "/nonexistent/db.txt", "-q", "/nonexistent/q.txt", "-k", bad], capture_output=True, text=True)
        assert out.returncode == 2 and out.stdout == "" and "-k must be in 1..1024" in out.stderr, bad
    # a legal -k gets as far as reading the lists
    out = subprocess.run([sel, "-l", "/nonexistent/db.txt", "-q", "/nonexistent/q.txt", "-k", "1024"], capture_output=True, text=True)
    assert out.returncode == 1 and "-k" not in out.stderr
    assert "-k" in subprocess.run([sel, "-x"], capture_output=True, text=True).stdout
