"""The all-pairs top-k in row rounds (selhip_ctx_set_topk_rounds), what needs no GPU: the numpy model of the rounds
(tests/topk_rounds_model.py) against nbr_reference on record sets with heavy ties, the header's contract, the symbols, the Python names
and every refusal of the front ends."""
import ctypes as C
import inspect
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import smhv_model as V
import topk_rounds_model as R
from test_allpairs_topk_host import nbr_reference
from test_smhv_gpu import case, tied_rows

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import PAIR_DTYPE, Selector

SEL = str(ROOT / "cuda_selection_criteria_amd" / "bin" / "selection")
LIB = ROOT / "cuda_selection_criteria_amd" / "lib" / "libselhip.so"


def tuples(rec):
    return list(zip(rec["i"].tolist(), rec["k"].tolist(), np.asarray(rec["jaccard"], dtype=np.float64).view(np.uint64).tolist()))


def random_records(n, density, levels, seed):
    """records {i < k, value} of a random graph on n owners whose values take `levels` distinct numbers: ties everywhere"""
    rng = np.random.default_rng(seed)
    i, k = np.triu_indices(n, 1)
    keep = rng.random(len(i)) < density
    rec = np.zeros(int(keep.sum()), dtype=PAIR_DTYPE)
    rec["i"], rec["k"] = i[keep], k[keep]
    rec["jaccard"] = rng.integers(1, levels + 1, len(rec)) / np.float64(levels)
    return rec[rng.permutation(len(rec))]


@pytest.mark.parametrize("n,density,levels", [(1, 1.0, 3), (2, 1.0, 1), (37, 0.5, 2), (130, 0.9, 4), (300, 0.3, 3), (300, 1.0, 5)])
def test_model_is_the_one_shot_cut(n, density, levels):
    S = random_records(n, density, levels, 19 * n + levels)
    n_pruned = 0
    for K in (1, 3, 10, 400):
        ref = nbr_reference(S, K)
        for rows in (1, 2, 7, 64, n, n + 5):
            C_, admitted, per_round, lists = R.replay(S, n, K, rows)
            assert tuples(C_) == tuples(ref), (n, K, rows)
            assert admitted <= len(S) and len(per_round) == -(-n // rows)
            assert all(len(c) <= n * K for c in lists)
            n_pruned += admitted < len(S)
            if rows >= n:
                assert admitted == len(S)                                  # one round: nothing to prune with
    if n >= 130:
        assert n_pruned > 0


def test_model_row_range_and_thresholds():
    n, K = 90, 2
    S = random_records(n, 0.8, 3, 5)
    part = S[(S["i"] >= 5) & (S["i"] < n - 3)]
    C_, admitted, per_round, lists = R.replay(S, n, K, 16, rows=(5, n - 3))
    assert tuples(C_) == tuples(nbr_reference(part, K)) and len(per_round) == -(-(n - 8) // 16)
    # thresholds only rise, and a full owner's threshold is its K-th value
    prev = np.full(n, -np.inf)
    for c in lists:
        thr = R.thresholds(c, n, K)
        assert np.all(thr >= prev)
        prev = thr
    owners, counts = np.unique(C_["i"], return_counts=True)
    assert np.all(np.isfinite(prev[owners[counts == K]])) and np.all(np.isinf(prev[np.setdiff1d(np.arange(n), owners[counts == K])]))


@pytest.mark.parametrize("m", [128, 100])
def test_model_prunes_the_dense_case(m):
    """the case the GPU test asserts on: n = 257, K = 1, R = 8 on the planted groups of test_smhv_gpu.case admits strictly fewer records
    than |S|.  (On tied_rows the model admits EVERY record at every R: a row's equals are its neighbours in rank, so the larger member
    of a pair of strangers has met none of its own group when the pair is counted and still stands at the value every pair has; a
    tie is admitted.  Stated here so that nobody looks for pruning there.)"""
    n = 257
    aux, cards = case(n, m)
    S, st = V.expected(aux, cards, -1.0, False, "jaccard", c_min=1)
    C_, admitted, per_round, _ = R.replay(S, n, 1, 8)
    assert tuples(C_) == tuples(nbr_reference(S, 1))
    assert 0 < admitted < len(S) and len(per_round) == 33
    assert per_round[0] == int((S["i"] < 8).sum())                        # the first round has no thresholds yet
    aux = tied_rows(n, m, 5 * m)
    S, st = V.expected(aux, cards, -1.0, False, "jaccard", c_min=1)
    assert len(S) == n * (n - 1) // 2
    C_, admitted, per_round, _ = R.replay(S, n, 1, 8)
    assert tuples(C_) == tuples(nbr_reference(S, 1)) and admitted == len(S)


def test_header_words():
    header = (ROOT / "include" / "selection_hip.h").read_text()
    for word in ("int selhip_ctx_set_topk_rounds(selhip_ctx* ctx, int64_t rows);", "#define SELHIP_TOPK_ROUNDS_AUTO (-1)", "ROW ROUNDS",
                 "V >= thr[i] || V >= thr[k']", "R n <= 2^27", '"topk_rounds_used"', '"topk_admitted_lo"', '"topk_admitted_hi"',
                 "not the admitted count", "largest attempt count of any round"):
        assert word in header, word
    plan = (ROOT / "cuda_selection_criteria_amd" / "csrc" / "host_plan.hpp").read_text()
    assert plan.count("1ll << 27") == 1                                    # the automatic rule, stated once


def test_symbols_and_wrappers():
    assert pkg._lib.TOPK_ROUNDS_AUTO == -1 and pkg.TOPK_ROUNDS_AUTO == -1
    assert "selhip_ctx_set_topk_rounds" in pkg._lib.HIP_SYMBOLS
    assert pkg.hip_lib().selhip_ctx_set_topk_rounds is not None
    exported = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    assert " T selhip_ctx_set_topk_rounds" in exported
    assert callable(Selector.set_topk_rounds)
    assert inspect.signature(Selector.run).parameters["rounds"].default is None
    assert inspect.signature(pkg.select_from_filelist).parameters["top_k_rounds"].default == 0


def test_setter_refusals(tmp_path):
    # without a context every value answers SELHIP_E_BADARG, and the wrapper refuses -2 before it gets there
    lib = pkg.hip_lib()
    for rows in (0, 5, -1, -2):
        assert lib.selhip_ctx_set_topk_rounds(None, C.c_int64(rows)) == -1
    from cuda_selection_criteria_amd.selection import topk_rounds_code
    assert topk_rounds_code("auto") == -1 and topk_rounds_code(-1) == -1 and topk_rounds_code(0) == 0 and topk_rounds_code(64) == 64
    for bad in (-2, -100, "Auto", "", 1.5, True, None):
        with pytest.raises(ValueError, match="rounds"):
            topk_rounds_code(bad)
    missing = str(tmp_path / "no_such_list.txt")
    ok = dict(mode=pkg.MODE_SMH, criterion="smh_c", min_matches=1, estimator="smh", top_k=3)
    with pytest.raises(RuntimeError, match="selhost error"):               # accepted: gets as far as reading the list
        pkg.select_from_filelist(missing, -1.0, 1024, top_k_rounds=2, **ok)
    with pytest.raises(RuntimeError, match="selhost error"):
        pkg.select_from_filelist(missing, -1.0, 1024, top_k_rounds="auto", **ok)
    for change in (dict(top_k=0), dict(estimator="hll"), dict(criterion="smh_a", min_matches=None, estimator="hll")):
        with pytest.raises(ValueError, match="top_k_rounds"):
            pkg.select_from_filelist(missing, -1.0, 1024, top_k_rounds=2, **{**ok, **change})
    with pytest.raises(ValueError, match="rounds"):
        pkg.select_from_filelist(missing, -1.0, 1024, top_k_rounds=-2, **ok)


def run(args):
    return subprocess.run([SEL] + args, capture_output=True, text=True)


def test_cli_refusals():
    base = ["-l", "/nonexistent/list.txt", "-h", "-1", "-n", "-c", "smh_c", "-C", "1", "-a", "1024", "-V", "smh"]
    for args, word in ((base + ["-R", "2"], "-R (the rows per round) is an option of -K"),
                       (base + ["-R", "auto"], "-R (the rows per round) is an option of -K"),
                       (["-q", "/nonexistent/q.txt"] + base + ["-k", "3", "-R", "2"], "-R (the rows per round of -K) cannot be combined with -q"),
                       (base + ["-p", "/nonexistent/pairs.txt", "-R", "2"], "cannot be combined with -p"),
                       (["-l", "/nonexistent/list.txt", "-M", "/nonexistent/out.tsv", "-R", "2"], "-R (the rows per round of -K) cannot be combined with -M"),
                       (base + ["-K", "3", "-R", "2", "-g", "2"], "-g"),
                       (base + ["-K", "3", "-R", "2", "-B", "100"], "-B"),
                       (base + ["-K", "3", "-R", "0"], "-R must be a number of rows >= 1 or auto"),
                       (base + ["-K", "3", "-R", "-2"], "-R must be a number of rows >= 1 or auto"),
                       (base + ["-K", "3", "-R", "7x"], "-R must be a number of rows >= 1 or auto"),
                       (base + ["-K", "3", "-R", ""], "-R must be a number of rows >= 1 or auto"),
                       (base[:-2] + ["-K", "3", "-R", "2"], "-R needs -c smh_c -V smh"),
                       (["-l", "/nonexistent/list.txt", "-h", "0.9", "-K", "3", "-R", "2"], "-R needs -c smh_c -V smh")):
        out = run(args)
        assert out.returncode == 2 and out.stdout == "" and word in out.stderr, (args, out)
        assert "nonexistent" not in out.stderr and "input file" not in out.stderr, (args, out.stderr)
    # accepted: the run gets as far as the list
    for extra in (["-K", "3", "-R", "2"], ["-K", "3", "-R", "auto"], ["-K", "10", "-R", "100000"]):
        out = run(base + extra)
        assert out.returncode not in (0, 2) and "No valid input file provided" in out.stderr, (extra, out)
    usage = run(["-x"]).stdout
    assert "-R rows|auto" in usage
