"""ALGO_INDEX of the query passes, the parts that need no GPU: the exported constant, the CLI's handling of `-A index`, and a numpy
restatement of the probe's emit rule (kernel_query_index.cuh): a pair is taken from the run of its FIRST equal band only."""
import re
import subprocess

import numpy as np

from conftest import ROOT

import cuda_selection_criteria_amd as pkg

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"


def test_algo_index_constant():
    assert pkg.ALGO_INDEX == 4
    assert "ALGO_INDEX" in pkg.__all__
    header = (ROOT / "include" / "selection_hip.h").read_text()
    m = re.search(r"^#define\s+SELHIP_ALGO_INDEX\s+(\d+)", header, re.M)
    assert m and int(m.group(1)) == 4


def test_cli_usage_mentions_index():
    out = subprocess.run([str(BIN / "selection"), "-x"], capture_output=True, text=True)
    assert out.returncode == 0 and "index" in out.stdout


def test_cli_index_needs_query_list(tmp_path):
    out = subprocess.run([str(BIN / "selection"), "-l", "x", "-A", "index", "-h", "0.9", "-a", "512"], cwd=tmp_path,
                         capture_output=True, text=True)
    assert out.returncode != 0
    assert "-q" in out.stderr and "index" in out.stderr


def _emit(sig_q, sig_d):
    """the probe, restated: per band the database signatures stably sorted with their ranks; per (query, band) the run of the
    query's signature by two binary searches; a run entry d is emitted iff no earlier band of (q, d) is equal"""
    n_q, nb = sig_q.shape
    out = []
    for b in range(nb):
        order = np.argsort(sig_d[:, b], kind="stable")
        keys = sig_d[order, b]
        for q in range(n_q):
            s, e = np.searchsorted(keys, sig_q[q, b], "left"), np.searchsorted(keys, sig_q[q, b], "right")
            run = order[s:e]
            assert np.all(np.diff(run) > 0)                              # stable sort: ranks ascend inside a run
            for d in run:
                if not np.any(sig_q[q, :b] == sig_d[d, :b]):
                    out.append((q, int(d)))
    return out


def test_emit_rule_each_pair_once():
    rng = np.random.default_rng(2024)
    for nb, n_q, n_d in ((8, 40, 300), (16, 25, 500), (64, 10, 200)):
        sig_q = rng.integers(0, 2**32, size=(n_q, nb), dtype=np.uint64).astype(np.uint32)
        sig_d = rng.integers(0, 2**32, size=(n_d, nb), dtype=np.uint64).astype(np.uint32)
        # planted equal bands, several per pair
        for _ in range(120):
            q, d = rng.integers(n_q), rng.integers(n_d)
            bands = rng.choice(nb, size=rng.integers(1, 5), replace=False)
            sig_d[d, bands] = sig_q[q, bands]
        # planted long runs: many database genomes (and a few queries) identical in every band, others in some bands
        sig_d[rng.choice(n_d, 70, replace=False)] = sig_q[0]
        sig_q[1:4] = sig_q[0]
        sig_d[rng.choice(n_d, 50, replace=False), nb // 2:] = sig_q[5, nb // 2:]
        want = {(int(q), int(d)) for q, d in zip(*np.nonzero((sig_q[:, None, :] == sig_d[None, :, :]).any(axis=2)))}
        got = _emit(sig_q, sig_d)
        assert len(want) > 4 * 70
        assert len(got) == len(set(got))                                 # no pair twice
        assert set(got) == want                                          # every pair with an equal band, and nothing else
