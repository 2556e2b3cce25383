"""Criterion "none" (SELHIP_CRIT_NONE), the parts that need no GPU: the constant and its documentation, the Python wrappers and the CLI
taking the name, and the committed reference goldens (tests/golden/make_golden_exhaustive.py: the reference's own `-c smh_a` run on
identical SuperMinHash sketches) against the oracle's flat-sketch output -- the trick the GPU tests take their expected values from."""
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import FP_FMA, FP_STRICT, PAIR_DTYPE

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
EXP = GOLDEN / "expected"
INVALID = "Option -c invalid. The accepted criteria are hll_a, hll_an and smh_a."


def flat_oracle_select(oracle, hll, cards, tau, use_cb, fp):
    """the exhaustive loop from the oracle: smh_a on SuperMinHash sketches that are all equal is true for every pair"""
    aux = np.zeros((hll.shape[0], 4), dtype=np.uint64)
    oracle.set_fma(fp)
    try:
        pairs, st = oracle.select(hll, aux, cards, tau, 1, 4, use_cb=use_cb, criterion=0)
    finally:
        oracle.set_fma(1)
    assert st["survivors"] == st["evaluated"]
    out = np.zeros(len(pairs), dtype=PAIR_DTYPE)
    out["i"], out["k"], out["jaccard"] = pairs["i"], pairs["k"], pairs["jacc"]
    return out, st


def test_constant_and_header():
    assert pkg.CRIT_NONE == 4
    assert (pkg.CRIT_SMH_A, pkg.CRIT_HLL_A, pkg.CRIT_HLL_AN, pkg.CRIT_HLL_A_SMH_A) == (0, 1, 2, 3)
    header = (ROOT / "include" / "selection_hip.h").read_text()
    assert "#define SELHIP_CRIT_NONE         4" in header
    for word in ("dense_fused", "dense_route_used", '"dense"'):
        assert word in header, word


def test_wrappers_accept_none(tmp_path):
    missing = str(tmp_path / "no_such_list.txt")
    # "none" gets as far as reading the list; any other unknown name is refused with the reference's message, as before
    with pytest.raises(RuntimeError, match="selhost error"):
        pkg.select_from_filelist(missing, 0.9, 0, criterion="none")
    with pytest.raises(RuntimeError, match="selhost error"):
        pkg.query_from_filelists(missing, missing, 0.9, 0, criterion="none")
    with pytest.raises(ValueError) as e:
        pkg.select_from_filelist(missing, 0.9, 32, criterion="cb")
    assert str(e.value) == INVALID
    with pytest.raises(ValueError) as e:
        pkg.query_from_filelists(missing, missing, 0.9, 32, criterion="cb")
    assert str(e.value) == INVALID


def test_cli_knows_none():
    sel = str(BIN / "selection")
    out = subprocess.run([sel, "-l", "/nonexistent/list.txt", "-h", "0.9", "-c", "none"], capture_output=True, text=True)
    assert out.returncode != 0 and "No valid input file provided" in out.stderr and INVALID not in out.stdout
    out = subprocess.run([sel, "-q", "/nonexistent/q.txt", "-h", "0.9", "-c", "none"], capture_output=True, text=True)
    assert out.returncode == 2 and "-q needs the database list" in out.stderr
    # every other unknown criterion: the message and exit codes of before, byte for byte
    out = subprocess.run([sel, "-l", "/nonexistent/list.txt", "-h", "0.9", "-c", "cb"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout == INVALID + "\n" and out.stderr == ""
    out = subprocess.run([sel, "-q", "/nonexistent/q.txt", "-l", "/nonexistent/list.txt", "-c", "cb"], capture_output=True, text=True)
    assert out.returncode == 2 and out.stderr == "selection: -q -c cb: the accepted criteria are hll_a, hll_an and smh_a\n"
    assert "none" in subprocess.run([sel, "-x"], capture_output=True, text=True).stdout


@pytest.mark.parametrize("flavour,fp", [("fma", FP_FMA), ("nofma", FP_STRICT)])
def test_goldens_equal_flat_oracle(oracle, monkeypatch, flavour, fp):
    monkeypatch.chdir(GOLDEN)
    ds = pkg.load_dataset("influenza_filelist.txt", 0, 0, fp)
    assert ds.hll.shape == (10, 16384)
    counts = {}
    for h in ("0.01", "0.5", "0.9"):
        want = (EXP / f"influenza_none_h{h}.{flavour}.txt").read_text()
        pairs, _ = flat_oracle_select(oracle, ds.hll, ds.cards, float(h), True, fp)
        assert pkg.format_lines(ds.names, pairs) == want, h
        counts[h] = len(pairs)
        # the real smh_a output of the same fixtures is a subset of it, line for line
        smh = (EXP / f"influenza_smh_a_a32_h{h}.{flavour}.txt").read_text().splitlines()
        assert set(smh) <= set(want.splitlines())
    assert counts == {"0.01": 41, "0.5": 7, "0.9": 7}
    assert len((EXP / f"influenza_smh_a_a32_h0.01.{flavour}.txt").read_text().splitlines()) == 10
