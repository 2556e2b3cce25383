"""Criterion smh_c (SELHIP_CRIT_SMH_C: at least c_min equal SuperMinHash buckets), the parts that need no GPU: the constant and its
documentation, the exported symbol, min_matches against brute force, the refusals of the wrappers, of the CLI and of the two drivers
whose signatures carry no threshold, and the pinned messages of the other criteria, unchanged."""
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_exhaustive_host import INVALID

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import SelhipError

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
SEL = str(BIN / "selection")


def test_constant_and_header():
    assert pkg.CRIT_SMH_C == 5
    assert (pkg.CRIT_SMH_A, pkg.CRIT_HLL_A, pkg.CRIT_HLL_AN, pkg.CRIT_HLL_A_SMH_A, pkg.CRIT_NONE) == (0, 1, 2, 3, 4)
    header = (ROOT / "include" / "selection_hip.h").read_text()
    assert "#define SELHIP_CRIT_SMH_C        5" in header
    assert "int selhip_ctx_set_min_matches(selhip_ctx* ctx, int c_min);" in header
    for word in ("smhc_path_used", "c_min > m", "selhip_multi_select and selhip_ooc_select"):
        assert word in header, word


def test_symbol_resolves():
    lib = pkg.hip_lib()
    assert lib.selhip_ctx_set_min_matches is not None
    assert lib.selhip_ctx_set_min_matches(None, 3) == -1          # SELHIP_E_BADARG: no context
    assert hasattr(pkg.Selector, "set_min_matches")


def brute_min_matches(m, j):
    for c in range(1, m + 1):
        if np.float64(c) / np.float64(m) >= np.float64(j):
            return c
    return None


def test_min_matches_against_brute_force():
    rng = np.random.default_rng(5)
    for m in list(range(1, 70)) + [100, 128, 192, 256, 512, 1000, 1024, 2048]:
        js = [-1.0, 0.0, 1e-300, 0.5, 0.8, 0.9, 0.95, 1.0, float(np.float32(0.8)), float(np.float32(0.9))]
        js += [c / m for c in range(0, m + 1, max(1, m // 16))]
        js += [np.nextafter(c / m, 2.0) for c in (1, m // 2, m - 1) if 0 < c < m] + [np.nextafter(c / m, -1.0) for c in (1, m // 2, m) if c > 0]
        js += rng.random(8).tolist()
        for j in js:
            want = brute_min_matches(m, j)
            assert want is not None, (m, j)
            got = pkg.min_matches(m, j)
            assert got == want and isinstance(got, int), (m, j, got, want)
    assert pkg.min_matches(512, 0.8) == 410 and pkg.min_matches(3, 1.0) == 3 and pkg.min_matches(10, -1) == 1
    for bad in (1.0000000000000002, 2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            pkg.min_matches(64, bad)
    with pytest.raises(ValueError):
        pkg.min_matches(0, 0.5)


def test_wrapper_refusals(tmp_path):
    missing = str(tmp_path / "no_such_list.txt")
    for call in (lambda **kw: pkg.select_from_filelist(missing, 0.9, 512, **kw),
                 lambda **kw: pkg.query_from_filelists(missing, missing, 0.9, 512, **kw),
                 lambda **kw: pkg.select_pairs_from_filelist(missing, missing, 0.9, 512, **kw)):
        # smh_c with its threshold gets as far as reading the list
        with pytest.raises(RuntimeError, match="selhost error"):
            call(criterion="smh_c", min_matches=7)
        with pytest.raises(ValueError, match="smh_c needs min_matches"):
            call(criterion="smh_c")
        for other in ("smh_a", "hll_a", "hll_an", "none"):
            with pytest.raises(ValueError, match="min_matches is the count threshold of criterion smh_c"):
                call(criterion=other, min_matches=7)
        # an unknown name: the reference's message, as before
        with pytest.raises(ValueError) as e:
            call(criterion="cb")
        assert str(e.value) == INVALID
    with pytest.raises(ValueError, match="aux_bytes"):
        pkg.select_from_filelist(missing, 0.9, 0, criterion="smh_c", min_matches=1)


def run(args):
    return subprocess.run([SEL] + args, capture_output=True, text=True)


def test_cli_refusals():
    lst = ["-l", "/nonexistent/list.txt", "-h", "0.9"]
    # every refusal comes before any file is read: exit 2, nothing on stdout, no word about the (missing) list
    for args, word in ((lst + ["-C", "5"], "-C"),
                       (lst + ["-C", "5", "-c", "smh_a"], "-C"),
                       (lst + ["-C", "5", "-c", "none"], "-C"),
                       (lst + ["-c", "smh_c", "-a", "512"], "-C c_min"),
                       (lst + ["-c", "smh_c", "-C", "5"], "-a"),
                       (lst + ["-c", "smh_c", "-C", "5", "-a", "4"], "-a"),
                       (lst + ["-c", "smh_c", "-C", "5", "-a", "512", "-g", "1"], "-g"),
                       (lst + ["-c", "smh_c", "-C", "5", "-a", "512", "-g", "2"], "-g"),
                       (lst + ["-c", "smh_c", "-C", "5", "-a", "512", "-B", "100"], "-B"),
                       (lst + ["-c", "smh_c", "-C", "0", "-a", "512"], "1..64"),
                       (lst + ["-c", "smh_c", "-C", "65", "-a", "512"], "1..64"),
                       (lst + ["-c", "smh_c", "-C", "-3", "-a", "512"], "1..64"),
                       (["-q", "/nonexistent/q.txt"] + lst + ["-c", "smh_c", "-a", "512"], "-C c_min"),
                       (["-p", "/nonexistent/p.txt"] + lst + ["-c", "smh_c", "-C", "5"], "-a"),
                       (lst + ["-K", "3", "-c", "smh_c", "-a", "512"], "-C c_min"),
                       (lst + ["-M", "/nonexistent/out.tsv", "-C", "5"], "-M")):
        out = run(args)
        assert out.returncode == 2 and out.stdout == "" and word in out.stderr, (args, out)
        assert "nonexistent" not in out.stderr and "input file" not in out.stderr, (args, out.stderr)
    # accepted: the run gets as far as the list
    out = run(lst + ["-c", "smh_c", "-C", "5", "-a", "512"])
    assert out.returncode != 0 and out.returncode != 2 and "No valid input file provided" in out.stderr and INVALID not in out.stdout
    out = run(lst + ["-c", "smh_c", "-C", "64", "-a", "512", "-n", "-K", "3"])
    assert out.returncode not in (0, 2) and "No valid input file provided" in out.stderr
    out = run(["-q", "/nonexistent/q.txt", "-c", "smh_c", "-C", "5", "-a", "512"])
    assert out.returncode == 2 and "-q needs the database list" in out.stderr
    usage = run(["-x"]).stdout
    assert "smh_c" in usage and "-C c_min" in usage


def test_pinned_messages_unchanged():
    out = run(["-l", "/nonexistent/list.txt", "-h", "0.9", "-c", "cb"])
    assert out.returncode == 0 and out.stdout == INVALID + "\n" and out.stderr == ""
    out = run(["-q", "/nonexistent/q.txt", "-l", "/nonexistent/list.txt", "-c", "cb"])
    assert out.returncode == 2 and out.stderr == "selection: -q -c cb: the accepted criteria are hll_a, hll_an and smh_a\n"
    out = run(["-l", "/nonexistent/list.txt", "-h", "0.9", "-c", "none"])
    assert out.returncode != 0 and "No valid input file provided" in out.stderr and INVALID not in out.stdout
    assert "none" in run(["-x"]).stdout


def test_drivers_refuse_the_criterion():
    """selhip_multi_select and selhip_ooc_select have no argument for the threshold: SELHIP_E_BADARG with a message that says so, before
    any device is touched"""
    hll = np.zeros((4, 16384), dtype=np.uint8)
    aux = np.zeros((4, 8), dtype=np.uint64)
    cards = np.arange(4, dtype=np.float64)
    with pytest.raises(SelhipError, match="smh_c"):
        pkg.ooc_select(hll, aux, cards, 0.5, 2, n_rows=1, n_bands=8, criterion=pkg.CRIT_SMH_C)
    with pytest.raises(SelhipError, match="smh_c"):
        pkg.selection.multi_select([0], hll, aux, cards, 0.5, n_rows=1, n_bands=8, gather=0, criterion=pkg.CRIT_SMH_C)
