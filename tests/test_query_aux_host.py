"""Query passes under the auxiliary-HLL criteria (hll_a, hll_an, hll_a + smh_a), the parts that need no GPU: exported symbols, Python
surface, and the CLI's handling of -q -c (checked or failing before any device is opened)."""
import inspect
import subprocess

from conftest import ROOT

import cuda_selection_criteria_amd as pkg

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"


def test_query_aux_symbols_exported():
    lib = pkg.hip_lib()
    for name in ("selhip_ctx_upload_queries_aux_hll", "selhip_ctx_attach_queries_aux_hll"):
        assert hasattr(lib, name), name


def test_query_aux_python_surface():
    for name in ("upload_queries_aux_hll", "attach_queries_aux_hll"):
        assert callable(getattr(pkg.Selector, name, None)), name
    params = inspect.signature(pkg.query_from_filelists).parameters
    assert "criterion" in params and params["criterion"].default == "smh_a"


def test_query_from_filelists_rejects_unknown_criterion(tmp_path):
    try:
        pkg.query_from_filelists(str(tmp_path / "q.txt"), str(tmp_path / "db.txt"), 0.9, 256, criterion="jaccard")
    except ValueError as e:
        assert "hll_a" in str(e)
    else:
        raise AssertionError("an unknown criterion was accepted")


def test_cli_query_usage_names_criteria():
    out = subprocess.run([str(BIN / "selection"), "-x"], capture_output=True, text=True)
    query_line = [ln for ln in out.stdout.splitlines() if "-q" in ln]
    assert out.returncode == 0 and query_line and "hll_a" in query_line[0] and "hll_an" in query_line[0]


def test_cli_query_hll_reads_lists(tmp_path):
    """-q -c hll_a is no longer refused up front: it gets as far as reading the lists, and names the mode, the criterion and the list"""
    for crit in ("hll_a", "hll_an"):
        out = subprocess.run([str(BIN / "selection"), "-l", str(tmp_path / "db.txt"), "-q", str(tmp_path / "q.txt"), "-h", "0.9", "-a", "256",
                              "-c", crit], cwd=tmp_path, capture_output=True, text=True)
        assert out.returncode != 0
        assert f"-q -c {crit}" in out.stderr and "db.txt" in out.stderr and "cannot be combined" not in out.stderr


def test_cli_query_rejects_unknown_criterion(tmp_path):
    out = subprocess.run([str(BIN / "selection"), "-l", "/nonexistent/db.txt", "-q", "/nonexistent/q.txt", "-h", "0.9", "-a", "256",
                          "-c", "jaccard"], cwd=tmp_path, capture_output=True, text=True)
    assert out.returncode == 2 and "-q" in out.stderr and "jaccard" in out.stderr
