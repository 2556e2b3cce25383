"""Query-vs-database selection, the parts that need no GPU: exported symbols, Python surface, and the CLI's refusal of options a
query pass does not combine with (checked before any device is opened)."""
import subprocess

import pytest

from conftest import ROOT

import cuda_selection_criteria_amd as pkg

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"


def test_query_symbols_exported():
    lib = pkg.hip_lib()
    for name in ("selhip_ctx_upload_queries", "selhip_ctx_attach_queries", "selhip_ctx_run_queries"):
        assert hasattr(lib, name), name


def test_query_python_surface():
    for name in ("upload_queries", "attach_queries", "run_queries"):
        assert callable(getattr(pkg.Selector, name, None)), name
    assert callable(pkg.query_from_filelists)


@pytest.mark.parametrize("extra,word", [(["-B", "100"], "-B"), (["-g", "2"], "-g"), (["-o", "out.selr"], "-o"),
                                        (["-c", "hll_a"], "hll_a"), (["-c", "hll_an"], "hll_an"), (["-r", "x.selr"], "-r")])
def test_cli_query_rejects_incompatible_options(tmp_path, extra, word):
    out = subprocess.run([str(BIN / "selection"), "-l", "/nonexistent/db.txt", "-q", "/nonexistent/q.txt", "-h", "0.9", "-a", "512", *extra],
                         cwd=tmp_path, capture_output=True, text=True)
    assert out.returncode != 0
    assert "-q" in out.stderr and word in out.stderr
    assert not (tmp_path / "out.selr").exists()


def test_cli_usage_mentions_query():
    out = subprocess.run([str(BIN / "selection"), "-x"], capture_output=True, text=True)
    assert out.returncode == 0 and "-q" in out.stdout
