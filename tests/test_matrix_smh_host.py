"""The SuperMinHash measures of the dense matrices (include/selection_hip.h section 2f), the parts that need no GPU: the numpy model and
its planted sets (smh_matrix_model.py), the constants, the measure names of the Python layer and the refusals of the command line."""
import subprocess

import numpy as np
import pytest

import smh_matrix_model as model
from conftest import GOLDEN, ROOT

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import _lib

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def test_model_counts_by_hand():
    A = np.array([[1, 2, 3, 4], [1, 2, 9, 9], [7, 7, 7, 7]], dtype=np.uint64)
    B = np.array([[1, 2, 3, 4], [7, 2, 7, 4]], dtype=np.uint64)
    assert model.match_counts(A, B).tolist() == [[4, 2], [2, 1], [0, 2]]
    assert model.match_counts(A, B, chunk=1).tolist() == [[4, 2], [2, 1], [0, 2]]
    assert model.expected(A, B, "smh_jaccard").tolist() == [[1.0, 0.5], [0.5, 0.25], [0.0, 0.5]]
    assert model.expected(A, B, "smh_matches", np.float32).dtype == np.float32
    # the compare is on the whole 64 bits: a difference in one dword alone is a difference
    lo, hi = np.uint64(5), np.uint64(5) | (np.uint64(1) << np.uint64(32))
    assert model.match_counts(np.array([[lo, hi]]), np.array([[hi, hi]])).tolist() == [[1]]


@pytest.mark.parametrize("m", [1, 3, 100, 512])
def test_random_rows_spread_the_counts(m):
    rows = model.random_rows(65, m, seed=m)
    assert rows.shape == (65, m) and rows.dtype == np.uint64
    c = model.match_counts(rows, rows)
    assert np.array_equal(c, c.T) and np.all(np.diagonal(c) == m)
    assert c.min() == 0
    if m >= 100:
        off = c[~np.eye(65, dtype=bool)]
        assert off.max() > 0.8 * m and len(np.unique(off)) > 20


@pytest.mark.parametrize("m", [100, 512])
def test_planted_sets(m):
    one = model.match_counts(model.planted_single(m, 1), model.planted_single(m, 1))
    assert np.all(one[0, 1:] == 1) and one[0, 0] == m
    most = model.match_counts(model.planted_all_but_one(m, 2), model.planted_all_but_one(m, 2))
    assert np.all(most[0, 1:] == m - 1) and np.all(np.diagonal(most) == m)
    off = most[1:, 1:][~np.eye(m, dtype=bool)]
    assert np.all(off == m - 2)


def test_half_equal_rows():
    m = 128
    rows = model.half_equal(9, m, 3)
    d = rows ^ rows[0][None, :]
    for g in range(1, 9):
        changed = d[g] != 0
        assert changed.any()
        if g & 1:
            assert np.all((d[g][changed] & np.uint64(0xFFFFFFFF)) == 0)           # upper dword only
        else:
            assert np.all((d[g][changed] >> np.uint64(32)) == 0)                  # lower dword only
        assert model.match_counts(rows[:1], rows[g:g + 1])[0, 0] == m - int(changed.sum())


# ---- the constants and the names ----------------------------------------------------------------------------------------------------
def test_constants_and_header():
    assert (_lib.MEASURE_SMH_MATCHES, _lib.MEASURE_SMH_JACCARD) == (16, 17)
    assert (pkg.MEASURE_SMH_MATCHES, pkg.MEASURE_SMH_JACCARD) == (16, 17)
    header = (ROOT / "include" / "selection_hip.h").read_text()
    defines = dict(line.split()[1:3] for line in header.splitlines() if line.startswith("#define SELHIP_MEASURE_"))
    assert defines["SELHIP_MEASURE_SMH_MATCHES"] == "16" and defines["SELHIP_MEASURE_SMH_JACCARD"] == "17"
    assert defines["SELHIP_MEASURE_JACCARD"] == "0" and defines["SELHIP_MEASURE_UNION"] == "1"


def test_measure_names():
    assert [pkg.measure_code(x) for x in ("jaccard", "union", "smh_matches", "smh_jaccard")] == [0, 1, 16, 17]
    assert pkg.measure_code(16) == 16 and pkg.measure_code(0) == 0
    for bad in ("smh", "mash", "", 2, 15, None, True, 1.0, 16.0):
        with pytest.raises(ValueError, match="smh_matches"):
            pkg.measure_code(bad)


@pytest.mark.parametrize("measure", ["smh_matches", "smh_jaccard", 16, 17])
def test_filelist_helpers_need_aux_bytes(measure, monkeypatch):
    monkeypatch.chdir(GOLDEN)
    for aux_bytes in (0, 7):                                    # 7 bytes: no whole bucket
        with pytest.raises(ValueError, match="aux_bytes"):
            pkg.matrix_from_filelist("influenza_filelist.txt", aux_bytes, measure=measure)
        with pytest.raises(ValueError, match="aux_bytes"):
            pkg.query_matrix_from_filelists("influenza_filelist.txt", "influenza_filelist.txt", aux_bytes, measure=measure)
    with pytest.raises(ValueError, match="measure"):
        pkg.matrix_from_filelist("influenza_filelist.txt", 512, measure="bogus")


# ---- the command line: refused before any file is read or any device opened -------------------------------------------------------------
@pytest.mark.parametrize("args,needle", [
    (["-l", "influenza_filelist.txt", "-M", "OUT", "-E", "smh"], "-a"),
    (["-l", "influenza_filelist.txt", "-M", "OUT", "-E", "smh_matches"], "-a"),
    (["-l", "influenza_filelist.txt", "-M", "OUT", "-E", "smh", "-a", "4"], "-a"),
    (["-l", "influenza_filelist.txt", "-M", "OUT", "-E", "smh", "-a", "512", "-U"], "-U"),
    (["-l", "influenza_filelist.txt", "-M", "OUT", "-E", "bogus", "-a", "512"], "bogus"),
    (["-l", "influenza_filelist.txt", "-E", "smh", "-a", "512"], "-M"),
    (["-l", "influenza_filelist.txt", "-E", "hll", "-a", "512"], "-M"),
])
def test_cli_refusals(tmp_path, args, needle):
    out_file = tmp_path / "no.tsv"
    args = [str(out_file) if a == "OUT" else a for a in args]
    out = subprocess.run([str(BIN / "selection")] + args, cwd=GOLDEN, capture_output=True, text=True)
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert "-E" in out.stderr and needle in out.stderr
    assert out.stdout == "" and not out_file.exists()
