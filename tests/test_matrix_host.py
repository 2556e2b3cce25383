"""Dense matrices (include/selection_hip.h section 2f), the parts that need no GPU: the text writer selhost_write_matrix of libselhost and
the new symbols of both libraries."""
import ctypes as C
import math

import numpy as np
import pytest

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import _lib


def write_matrix(host, path, values, row_names, col_names, ld=None):
    values = np.ascontiguousarray(values, dtype=np.float64)
    n_rows, width = values.shape
    n_cols = len(col_names)
    rn = (C.c_char_p * max(1, n_rows))(*[s.encode() for s in row_names])
    cn = (C.c_char_p * max(1, n_cols))(*[s.encode() for s in col_names])
    return host.selhost_write_matrix(str(path).encode(), values.ctypes.data if values.size else None, n_rows, n_cols,
                                     width if ld is None else ld, rn, cn)


def read_matrix(path):
    """-> (row names, column names, f64 array) of a table written by selhost_write_matrix"""
    lines = open(path).read().split("\n")
    assert lines[-1] == ""                                    # every line ends with a newline
    head = lines[0].split("\t")
    assert head[0] == ""                                      # the first line starts with a tab
    rows, vals = [], []
    for line in lines[1:-1]:
        f = line.split("\t")
        rows.append(f[0])
        vals.append([float(x) for x in f[1:]])
    return rows, head[1:], np.array(vals, dtype=np.float64).reshape(len(rows), len(head) - 1)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(both_nan | (a.view(np.uint64) == b.view(np.uint64))))


def test_write_matrix_round_trips_exactly(host, tmp_path):
    sub = 5e-324                                              # the smallest subnormal
    m = np.array([[1.0, float("nan"), -2.2250738585072014e-308],
                  [sub, 0.1 + 0.2, -0.0],
                  [1.7976931348623157e308, 1.0 / 3.0, 12345.678901234567]], dtype=np.float64)
    names = ["a/b c.fna.gz", "g2", "third"]
    path = tmp_path / "m.tsv"
    assert write_matrix(host, path, m, names, names) == 0
    rows, cols, got = read_matrix(path)
    assert rows == names and cols == names
    assert same_bits(got, m)
    assert math.isnan(got[0, 1]) and got[1, 0] == sub and got[0, 0] == 1.0 and np.signbit(got[1, 2])
    text = path.read_text()
    assert text.startswith("\t" + "\t".join(names) + "\n")
    assert text.splitlines()[1].startswith("a/b c.fna.gz\t1\t")


def test_write_matrix_rectangular_and_ld(host, tmp_path):
    rng = np.random.default_rng(5)
    m = rng.standard_normal((2, 5))
    padded = np.full((2, 8), 777.0)
    padded[:, :5] = m
    path = tmp_path / "r.tsv"
    assert write_matrix(host, path, padded, ["q0", "q1"], ["d0", "d1", "d2", "d3", "d4"], ld=8) == 0
    rows, cols, got = read_matrix(path)
    assert rows == ["q0", "q1"] and cols == ["d0", "d1", "d2", "d3", "d4"]
    assert same_bits(got, m)
    # no rows: the header line alone
    assert write_matrix(host, path, np.zeros((0, 2)), [], ["x", "y"]) == 0
    assert path.read_text() == "\tx\ty\n"


def test_write_matrix_errors_are_statuses(host, tmp_path):
    m = np.zeros((1, 1))
    rc = write_matrix(host, tmp_path / "no_such_dir" / "m.tsv", m, ["a"], ["a"])
    assert rc == -2 and b"cannot open" in host.selhost_last_error()          # SELHOST_E_IO
    assert write_matrix(host, tmp_path / "m.tsv", np.zeros((1, 3)), ["a"], ["a", "b", "c"], ld=2) == -1     # ld < n_cols
    assert host.selhost_write_matrix(None, None, 0, 0, 0, None, None) == -1


def test_new_symbols_resolve():
    hip, host = pkg.hip_lib(), pkg.host_lib()
    for name in ("selhip_ctx_matrix", "selhip_ctx_query_matrix"):
        assert name in _lib.HIP_SYMBOLS and getattr(hip, name) is not None
    for name in ("selhost_write_matrix", "selhost_dataset_order"):
        assert name in _lib.HOST_SYMBOLS and getattr(host, name) is not None
    assert (pkg.MEASURE_JACCARD, pkg.MEASURE_UNION, pkg.F64, pkg.F32) == (0, 1, 0, 1)
    # a null context is an argument error, not a crash
    assert hip.selhip_ctx_matrix(None, 0, 0, 0, 0, None, 0, 0, 0, None, None) == -1
    assert hip.selhip_ctx_query_matrix(None, 0, 0, 0, 0, None, 0, 0, 0, None, None) == -1


def test_dataset_order_is_the_sort_permutation(monkeypatch):
    from conftest import GOLDEN
    monkeypatch.chdir(GOLDEN)
    ds = pkg.load_dataset("influenza_filelist.txt", 0)
    listed = [l.strip() for l in (GOLDEN / "influenza_filelist.txt").read_text().splitlines() if l.strip()]
    assert sorted(ds.order.tolist()) == list(range(len(listed)))
    assert [listed[j] for j in ds.order] == ds.names
    assert np.all(np.diff(ds.cards) >= 0)
