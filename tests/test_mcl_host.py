"""The Markov clustering without a GPU (include/selection_hip.h section 2o): tests/mcl_model.py against an independent dense float64 MCL,
and the public names."""
import re

import numpy as np
import pytest

import mcl_model as MM
from conftest import ROOT

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import _lib


def dense_mcl(A, r, prune, iters):
    """MCL in whole-matrix operations: matrix power, element power, the prune threshold, column normalisation; nothing is cut"""
    top = A.max(axis=0)
    M = A + np.diag(np.where(top > 0, top, 1.0))
    M = M / M.sum(axis=0)
    for _ in range(iters):
        M = np.linalg.matrix_power(M, 2) ** r
        M[M < prune * M.max(axis=0)] = 0.0
        M = M / M.sum(axis=0)
    return M


@pytest.mark.parametrize("hub", [True, False])
def test_model_against_dense_mcl(hub):
    """K >= n, so nothing is cut.  The bound is one ulp of 1.0, the largest flow: measured on the CPU, the greatest difference of a final
    flow was 7.3e-18 (no hub) and 0.0 (hub) -- BLAS adds in another order than the model, the converged flows hide most of it"""
    row_ptr, col, val, n = MM.planted(hub=hub)
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(row_ptr)), col] = val
    got = MM.mcl(row_ptr, col, val, n, max_entries=n)
    ref = dense_mcl(A, 2.0, 1e-4, got["iters"])
    assert got["n_clusters"] == 8 and 1 < got["iters"] < 64 and got["chaos"] <= 1e-3
    assert np.abs(ref - MM.dense(got["columns"], n)).max() <= 2.0 ** -52
    i, j = np.nonzero(ref)
    label = np.arange(n)
    for _ in range(n):                                                          # components of the reference's entries, by relaxation
        low = np.minimum(label[i], label[j])
        np.minimum.at(label, i, low)
        np.minimum.at(label, j, low)
    assert np.array_equal(label, got["label"])


def test_public_names():
    header = (ROOT / "include" / "selection_hip.h").read_text()
    for name in ("selhip_mcl", "selhip_ctx_mcl"):
        assert name in _lib.HIP_SYMBOLS and re.search(rf"\bint {name}\(", header)
    assert "mcl" in pkg.__all__ and callable(pkg.mcl) and callable(pkg.Selector.mcl)
