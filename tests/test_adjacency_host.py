"""The sparse adjacency without a GPU: the numpy model (tests/adjacency_model.py) against a plain dict loop, and the exported names."""
import struct

import numpy as np
import pytest

from conftest import ROOT
import adjacency_model as AM

import cuda_selection_criteria_amd as pkg

# a dozen records: a duplicate pair (3, 5) with three values, -0.0 and +0.0 on one pair, a NaN, a self loop, a pair listed in both directions
RECORDS = [(3, 5, 0.25), (0, 1, 0.5), (3, 5, 0.75), (5, 3, 0.5), (2, 4, -0.0), (2, 4, 0.0), (1, 6, float("nan")), (6, 6, 1.0),
           (4, 2, -1.5), (0, 6, 0.125), (3, 5, 0.25), (1, 0, 0.5)]


def total_order(v):
    bits = struct.unpack("<Q", struct.pack("<d", v))[0]
    return bits ^ (1 << 63) if bits >> 63 == 0 else bits ^ ((1 << 64) - 1)


def dict_loop(records, n_rows, symmetric, min_value):
    best = {}
    for i, k, v in records:
        if not v >= min_value:
            continue
        for r, c in {(i, k), (k, i)} if symmetric else {(i, k)}:
            if (r, c) not in best or total_order(v) > total_order(best[r, c]):
                best[r, c] = v
    cells = sorted(best)
    row_ptr = [sum(1 for r, _ in cells if r < row) for row in range(n_rows + 1)]
    return row_ptr, [c for _, c in cells], [best[cell] for cell in cells]


@pytest.mark.parametrize("symmetric", [False, True])
@pytest.mark.parametrize("min_value", [-np.inf, 0.0, 0.5])
def test_model_against_dict_loop(symmetric, min_value):
    i, k, v = (np.array(x) for x in zip(*RECORDS))
    row_ptr, col, val = AM.csr(i, k, v, 7, symmetric, min_value)
    want = dict_loop(RECORDS, 7, symmetric, min_value)
    assert row_ptr.tolist() == want[0] and col.tolist() == want[1]
    assert val.tobytes() == np.array(want[2], dtype=np.float64).tobytes()
    if min_value <= 0.0:
        assert val[list(zip(np.repeat(np.arange(7), np.diff(row_ptr)), col)).index((2, 4))].tobytes() == np.float64(0.0).tobytes()   # +0.0 beats -0.0


def test_names():
    header = (ROOT / "include" / "selection_hip.h").read_text()
    for name in ("selhip_ctx_adjacency", "selhip_adjacency"):
        assert name in pkg._lib.HIP_SYMBOLS and f"int {name}(" in header and getattr(pkg.hip_lib(), name) is not None
    assert " 2n. " in header and "selhip_csr_t" in header
    assert "adjacency" in pkg.__all__ and callable(pkg.adjacency) and callable(pkg.Selector.adjacency)
