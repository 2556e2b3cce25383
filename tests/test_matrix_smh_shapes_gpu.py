"""The narrow (m = 32, 64) and the wide (m = 2048 .. 8192 in steps of 1024) kernel of the SuperMinHash matrices (kernel_matrix_smh.cuh,
DESIGN.md section 36): every call against the numpy model of smh_matrix_model.py, byte for byte, twice, and against the same call on
the generic kernel ("matrix_smh_generic" = 1); "matrix_smh_kernel_used" must name the kernel that ran."""
import numpy as np
import pytest
import torch

import smh_matrix_model as model
from test_matrix_smh_gpu import COMBOS, NP, SENTINEL, exact, no_hll, upload

from cuda_selection_criteria_amd import Selector

pytestmark = pytest.mark.gpu

KIND = {32: 2, 64: 2, 2048: 3, 3072: 3}                       # "matrix_smh_kernel_used": 2 narrow, 3 wide (an even and an odd chunk count)
SHAPES = [(1, 1), (2, 3), (5, 63), (13, 65), (37, 129), (50, 200)]


def check(sel, m, call, fill, what):
    """fill(counts / m or counts, dtype) -> the buffer `call(measure, dtype)` must return: from the kernel of m twice, then from the generic one"""
    for measure, dt in COMBOS:
        want = fill(measure == "smh_jaccard", NP[dt])
        for generic, kind in ((0, KIND[m]), (0, KIND[m]), (1, 0)):
            sel.set_param("matrix_smh_generic", generic)
            got = call(measure, dt).cpu().numpy()
            sel.set_param("matrix_smh_generic", 0)
            assert sel.get_param("matrix_smh_kernel_used") == kind and sel.get_param("matrix_smh_path_used") == 0, (what, generic)
            exact(got, want, (what, measure, dt, generic))
            first = got if generic == 0 else first
        exact(got, first, (what, "generic against new"))


@pytest.mark.parametrize("query", [False, True], ids=["self", "query"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("m", sorted(KIND))
def test_shapes(m, shape, query):
    n_r, n_c = shape
    rows = model.random_rows(n_r + n_c, m, seed=31 * m + n_c)
    D = rows[n_r:]
    A = rows[:n_r] if query else D[:n_r]                       # self: the slab [0, n_r) of the n_c x n_c matrix
    counts = model.match_counts(A, D).astype(np.float64)
    with Selector(0) as sel:
        upload(sel, D)
        if query:
            sel.upload_queries(no_hll(n_r), A, np.zeros(n_r))
        call = (lambda ms, dt: sel.query_matrix(ms, dtype=dt)) if query else (lambda ms, dt: sel.matrix(ms, dtype=dt, rows=(0, n_r)))
        check(sel, m, call, lambda jac, t: (counts / np.float64(m) if jac else counts).astype(t), (m, shape, query))


@pytest.mark.parametrize("mode", ["mirror", "upper", "query"])
@pytest.mark.parametrize("m", sorted(KIND))
def test_slab_positions_ld(m, mode):
    n, r0, r1 = 50, 7, 30
    rows = model.random_rows(2 * n, m, seed=7 * m)
    D, A = rows[:n], rows[:n] if mode != "query" else rows[n:]
    counts = model.match_counts(A, D).astype(np.float64)
    rng = np.random.default_rng(m)
    rp, cp = rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)

    def fill(jac, t):
        want = np.full((n, n + 3), SENTINEL, dtype=t)
        for i in range(r0, r1):                                 # without mirrored stores a row keeps the columns [0, r0) u [i, n)
            ks = np.r_[0:r0, i:n] if mode == "upper" else np.arange(n)
            want[rp[i], cp[ks]] = ((counts / np.float64(m) if jac else counts)[i, ks]).astype(t)
        return want

    def call(measure, dt):
        buf = torch.full((n, n + 3), SENTINEL, dtype=dt, device="cuda")
        (sel.query_matrix if mode == "query" else sel.matrix)(measure, dtype=dt, rows=(r0, r1), row_pos=rp, col_pos=cp, out=buf[:, :n])
        return buf

    with Selector(0) as sel:
        upload(sel, D)
        sel.upload_queries(no_hll(n), A, np.zeros(n))
        sel.set_param("matrix_mirror", 0 if mode == "upper" else 1)
        check(sel, m, call, fill, (m, mode))


@pytest.mark.parametrize("m", sorted(KIND))
def test_planted_rows(m):
    """row 0 is the base; row i shares with it exactly the buckets of PLANT[i - 1] -- so the model's row 0 is known by construction"""
    plant = [[0], [m - 1], [2], [3], [m - 2], [m - 3], [5]]    # one bucket: the first, the last, .x and .y halves of a 16-byte load
    # rows 8 .. 11 lie in one wave load of the narrow kernel (4 k .. 4 k + 3): last bucket of one group, first bucket of the next
    plant += [[m - 1], [0], [m - 1], [0]]
    if m >= 2048:                                              # wide: the last bucket of a chunk and the first of the next
        plant += [[1023], [1024], [m - 1025], [m - 1024], [1023, 1024]]
    plant += [list(range(m)), [], []]
    idx = np.arange((len(plant) + 1) * m, dtype=np.uint64).reshape(-1, m) + np.uint64(1)
    rows = (idx << np.uint64(32)) | (idx * np.uint64(2654435761) & np.uint64(0xFFFFFFFF))       # all distinct, in both dwords
    for i, buckets in enumerate(plant):
        rows[i + 1, buckets] = rows[0, buckets]
    rows[-2] = rows[0] ^ np.uint64(1 << 32)                     # differs from the base in the high dword only ...
    rows[-1] = rows[0] ^ np.uint64(1)                           # ... and in the low dword only
    counts = model.match_counts(rows, rows).astype(np.float64)
    assert counts[0, 1:].tolist() == [float(len(b)) for b in plant]
    with Selector(0) as sel:
        upload(sel, rows)
        sel.upload_queries(no_hll(5), rows[:5], np.zeros(5))
        for call, want in ((sel.matrix, counts), (sel.query_matrix, counts[:5])):
            check(sel, m, lambda ms, dt: call(ms, dtype=dt), lambda jac, t: (want / np.float64(m) if jac else want).astype(t), (m, "planted"))
