"""The Markov clustering on the GPU (selhip_mcl, selhip_ctx_mcl; include/selection_hip.h section 2o) against tests/mcl_model.py: with
inflation 2.0 labels, dense ids, counts, iterations and the chaos bit for bit; with 1.7 everything but the chaos, on a graph whose prune
and cut decisions the model found at least 1e-9 (relative) away from their thresholds.  K takes both sides of each kernel class edge."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import adjacency_model as AM
import mcl_model as MM
from test_cluster_gpu import snapshot
from test_smhv_gpu import case, configure, zeros_hll

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import MODE_SMH, SelhipError, Selector
from cuda_selection_criteria_amd._lib import Csr, Mcl, MclParams

pytestmark = pytest.mark.gpu

SENTINEL = -77
KCLASS = {1: 0, 8: 0, 9: 1, 32: 1, 33: 2, 64: 2}
CASES = [(K, True) for K in KCLASS] + [(64, False)]                              # hub: one row of 78 entries; without it no row reaches 64: nothing is cut


@functools.lru_cache(maxsize=None)
def model(K, hub, r):
    return MM.mcl(*MM.planted(hub=hub), inflation=r, max_entries=K)


def assert_equal(got, want, what, chaos=True):
    for name in ("label", "cluster"):
        assert got[name].dtype == np.int32 and np.array_equal(got[name], want[name]), (what, name)
    assert (got["n_clusters"], got["iters"]) == (want["n_clusters"], want["iters"]), (what, got["n_clusters"], got["iters"], got["chaos"], want["chaos"])
    if chaos:
        assert np.float64(got["chaos"]).tobytes() == np.float64(want["chaos"]).tobytes(), (what, got["chaos"], want["chaos"])


@pytest.mark.parametrize("r", [2.0, 1.7])
@pytest.mark.parametrize("K,hub", CASES)
def test_planted(K, hub, r):
    row_ptr, col, val, n = MM.planted(hub=hub)
    assert (np.diff(row_ptr).max() > 64) == hub
    want = model(K, hub, r)
    assert r == 2.0 or want["margin"] > 1e-9
    assert_equal(pkg.mcl(row_ptr, col, val, n, inflation=r, max_entries=K), want, (K, hub, r), chaos=r == 2.0)


@pytest.mark.parametrize("K", KCLASS)
def test_behind_a_pass(K):
    n, m = 120, 128
    aux, cards = case(n, m)
    with Selector(0) as sel:
        assert sel.get_param("mcl_iters_last") == sel.get_param("mcl_clusters_last") == sel.get_param("mcl_kclass_last") == -1
        sel.upload(zeros_hll(n), aux, cards)
        configure(sel, c_min=4)
        sel.run(-1.0, MODE_SMH, 7, 3)
        rec = sel.fetch()
        assert len(rec) > n
        before = snapshot(sel)
        sel.timing(1)
        for cut in (None, float(np.median(rec["jaccard"]))):
            row_ptr, col, val = AM.csr(rec["i"], rec["k"], rec["jaccard"], n, True, -np.inf if cut is None else cut)
            want = MM.mcl(row_ptr, col, val, n, max_entries=K)
            assert_equal(sel.mcl(cut, max_entries=K), want, (K, cut))
            assert (sel.get_param("mcl_iters_last"), sel.get_param("mcl_clusters_last"), sel.get_param("mcl_kclass_last")) == (want["iters"], want["n_clusters"], KCLASS[K])
        got = sel.mcl(cut, max_entries=K, to_host=False)
        assert got["label"].is_cuda and np.array_equal(got["cluster"].cpu().numpy(), want["cluster"])
        assert sel.kernel_ms("mcl") > 0
        sel.timing(0)
        assert snapshot(sel) == before                                          # list, statistics, attempts: as they were
        sel.upload_queries(zeros_hll(5), aux[:5], cards[:5])
        sel.run_queries(-1.0, MODE_SMH, 7, 3)
        with pytest.raises(SelhipError, match="query pass") as err:
            sel.mcl()
        assert err.value.code == -5


def test_long_start_row():
    """a star whose hub row has 5 000 entries: the start's route beyond the LDS; K = 8 of them stay, and a second iteration works on what the
    start cut.  The self loop must carry the row's largest value: the chaos bits show it"""
    n, rng = 5001, np.random.default_rng(3)
    w = rng.uniform(0.1, 1.0, n - 1)
    row_ptr = np.concatenate([[0, n - 1], n - 1 + np.arange(1, n)]).astype(np.int64)
    col = np.concatenate([np.arange(1, n), np.zeros(n - 1)]).astype(np.int32)
    val = np.concatenate([w, w])
    assert_equal(pkg.mcl(row_ptr, col, val, n, max_entries=8, max_iters=2), MM.mcl(row_ptr, col, val, n, max_entries=8, max_iters=2), "star")


def test_empty_shapes_and_one_iteration():
    none = np.zeros(0)
    got = pkg.mcl(np.zeros(1, dtype=np.int64), none.astype(np.int32), none, 0)
    assert (len(got["label"]), got["n_clusters"], got["iters"], got["chaos"]) == (0, 0, 0, 0.0)
    got = pkg.mcl(np.zeros(8, dtype=np.int64), none.astype(np.int32), none, 7)               # nnz = 0: singletons
    assert got["label"].tolist() == got["cluster"].tolist() == list(range(7)) and (got["n_clusters"], got["iters"], got["chaos"]) == (7, 1, 0.0)
    want = MM.mcl(*MM.planted(), max_iters=1)
    assert want["chaos"] > 1e-3
    assert_equal(pkg.mcl(*MM.planted(), max_iters=1), want, "max_iters = 1")


@pytest.mark.parametrize("bad", [np.nan, -0.5, np.inf])
def test_bad_value_writes_nothing(bad):
    row_ptr, col, val, n = MM.planted()
    val = val.copy()
    val[[100, 2000]] = bad
    dev = [torch.from_numpy(a).cuda() for a in (row_ptr, col, val)]
    label, cluster = (torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda") for _ in range(2))
    scalars = C.c_int64(SENTINEL), C.c_int64(SENTINEL), C.c_double(SENTINEL)
    out = Mcl(label.data_ptr(), cluster.data_ptr(), *(C.pointer(s) for s in scalars))
    rc = pkg.hip_lib().selhip_mcl(C.byref(Csr(*(d.data_ptr() for d in dev))), n, len(col), C.byref(MclParams()), C.byref(out), None)
    assert rc == -1 and re_match(r"2 entries .* entry 100 is one")
    assert torch.all(label == SENTINEL) and torch.all(cluster == SENTINEL) and all(s.value == SENTINEL for s in scalars)
    for params in (MclParams(inflation=1.0), MclParams(inflation=np.nan), MclParams(max_entries=65), MclParams(prune=1.0), MclParams(max_iters=-1),
                   MclParams(chaos_tol=-1.0)):
        assert pkg.hip_lib().selhip_mcl(C.byref(Csr(*(d.data_ptr() for d in dev))), n, len(col), C.byref(params), C.byref(out), None) == -1
    swapped = col.copy()
    swapped[[0, 1]] = col[[1, 0]]                                                # row 0: its first two columns out of order
    with pytest.raises(SelhipError, match="1 entries .* entry 1 is one"):
        pkg.mcl(row_ptr, swapped, MM.planted()[2], n)


def re_match(pattern):
    import re
    return re.search(pattern, pkg.hip_lib().selhip_last_error(None).decode())
