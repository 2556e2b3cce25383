"""The sparse adjacency on the GPU (selhip_adjacency, selhip_ctx_adjacency).  Every output is compared as bytes with
tests/adjacency_model.py run on the same records, or on the records fetched from the pass.  The stand-alone cases are star-plus-noise
graphs whose hub row sits on every edge between the three sort kernels, once fed from the i side and once from the k side."""
import ctypes as C

import numpy as np
import pytest
import torch

import adjacency_model as AM
import smhc_model as M
from test_cluster_gpu import snapshot
from test_smhv_gpu import case, configure, zeros_hll

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import CRIT_NONE, CRIT_SMH_A, MODE_CB_SMH, MODE_SMH, SelhipError, Selector
from cuda_selection_criteria_amd._lib import Csr

pytestmark = pytest.mark.gpu

CAP = 4096                      # kAdjLdsCap
GUARD, SENTINEL = 64, -77
FORMS = {"directed": 0, "symmetric": 1}


def raw(pairs, values, n_rows, n_cols, form, min_value=-np.inf, short=0, with_val=True):
    """selhip_adjacency into guarded buffers of the bound's size less `short`: (rc, row_ptr, col, val, nnz, long_rows)"""
    lib = pkg.hip_lib()
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    cap = max(len(pairs) * (1 + FORMS[form]) - short, 0)
    dp = torch.from_numpy(pairs).cuda()
    dv = None if values is None else torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).cuda()
    rbuf = torch.full((n_rows + 1 + 2 * GUARD,), SENTINEL, dtype=torch.int64, device="cuda")
    cbuf = torch.full((cap + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    vbuf = torch.full((cap + 2 * GUARD,), float(SENTINEL), dtype=torch.float64, device="cuda")
    out = Csr(rbuf.data_ptr() + 8 * GUARD, cbuf.data_ptr() + 4 * GUARD, vbuf.data_ptr() + 8 * GUARD if with_val else None)
    nnz, long_rows = C.c_int64(-5), C.c_int64(-5)
    rc = lib.selhip_adjacency(dp.data_ptr() if len(pairs) else None, None if dv is None else dv.data_ptr(), len(pairs), n_rows, n_cols, FORMS[form],
                              min_value, C.byref(out), cap, C.byref(nnz), C.byref(long_rows), None)
    r, c, v = rbuf.cpu().numpy(), cbuf.cpu().numpy(), vbuf.cpu().numpy()
    kept = max(min(nnz.value, cap), 0) if rc == 0 else cap
    for a, n in ((r, n_rows + 1), (c, kept), (v, kept if with_val else 0)):               # nothing outside the arrays, nothing behind nnz
        assert np.all(a[:GUARD] == SENTINEL) and np.all(a[GUARD + n:] == SENTINEL), rc
    return rc, r[GUARD:GUARD + n_rows + 1], c[GUARD:GUARD + kept], v[GUARD:GUARD + kept], nnz.value, long_rows.value


def assert_csr(got, want, what):
    assert got[0] == 0, (what, pkg.hip_lib().selhip_last_error(None).decode())
    assert got[4] == len(want[1]), (what, got[4], len(want[1]))
    for g, w, name in zip(got[1:4], want, ("row_ptr", "col", "val")):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (what, name)


def star_noise(L, hub_last, seed):
    """(n, pairs, values): a hub with exactly L partners, as the records' i (hub = 0) or k (hub = n - 1), and 200 records among the others"""
    n = max(L + 2, 70)
    rng = np.random.default_rng(seed)
    hub, lo = (n - 1, 0) if hub_last else (0, 1)
    others = lo + rng.permutation(n - 1)[:L]
    spokes = np.stack([others, np.full(L, hub)] if hub_last else [np.full(L, hub), others], axis=1)
    pairs = np.concatenate([spokes, lo + rng.integers(0, n - 1, size=(200, 2))])
    return n, pairs, rng.random(len(pairs))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("hub_last", [False, True], ids=["hub-i-side", "hub-k-side"])
@pytest.mark.parametrize("L", [0, 1, 2, 63, 64, 65, CAP - 1, CAP, CAP + 1, 3 * CAP + 7])
def test_class_edges(L, hub_last, form):
    n, pairs, values = star_noise(L, hub_last, L + hub_last)
    rng = np.random.default_rng(L)
    for reps in (1, 3):                                                                     # each record once; three times with different values
        p, v = np.tile(pairs, (reps, 1)), np.concatenate([values + r for r in range(reps)])
        order = rng.permutation(len(p))
        p, v = p[order], v[order]
        got = raw(p, v, n, n, form)
        assert_csr(got, AM.csr(p[:, 0], p[:, 1], v, n, form == "symmetric"), (L, hub_last, form, reps))
        hub_row = reps * L if form == "symmetric" or not hub_last else 0
        assert got[5] == (hub_row > CAP), (L, hub_last, form, reps, got[5])


@pytest.mark.parametrize("form,rows", [("directed", 1), ("symmetric", 2)])
def test_one_pair_beyond_the_lds(form, rows):
    """one pair listed kAdjLdsCap + 5 times: a single column range that no LDS pass holds -- the sort through global memory"""
    values = np.random.default_rng(5).permutation(CAP + 5) / 8.0
    pairs = np.tile([[2, 5]], (CAP + 5, 1))
    got = raw(pairs, values, 8, 8, form)
    assert_csr(got, AM.csr(pairs[:, 0], pairs[:, 1], values, 8, form == "symmetric"), form)
    assert got[4] == rows and got[5] == rows and np.all(got[3] == values.max())


@pytest.mark.parametrize("form", FORMS)
def test_cuts_and_special_values(form):
    n, rng = 300, np.random.default_rng(9)
    pairs = rng.integers(0, n, size=(3000, 2))
    specials = np.array([np.nan, 0.0, -0.0, -1.5, np.inf, -np.inf, 0.25, 1.0, 5e-324, -5e-324])
    for values, cut in ((rng.random(3000), 0.5), (specials[rng.integers(0, len(specials), size=3000)], 0.0), (None, 1.0), (None, 1.5)):
        v = np.ones(3000) if values is None else values
        want = AM.csr(pairs[:, 0], pairs[:, 1], v, n, form == "symmetric", cut)
        assert_csr(raw(pairs, values, n, n, form, cut), want, (form, cut))
        got = raw(pairs, values, n, n, form, cut, with_val=False)                           # d_val = NULL
        assert got[0] == 0 and got[1].tobytes() == want[0].tobytes() and got[2].tobytes() == want[1].tobytes()
    rect = np.stack([pairs[:, 0] % 7, pairs[:, 1]], axis=1)                                 # 7 rows, 300 columns
    assert_csr(raw(rect, v, 7, n, "directed"), AM.csr(rect[:, 0], rect[:, 1], v, 7, False), "rectangle")


def test_sizes_and_refusals():
    none = np.zeros((0, 2), dtype=np.int32)
    for form in FORMS:
        got = raw(none, None, 0, 0, form)
        assert got[0] == 0 and got[1].tolist() == [0] and got[4] == 0                       # n_rows = 0
        got = raw(none, None, 5, 5, form)
        assert got[0] == 0 and got[1].tolist() == [0] * 6 and got[4] == 0                   # an empty list
    pairs, values = np.array([[0, 1], [1, 2], [0, 1], [3, 3]]), np.array([0.5, 0.25, 0.75, 1.0])
    want = AM.csr(pairs[:, 0], pairs[:, 1], values, 4, True)
    got = raw(pairs, values, 4, 4, "symmetric", short=8 - len(want[1]) + 1)                 # cap = nnz - 1
    assert got[0] == -3 and got[4] == len(want[1]) == 5 and got[1].tobytes() == want[0].tobytes()
    assert raw(pairs, values, 4, 4, "symmetric", short=8 - len(want[1]))[0] == 0            # cap = nnz
    assert raw(pairs, values, 4, 4, "directed", min_value=np.nan)[0] == -1
    assert raw(pairs, values, 3, 4, "directed")[0] == -1 and raw(pairs, values, 4, 3, "directed")[0] == -1      # a rank out of range
    assert raw(pairs, values, 4, 5, "symmetric")[0] == -1                                   # no square


# ---- the context entry, behind every kind of list ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["smh_a", "none", "topk", "pairs", "query"])
def test_behind_a_pass(oracle, kind):
    n, m = 257, 128
    stream = torch.cuda.Stream() if kind == "topk" else None                                # one case on a caller's non-blocking stream
    with Selector(0) as sel:
        assert sel.get_param("adjacency_nnz_last") == -1 and sel.get_param("adjacency_long_rows_last") == -1
        if stream is not None:
            sel.set_stream(stream.cuda_stream)
        n_rows = n
        if kind in ("smh_a", "none"):
            hll, aux, cards = M.ranked(oracle, M.hll_pool(n), M.planted_groups(n, 256, 77 + n))
            sel.upload(hll, aux, cards)
            sel.set_criterion(CRIT_SMH_A if kind == "smh_a" else CRIT_NONE)
            rec = sel.run(0.3, MODE_CB_SMH, 2, 128) if kind == "smh_a" else sel.run(0.05, MODE_CB_SMH, 1, 1)
        else:
            aux, cards = case(n, m)
            sel.upload(zeros_hll(n), aux, cards)
            configure(sel, c_min=1)
            whole = sel.run(-1.0, MODE_SMH, 7, 3, top_k=3 if kind == "topk" else 0)
            if kind == "pairs":                                                             # entries listed twice
                lst = np.concatenate([np.stack([whole["k"], whole["i"]], axis=1)[:40], np.stack([whole["i"], whole["k"]], axis=1)[:3]]).astype(np.int32)
                sel.run_pairs(lst, -1.0, MODE_SMH, 7, 3)
            elif kind == "query":
                n_rows = 5
                sel.upload_queries(zeros_hll(5), aux[:5], cards[:5])
                sel.run_queries(-1.0, MODE_SMH, 7, 3)
            rec = sel.fetch()
        assert len(rec) > 0
        before = snapshot(sel)
        sel.timing(1)
        cuts = (None, float(np.median(rec["jaccard"])))
        for form in FORMS:
            if kind == "query" and form == "symmetric":
                with pytest.raises(SelhipError, match="query pass") as err:
                    sel.adjacency(form)
                assert err.value.code == -5
                continue
            for cut in cuts:
                want = AM.csr(rec["i"], rec["k"], rec["jaccard"], n_rows, form == "symmetric", -np.inf if cut is None else cut)
                got = sel.adjacency(form, cut, to_torch=False)
                assert got["nnz"] == len(want[1]) == sel.get_param("adjacency_nnz_last") and sel.get_param("adjacency_long_rows_last") == 0
                for name, w in zip(("row_ptr", "col", "val"), want):
                    assert got[name].is_cuda and got[name].cpu().numpy().tobytes() == w.tobytes(), (kind, form, cut, name)
                assert sel.adjacency(form, cut, values=False, to_torch=False)["val"] is None
            if kind in ("topk", "pairs") and form == "symmetric":
                assert got["nnz"] < 2 * np.count_nonzero(rec["jaccard"] >= cuts[1])         # mutual neighbours, repeated entries: merged
            t = sel.adjacency(form)
            assert t.layout == torch.sparse_csr and t.is_cuda and tuple(t.shape) == (n_rows, n) and t.crow_indices().dtype == torch.int32
            args = t.crow_indices(), t.col_indices(), t.values()
            try:
                torch.sparse_csr_tensor(*args, size=t.shape, check_invariants=True)
            except (RuntimeError, NotImplementedError):                                     # (no device check in this build: on a host copy)
                torch.sparse_csr_tensor(*(a.cpu() for a in args), size=t.shape, check_invariants=True)
        assert sel.kernel_ms("adjacency") > 0
        sel.timing(0)
        assert snapshot(sel) == before                                                      # list, statistics, attempts: as they were
