"""Every instantiation of stage 2a's bit-plane histogram (csrc/kernel_hllbs.cuh) in each kernel that uses it, on the forged sets of
tests/bitplane_model.py (whose properties tests/test_bitplane_model_host.py asserts): pairs, J bits and statistics against the oracle.

  all-pairs grid   hll_union_hist_bs_kernel<NB, G1> at every (NB, G1 = T / 4) the host can launch, G1 = 0 included, as one pair per wave,
                   as runs of four on 32 waves and as the dense walk; the two rules that switch the lists off
  counts           selhip_hll_union_hist_planes: the 64 counts of every ordered pair of a ladder set with flat rows, values up to 63
  pair lists       a shuffled list with repeats and reversed entries, ungrouped and on 32 waves: a wave's cached query row changes at
                   arbitrary points of its runs and tasks; and the same list grouped
  small pass       small_pass_kernel<FMA, 4 | 5>, its khi 32 / 33 gate, walks above 24 with the next pair's kp prefetched
  query passes     query_union_hist_kernel<4 | 5 | 6> and the fused dense kernel with different khi and different maxima on the two sides
  matrices         the self and query matrix kernels over the same sets
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import bitplane_model as B
from test_exhaustive_gpu import union_cross_pairs
from test_matrix_gpu import assert_bits, jaccard_of, union_cells
from test_query_aux_gpu import union_reference as aux_union_reference

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import (ALGO_SIG, ALGO_STREAM, CRIT_HLL_A_SMH_A, CRIT_NONE, CRIT_SMH_A, FP_FMA, MODE_CB_SMH, MODE_SMH,
                                         PAIR_DTYPE, Selector)

pytestmark = pytest.mark.gpu

R, NBANDS = 4, 16                       # of the 64 equal buckets of bitplane_model.aux_equal: a shape every stage 1 takes
TAU_ALL, TAU_CB = -1.0, 0.05            # every evaluated pair is selected; a CB bound that the sets' cardinalities all pass
VMAXES = (15, 31, 51)


def oracle_pairs(oracle, hll, cards, tau, use_cb):
    pairs, st = oracle.select(hll, B.aux_equal(hll.shape[0]), cards, tau, R, NBANDS, use_cb=use_cb)
    out = np.zeros(len(pairs), dtype=PAIR_DTYPE)
    out["i"], out["k"], out["jaccard"] = pairs["i"], pairs["k"], pairs["jacc"]
    return out, st


def assert_same(got, want, what=""):
    assert got.shape[0] == want.shape[0], (what, got.shape[0], want.shape[0])
    assert np.array_equal(got["i"], want["i"]) and np.array_equal(got["k"], want["k"]), what
    bad = np.nonzero(got["jaccard"].view(np.uint64) != want["jaccard"].view(np.uint64))[0]
    assert bad.size == 0, (what, int(bad.size), [(int(got["i"][j]), int(got["k"][j])) for j in bad[:5]])


def assert_stats(st, wst, n_sel, what=""):
    assert (st["evaluated"], st["survivors"], st["selected"]) == (wst["evaluated"], wst["survivors"], n_sel), (what, st, wst)


@functools.lru_cache(maxsize=None)
def ladder_case(oracle, vmax, per):
    """a ranked ladder set, its levels, and the oracle's all-pairs results without and with the CB bound"""
    rows, level = B.ladder_set(vmax, per)
    hll, cards, _, level = B.rank_set(oracle, rows, level)
    n = hll.shape[0]
    e = cards.astype(np.int64)
    assert e.min() / e.max() > 2 * TAU_CB
    want, st = oracle_pairs(oracle, hll, cards, TAU_ALL, False)
    want_cb, st_cb = oracle_pairs(oracle, hll, cards, TAU_CB, True)
    assert len(want) == len(want_cb) == n * (n - 1) // 2
    return hll, cards, level, (want, st), (want_cb, st_cb)


# ---- 1. the all-pairs list kernel at every (NB, G1) -------------------------------------------------------------------------------
@pytest.mark.parametrize("vmax,t", B.GRID_ON + B.GRID_OFF, ids=lambda v: str(v))
def test_all_pairs_grid(oracle, vmax, t):
    hll, cards, _ = B.rank_set(oracle, B.grid_set(vmax, t))
    n = hll.shape[0]
    k = B.khi(hll)
    t_model = B.sparse_t(hll, k)
    assert t_model == (t if (vmax, t) in B.GRID_ON else 0)
    want, wst = oracle_pairs(oracle, hll, cards, TAU_ALL, False)
    want_cb, wst_cb = oracle_pairs(oracle, hll, cards, TAU_CB, True)
    assert len(want) == len(want_cb) == n * (n - 1) // 2
    with Selector(0) as sel:
        sel.upload(hll, B.aux_equal(n), cards)
        assert sel.get_param("hll_khi") == k
        # one pair per wave (the automatic choice on a list this short); 32 waves with several tasks each of four pairs, a wave's query
        # row and its sparse image kept across them ("hist_run" 64 is cut to n_pairs / 64); the dense walk (every XCD walks the whole
        # list in tasks of 64 and takes the pairs whose candidate row is its own)
        for run, dense, blocks in ((0, 32, 2048), (64, 32, 8), (0, 0, 2048)):
            sel.set_param("hist_run", run)
            sel.set_param("hist_dense_degree", dense)
            sel.set_param("hist_bs_blocks", blocks)
            for sparse in (1, 0):
                sel.set_param("hist_sparse", sparse)
                assert sel.get_param("hist_sparse_t") == (t_model if sparse else 0)
                got = sel.run(TAU_ALL, MODE_SMH, R, NBANDS)
                assert_same(got, want, (vmax, t, run, dense, blocks, sparse))
                assert_stats(sel.stats(), wst, len(want), (vmax, t, run, dense, sparse))
        sel.set_param("hist_run", 0)
        sel.set_param("hist_dense_degree", 32)
        sel.set_param("hist_sparse", 1)
        assert_same(sel.run(TAU_CB, MODE_CB_SMH, R, NBANDS), want_cb, (vmax, t, "cb"))
        assert_stats(sel.stats(), wst_cb, len(want_cb), (vmax, t, "cb"))


# ---- 2. the counts themselves -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vmax", [15, 31, 51, 63])
def test_union_counts_of_every_pair(oracle, vmax):
    """not J, whose estimator forgives a count moved between neighbouring bins of a large value: the 64 counts of every ordered pair"""
    rows, _ = B.ladder_set(min(vmax, 51), B.ladder_per(min(vmax, 51)))
    flat = B.flat_rows([v for v in B.FLAT_VALUES if v <= vmax])
    hll = np.concatenate([rows, flat] + ([B.top_row()[None]] if vmax == 63 else []))
    n = hll.shape[0]
    assert n <= 64 and int(hll.max()) == vmax
    x, y = np.divmod(np.arange(n * n, dtype=np.int32), n)
    pairs = np.ascontiguousarray(np.stack([x, y], axis=1)[np.random.default_rng(vmax).permutation(n * n)], dtype=np.int32)
    lib = pkg.hip_lib()
    dev = torch.device("cuda", 0)
    d_hll, d_pairs = torch.from_numpy(hll).to(dev), torch.from_numpy(pairs).to(dev)
    d_planes = torch.zeros((n, 6, 512), dtype=torch.int32, device=dev)
    d_gmax = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_counts = torch.full((len(pairs), 64), -1, dtype=torch.int32, device=dev)
    khi = C.c_int(0)
    pkg._lib.check(lib.selhip_hll_bitslice(d_hll.data_ptr(), n, d_planes.data_ptr(), d_gmax.data_ptr(), C.byref(khi), None))
    assert khi.value == vmax + 1 == B.khi(hll)
    assert np.array_equal(d_gmax.cpu().numpy(), hll.max(axis=1))
    pkg._lib.check(lib.selhip_hll_union_hist_planes(d_planes.data_ptr(), d_gmax.data_ptr(), khi.value, d_pairs.data_ptr(), len(pairs),
                                                    d_counts.data_ptr(), None))
    counts = d_counts.cpu().numpy().view(np.uint32)
    full_bins = set()
    for j, (a, c) in enumerate(pairs.tolist()):
        want = B.union_hist(hll[a], hll[c])
        assert np.array_equal(counts[j], want), (vmax, a, c, np.nonzero(counts[j] != want)[0].tolist())
        if want.max() == 16384:
            full_bins.add(int(want.argmax()) % 4)
        if j % 16 == 0:
            assert np.array_equal(want, oracle.union_hist(hll[a], hll[c]))
    if vmax >= 51:
        assert full_bins == {0, 1, 2, 3}                                  # a bin of 16 384 through each count formula of bs_decode


# ---- 3. pair lists ------------------------------------------------------------------------------------------------------------------
def shuffled_list(n, seed, min_len=900):
    """every pair several times (at least min_len entries), each entry with three chances in ten of coming as (larger, smaller), in
    random order: neighbouring entries nearly always have different first rows, and now and then the same"""
    rng = np.random.default_rng(seed)
    x, y = np.triu_indices(n, 1)
    L = np.tile(np.stack([x, y], axis=1).astype(np.int32), (-(-min_len // len(x)), 1))
    flip = rng.random(len(L)) < 0.3
    L[flip] = L[flip][:, ::-1]
    L = np.concatenate([L, L[rng.integers(0, len(L), 37)]])
    rng.shuffle(L)
    assert len(L) % 64
    return np.ascontiguousarray(L, dtype=np.int32)


def records_of(want, L):
    """the records of `want` (all pairs of the set) that the entries of L select, with multiplicity, sorted by (i, k)"""
    J = {(int(i), int(k)): j for i, k, j in zip(want["i"], want["k"], want["jaccard"])}
    hit = sorted((min(a, c), max(a, c)) for a, c in L.tolist())
    out = np.zeros(len(hit), dtype=PAIR_DTYPE)
    out["i"], out["k"] = zip(*hit)
    out["jaccard"] = [J[p] for p in hit]
    return out


# the list as the caller orders it: no stage-2 grouping (the library's default for sets this small), and so few waves that each takes
# several tasks of up to five consecutive entries (32 waves; the kernel gives a wave runs of n_pairs / 64 entries at most)
UNGROUPED = {"group_min_n": 2048, "hist_bs_blocks": 8, "hist_run": 5}
GROUPED = {"group_min_n": 0, "hist_bs_blocks": 2048, "hist_run": 0}


@pytest.mark.parametrize("vmax", VMAXES)
def test_pair_lists(oracle, vmax):
    """stage 1 of a list pass passes the entries on smaller rank first, in the caller's order inside each block of 512 entries: with
    UNGROUPED the histogram kernel walks that order, a wave keeps its query row across the entries of a run and across its tasks, and
    the row changes at most steps but not at all"""
    hll, cards, level, (want, _), (want_cb, _) = ladder_case(oracle, vmax, B.ladder_per(vmax))
    n = hll.shape[0]
    L = shuffled_list(n, vmax)
    row = L.min(axis=1)
    change = row[1:] != row[:-1]
    assert len(L) >= 64 * UNGROUPED["hist_run"] and change.mean() > 0.7 and np.count_nonzero(~change) >= 10
    assert np.any(level[row[1:]][change] != level[row[:-1]][change])     # ... to rows with another largest register
    rec, rec_cb = records_of(want, L), records_of(want_cb, L)
    wst = {"evaluated": len(L), "survivors": len(L)}
    t_model = B.sparse_t(hll, B.khi(hll))
    assert t_model == 4
    with Selector(0) as sel:
        sel.upload(hll, B.aux_equal(n), cards)
        for crit in (CRIT_NONE, CRIT_SMH_A):
            sel.set_criterion(crit)
            for params in (UNGROUPED, GROUPED):
                for name, value in params.items():
                    sel.set_param(name, value)
                for sparse in (0, 1):
                    sel.set_param("hist_sparse", sparse)
                    assert sel.get_param("hist_sparse_t") == (t_model if sparse else 0)
                    got = sel.run_pairs(L, TAU_ALL, MODE_SMH, R, NBANDS)
                    assert_same(got, rec, (vmax, crit, params, sparse))
                    assert_stats(sel.stats(), wst, len(rec), (vmax, crit, params, sparse))
            for name, value in UNGROUPED.items():
                sel.set_param(name, value)
            sel.set_param("hist_sparse", 0)
            assert_same(sel.run_pairs(L, TAU_CB, MODE_CB_SMH, R, NBANDS), rec_cb, (vmax, crit, "cb"))
            assert_stats(sel.stats(), wst, len(rec_cb), (vmax, crit, "cb"))


# ---- 4. the one-launch small pass -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vmax,used", [(15, 1), (23, 1), (24, 1), (31, 1), (32, 0)])
def test_small_pass(oracle, vmax, used):
    hll, cards, level, (want, wst), (want_cb, wst_cb) = ladder_case(oracle, vmax, B.per_level_for(vmax, 130))
    n = hll.shape[0]
    assert wst["survivors"] >= 130 and n - 1 > 4                          # a block's first row keeps more pairs than it has waves: kp is prefetched
    with Selector(0) as sel:
        sel.set_param("small_pass", 1)
        sel.upload(hll, B.aux_equal(n), cards)
        assert sel.get_param("hll_khi") == vmax + 1
        for _ in range(2):
            got = sel.run(TAU_ALL, MODE_SMH, R, NBANDS)
            assert sel.get_param("small_pass_used") == used
            assert_same(got, want, vmax)
            assert_stats(sel.stats(), wst, len(want), vmax)
        got = sel.run(TAU_CB, MODE_CB_SMH, R, NBANDS)
        assert sel.get_param("small_pass_used") == used
        assert_same(got, want_cb, (vmax, "cb"))
        assert_stats(sel.stats(), wst_cb, len(want_cb), (vmax, "cb"))


# ---- 5. query passes ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def query_sets(oracle, vmax_q, vmax_d):
    return B.query_case(oracle, vmax_q, vmax_d)


def check_query_passes(oracle, sel, Q, D, what):
    Q3, D3 = Q[:3], D[:3]
    for tau, mode in ((TAU_ALL, MODE_SMH), (TAU_CB, MODE_CB_SMH)):
        want, ev = union_cross_pairs(oracle, Q3, D3, tau, mode == MODE_CB_SMH, FP_FMA)
        assert len(want) == ev == len(Q[2]) * len(D[2])
        wst = {"evaluated": ev, "survivors": ev}
        sel.set_criterion(CRIT_SMH_A)
        for algo in ((ALGO_STREAM, ALGO_SIG) if mode == MODE_SMH else (ALGO_SIG,)):
            got = sel.run_queries(tau, mode, R, NBANDS, algo=algo)
            assert_same(got, want, (what, "smh_a", algo, mode))
            assert_stats(sel.stats(), wst, len(want), (what, "smh_a", algo, mode))
        sel.set_criterion(CRIT_NONE)
        for fused in ((1, 0) if mode == MODE_SMH else (1,)):
            sel.set_param("dense_fused", fused)
            got = sel.run_queries(tau, mode, 1, 1)
            assert sel.get_param("dense_route_used") == fused
            assert_same(got, want, (what, "none", fused, mode))
            assert_stats(sel.stats(), wst, len(want), (what, "none", fused, mode))


@pytest.mark.parametrize("vmax_d", VMAXES)
@pytest.mark.parametrize("vmax_q", VMAXES)
def test_query_passes(oracle, vmax_q, vmax_d):
    Q, D = query_sets(oracle, vmax_q, vmax_d)
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_aux_hll(D[4], 8)
        sel.upload_queries(Q[0], Q[1], Q[2])
        sel.upload_queries_aux_hll(Q[4], 8)
        assert sel.get_param("hll_khi") == vmax_d + 1
        check_query_passes(oracle, sel, Q, D, (vmax_q, vmax_d))
        # the two-stage criterion: the hll_a stage thins the list the histogram kernel walks
        tau = 0.5
        Qa, Da = (Q[0], Q[1], Q[2], Q[4]), (D[0], D[1], D[2], D[4])
        want, wst = aux_union_reference(oracle, Qa, Da, tau, R, NBANDS, False, FP_FMA, CRIT_HLL_A_SMH_A, 8)
        assert len(want) > 0
        sel.set_criterion(CRIT_HLL_A_SMH_A)
        got = sel.run_queries(tau, MODE_SMH, R, NBANDS)
        assert_same(got, want, (vmax_q, vmax_d, "hll_a+smh_a"))
        assert_stats(sel.stats(), wst, len(want), (vmax_q, vmax_d, "hll_a+smh_a"))


@pytest.mark.parametrize("vmax_q,vmax_d", [(15, 51), (51, 15)])
def test_query_passes_build_the_database_planes(oracle, vmax_q, vmax_d):
    """a database loaded under "hist_algo" = 0 has no planes of its own: the query pass slices D itself, with D's own khi and maxima"""
    Q, D = query_sets(oracle, vmax_q, vmax_d)
    want, ev = union_cross_pairs(oracle, Q[:3], D[:3], TAU_ALL, False, FP_FMA)
    with Selector(0) as sel:
        sel.set_param("hist_algo", 0)
        sel.upload(D[0], D[1], D[2])
        assert sel.get_param("hist_bitplanes") == 0
        sel.upload_queries(Q[0], Q[1], Q[2])
        for algo in (ALGO_STREAM, ALGO_SIG):
            for _ in range(2):                                            # (the second pass finds the planes the first one built)
                got = sel.run_queries(TAU_ALL, MODE_SMH, R, NBANDS, algo=algo)
                assert_same(got, want, (vmax_q, vmax_d, algo))
                assert_stats(sel.stats(), {"evaluated": ev, "survivors": ev}, len(want), (vmax_q, vmax_d, algo))


# ---- 6. matrices ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vmax_d", VMAXES)
@pytest.mark.parametrize("vmax_q", VMAXES)
def test_matrices(oracle, vmax_q, vmax_d):
    Q, D = query_sets(oracle, vmax_q, vmax_d)
    U = union_cells(oracle, Q[0], D[0], FP_FMA)
    J = jaccard_of(U, Q[2], D[2])
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        assert_bits(sel.query_matrix("union"), U, "query union")
        assert_bits(sel.query_matrix("jaccard"), J, "query jaccard")
    # the self matrix over Q u D in its own rank order
    hll, cards, _ = B.rank_set(oracle, np.concatenate([Q[0], D[0]]))
    U = union_cells(oracle, hll, hll, FP_FMA)
    J = jaccard_of(U, cards, cards, diagonal_one=True)
    with Selector(0) as sel:
        sel.upload(hll, B.aux_equal(hll.shape[0]), cards)
        assert sel.get_param("hll_khi") == max(vmax_q, vmax_d) + 1
        assert_bits(sel.matrix("union"), U, "union")
        assert_bits(sel.matrix("jaccard"), J, "jaccard")
