"""Criterion smh_c (SELHIP_CRIT_SMH_C) on the GPU: a pair of the pass's pair space survives stage 1 iff at least c_min of its m
SuperMinHash buckets are equal.  Expected records and statistics come from tests/smhc_model.py: the `none` ground truth of the oracle
filtered by a numpy bucket count, and -- independent of numpy -- the oracle's own smh_a at the two ends c_min = 1 and c_min = m.
Records are compared with == on (i, k, J bits); the kernel that ran ("smhc_path_used") is read back."""
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import smhc_model as M
from smh_matrix_model import half_equal, planted_all_but_one, planted_single
from test_allpairs_topk_host import nbr_reference
from test_query_topk_host import topk_reference

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import (CRIT_NONE, CRIT_SMH_A, CRIT_SMH_C, FP_FMA, FP_STRICT, MODE_CB_SMH, MODE_SMH, PAIR_DTYPE, SelhipError,
                                         Selector)
from cuda_selection_criteria_amd.selection import multi_select

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
FAST_M = (128, 256, 512, 1024)
GENERIC_M = (1, 3, 64, 100, 192, 2048)


def run_c(sel, c_min, tau, mode, rows=None):
    """one all-pairs pass under smh_c; the band shape handed over is NOT a factorisation of m: the criterion ignores it"""
    sel.set_criterion(CRIT_SMH_C)
    sel.set_min_matches(c_min)
    got = sel.run(tau, mode, 7, 3, rows=rows)
    return got, sel.stats()


def assert_pass(got, st, want, wst, what=""):
    assert M.tuples(got) == M.tuples(want), (what, len(got), len(want))
    assert st == wst, (what, st, wst)
    assert st["survivors"] == st["candidates"]


def assert_path(sel, m):
    assert sel.get_param("smhc_path_used") == (1 if m in FAST_M else 0), m


def merged(parts):
    out = np.concatenate(parts) if parts else np.zeros(0, dtype=PAIR_DTYPE)
    return out[np.lexsort((out["k"], out["i"]))]


def thresholds(m):
    return sorted({1, max(1, m // 2), m})


# ---- 1. the influenza fixtures ---------------------------------------------------------------------------------------------------
INFLUENZA = {512: ((1, 21, 48, 87, 481, 502, 507), (45, 13, 12, 7, 6, 1, 0)), 64: ((1, 8, 9, 63, 64), (27, 8, 7, 2, 0))}


def selection(args):
    out = subprocess.run([str(BIN / "selection")] + args, cwd=GOLDEN, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return out.stdout


@pytest.mark.parametrize("m", [512, 64])
@pytest.mark.parametrize("fp", [FP_FMA, FP_STRICT])
def test_influenza(oracle, monkeypatch, m, fp):
    monkeypatch.chdir(GOLDEN)
    ds = pkg.load_dataset("influenza_filelist.txt", m, 0, fp)
    c_mins, n_records = INFLUENZA[m]
    truth = M.Truth(oracle, ds.hll, ds.aux, ds.cards, -1.0, False, fp)
    ends = M.oracle_ends(oracle, ds.hll, ds.aux, ds.cards, -1.0, False, fp)
    assert len(truth.none) == 45
    with Selector(0, fp) as sel:
        sel.upload(ds.hll, ds.aux, ds.cards)
        for c_min, n_rec in zip(c_mins, n_records):
            got, st = run_c(sel, c_min, -1.0, MODE_SMH)
            print(f"influenza m={m} fp={fp} c_min={c_min}: {st}")
            assert len(got) == n_rec, (c_min, len(got), n_rec)
            assert_pass(got, st, *truth.expected(c_min), what=c_min)
            if c_min in ends:
                assert_pass(got, st, *ends[c_min], what=("oracle", c_min))
            assert_path(sel, m)
            # the file-list helper and the CLI print these records
            text = pkg.format_lines(ds.names, got)
            flag = "1" if fp == FP_FMA else "0"
            assert pkg.select_from_filelist("influenza_filelist.txt", -1.0, 8 * m, mode=MODE_SMH, fp_mode=fp, criterion="smh_c", min_matches=c_min) == text
            assert selection(["-l", "influenza_filelist.txt", "-c", "smh_c", "-C", str(c_min), "-a", str(8 * m), "-h", "-1", "-n", "-F", flag]) == text
            assert len(text.splitlines()) == n_rec
        # tau = 0.9 with the CB bound
        cb = M.Truth(oracle, ds.hll, ds.aux, ds.cards, 0.9, True, fp)
        for c_min in c_mins:
            got, st = run_c(sel, c_min, 0.9, MODE_CB_SMH)
            assert_pass(got, st, *cb.expected(c_min), what=("cb", c_min))
        assert selection(["-l", "influenza_filelist.txt", "-c", "smh_c", "-C", "1", "-a", str(8 * m), "-h", "0.9", "-F", "1" if fp == FP_FMA else "0"]) == \
            pkg.format_lines(ds.names, cb.expected(1)[0])


# ---- 2. shapes -------------------------------------------------------------------------------------------------------------------
_NONE = {}


def shaped(oracle, n, m, tau, use_cb, seed=0):
    """(hll, aux, cards, truth) of n pooled genomes with planted bucket groups; the HLL side of the truth is computed once per (n, tau, mode)"""
    hll, aux, cards = M.ranked(oracle, M.hll_pool(n), M.planted_groups(n, m, 1000 * m + n + seed))
    key = (n, tau, use_cb)
    if key not in _NONE:
        _NONE[key] = M.Truth(oracle, hll, np.zeros((n, 1), dtype=np.uint64), cards, tau, use_cb)
    truth = M.Truth.__new__(M.Truth)
    truth.none, truth.st, truth.E = _NONE[key].none, _NONE[key].st, _NONE[key].E
    truth.counts = M.match_counts(aux, aux)
    truth.n, truth.m = aux.shape
    return hll, aux, cards, truth


@pytest.mark.parametrize("m", GENERIC_M + FAST_M)
def test_shapes(oracle, m):
    sizes = [1, 2, 3, 5, 25, 63, 64, 65, 129] + ([1030] if m == 128 else [])
    with Selector(0) as sel:
        for n in sizes:
            use_cb = n % 2 == 1
            tau = 0.3
            hll, aux, cards, truth = shaped(oracle, n, m, tau, use_cb)
            ends = M.oracle_ends(oracle, hll, aux, cards, tau, use_cb) if n in (65, 1030) else {}
            sel.upload(hll, aux, cards)
            for c_min in thresholds(m):
                got, st = run_c(sel, c_min, tau, MODE_CB_SMH if use_cb else MODE_SMH)
                want, wst = truth.expected(c_min)
                assert_pass(got, st, want, wst, what=(m, n, c_min))
                if c_min in ends:
                    assert_pass(got, st, *ends[c_min], what=("oracle", m, n, c_min))
                if n >= 25 and m > 1:
                    assert 0 < wst["survivors"] < wst["evaluated"], (m, n, c_min, wst)      # a proper, non-empty subset
                if n >= 2:
                    assert_path(sel, m)
    # (n = 1030: candidates cross a kChunk = 1024 boundary; 25, 63, 65, 129, 1030 are no multiples of the tile heights 12, 6, 3)


# ---- 3. every bucket position ----------------------------------------------------------------------------------------------------
def zero_pairs(oracle, hll, cards, g0):
    """the exhaustive records (tau = -1, no CB) of every pair that holds rank g0, by (i, k)"""
    out = []
    for g in range(len(cards)):
        if g != g0:
            i, k = min(g, g0), max(g, g0)
            out.append((i, k, np.float64(oracle.jaccard(hll[i], hll[k], cards[i], cards[k])).view(np.uint64).item()))
    return sorted(out)


@pytest.mark.parametrize("m", [128, 256, 512, 1024, 100])
def test_every_bucket_position(oracle, m):
    n = m + 1
    pool = M.hll_pool(n)
    with Selector(0) as sel:
        for rows, hit, miss in ((planted_single(m, 31 + m), 1, 2), (planted_all_but_one(m, 37 + m), m - 1, m)):
            # genome 0 goes to the middle of the cardinality order: it is a query row for the ranks above it and a candidate of the ring
            # for the ranks below
            order = np.argsort(M.ranked(oracle, pool, np.arange(n)[:, None].astype(np.uint64))[1][:, 0])     # rank of every pool row
            src = np.arange(n)
            mid = int(np.nonzero(order == n // 2)[0][0])
            src[[0, mid]] = src[[mid, 0]]                     # pool row `mid` (rank n / 2) carries bucket row 0
            aux_by_pool = np.empty_like(rows)
            aux_by_pool[src] = rows
            hll, aux, cards = M.ranked(oracle, pool, aux_by_pool)
            g0 = n // 2
            assert np.array_equal(aux[g0], rows[0])
            sel.upload(hll, aux, cards)
            got, st = run_c(sel, hit, -1.0, MODE_SMH)
            want = zero_pairs(oracle, hll, cards, g0)
            assert M.tuples(got) == want, (m, hit)
            assert np.count_nonzero(got["i"] == g0) > 0 and np.count_nonzero(got["k"] == g0) > 0
            assert st == {"evaluated": n * (n - 1) // 2, "survivors": m, "selected": m, "candidates": m}
            if hit == 1:
                assert_pass(got, st, *M.oracle_ends(oracle, hll, aux, cards, -1.0, False)[1], what="oracle")
            got, st = run_c(sel, miss, -1.0, MODE_SMH)
            assert len(got) == 0 and st["survivors"] == 0 and st["evaluated"] == n * (n - 1) // 2, (m, miss, st)
            assert_path(sel, m)


# ---- 4. boundaries, dwords, empty rows ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [128, 256, 512, 1024, 100])
def test_boundary_triples(oracle, m):
    pool = M.hll_pool(4)
    with Selector(0) as sel:
        for c_min in sorted({1, 2, 63, 64, 65, m // 2, m - 1, m}):
            for perm in ([0, 1, 2, 3], [3, 2, 1, 0]):          # the base as the first and as the last rank
                rows = M.boundary_triple_rows(m, c_min, 7 * m + c_min)
                hll, cards = M.ranked(oracle, pool, np.zeros((4, 1), dtype=np.uint64))[::2]
                aux = rows[perm]
                truth = M.Truth(oracle, hll, aux, cards, -1.0, False)
                sel.upload(hll, aux, cards)
                got, st = run_c(sel, c_min, -1.0, MODE_SMH)
                want, wst = truth.expected(c_min)
                assert_pass(got, st, want, wst, what=(m, c_min, perm))
                # the base row with the rows that share c_min - 1, c_min and c_min + 1 (at most m) buckets with it
                base, found = perm.index(0), {(i, k) for i, k, _ in M.tuples(got)}
                assert [tuple(sorted((base, perm.index(j)))) in found for j in (1, 2, 3)] == [False, True, True], (m, c_min, perm)


@pytest.mark.parametrize("m", [128, 512, 100])
def test_buckets_that_differ_in_one_dword(oracle, m):
    n = 40
    hll, aux, cards = M.ranked(oracle, M.hll_pool(n), half_equal(n, m, 11 + m))
    truth = M.Truth(oracle, hll, aux, cards, -1.0, False)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        seen = set()
        for c_min in sorted({1, m // 3, m // 2, m // 2 + 1, m - m // 3, m - 1, m}):
            got, st = run_c(sel, c_min, -1.0, MODE_SMH)
            assert_pass(got, st, *truth.expected(c_min), what=(m, c_min))
            seen.add(len(got))
        assert len(seen) > 2 and 0 in seen                    # (no two rows are equal: nothing at c_min = m)


@pytest.mark.parametrize("m", [256, 100])
def test_empty_rows(oracle, m):
    n = 30
    hll = M.hll_pool(n)
    aux = M.planted_groups(n, m, 5, shares=[1, m // 2, m - 1])
    aux[[3, 9, 20, 21, 22]] = M.EMPTY                         # empty SuperMinHash rows ...
    hll[[20, 21]] = 0                                         # ... two of them of genomes whose HLL sketch is empty too (e = 0)
    hll, aux, cards = M.ranked(oracle, hll, aux)
    assert np.all(cards[:2] == 0) and cards[2] > 0 and np.all(aux[:2] == M.EMPTY)
    for mode, tau in ((MODE_SMH, -1.0), (MODE_CB_SMH, 0.2)):
        truth = M.Truth(oracle, hll, aux, cards, tau, mode == MODE_CB_SMH)
        ends = M.oracle_ends(oracle, hll, aux, cards, tau, mode == MODE_CB_SMH)
        with Selector(0) as sel:
            sel.upload(hll, aux, cards)
            for c_min in (1, m // 2, m):
                got, st = run_c(sel, c_min, tau, mode)
                want, wst = truth.expected(c_min)
                assert_pass(got, st, want, wst, what=(m, mode, c_min))
                if c_min in ends:
                    assert_pass(got, st, *ends[c_min], what="oracle")
            if mode == MODE_SMH:
                # two empty rows count m: the three empty rows of non-empty genomes pair up, and each pairs with the two e = 0 ranks
                # only as the candidate (e_k != 0): 3 + 2 * 3 pairs at c_min = m
                assert wst["survivors"] == 9 and not np.any(want["k"] < 2)


# ---- 5. CB windows, zero cardinalities, partitions, overflow ---------------------------------------------------------------------
def test_cb_windows_and_zero_cardinalities(oracle):
    n, m, tau = 300, 128, 0.9
    hll = M.hll_pool(n)
    hll[:3] = 0
    hll, aux, cards = M.ranked(oracle, hll, M.planted_groups(n, m, 77))
    assert np.all(cards[:3] == 0) and cards[3] > 0
    e = cards.astype(np.int64).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        hi = np.array([np.max(np.nonzero((e == 0) | (e[i] / e >= np.float64(np.float32(tau))))[0]) for i in range(n)])
    assert any(len(set(hi[t:t + 12].tolist())) > 1 for t in range(0, n, 12))        # tiles whose rows end at different candidates
    truth = M.Truth(oracle, hll, aux, cards, tau, True)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        for c_min in thresholds(m):
            got, st = run_c(sel, c_min, tau, MODE_CB_SMH)
            want, wst = truth.expected(c_min)
            assert_pass(got, st, want, wst, what=c_min)
            assert wst["evaluated"] < (n - 3) * (n - 4) // 2 + 3 * (n - 3)          # the bound cut something
        assert not np.any(truth.none["k"] < 3)


@pytest.mark.parametrize("m", [256, 100])
def test_partitions_add_up(oracle, m):
    n, tau, c_min = 700, 0.3, max(1, m // 2)
    hll, aux, cards, truth = shaped(oracle, n, m, tau, True)
    want, wst = truth.expected(c_min)
    assert 0 < len(want)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        parts, sts = [], []
        for rb, re in ((0, 1), (1, 130), (130, 130), (130, 699), (699, n)):
            got, st = run_c(sel, c_min, tau, MODE_CB_SMH, rows=(rb, re))
            assert_pass(got, st, *truth.expected(c_min, rows=(rb, re)), what=(rb, re))
            parts.append(got); sts.append(st)
        assert M.tuples(merged(parts)) == M.tuples(want)
        assert sum(s["evaluated"] for s in sts) == wst["evaluated"] and sum(s["survivors"] for s in sts) == wst["survivors"]
        parts, sts = [], []
        for part in range(3):
            sel.set_row_interleave(32, 3, part)
            got, st = run_c(sel, c_min, tau, MODE_CB_SMH)
            parts.append(got); sts.append(st)
        sel.set_row_interleave(32, 1, 0)
        assert M.tuples(merged(parts)) == M.tuples(want)
        assert sum(s["evaluated"] for s in sts) == wst["evaluated"] and sum(s["survivors"] for s in sts) == wst["survivors"]
        h = 333
        sel.set_candidate_begin(h)
        got, st = run_c(sel, c_min, tau, MODE_CB_SMH, rows=(0, h))
        sel.set_candidate_begin(0)
        assert_pass(got, st, *truth.expected(c_min, rows=(0, h), cand_begin=h), what="cand_begin")
        sel.set_pipeline(2)
        got, st = run_c(sel, c_min, tau, MODE_CB_SMH)
        assert sel.get_param("chunks") == 2
        assert_pass(got, st, want, wst, what="pipeline")


@pytest.mark.parametrize("m", [128, 100])
def test_survivor_list_overflow(oracle, m):
    n = 300
    aux = M.planted_groups(n, m, 9)
    aux[:, : m // 2] = aux[0, : m // 2]                        # every pair shares half its buckets
    hll, aux, cards = M.ranked(oracle, M.hll_pool(n), aux)
    truth = M.Truth(oracle, hll, aux, cards, 0.3, False)
    want, wst = truth.expected(m // 2)
    assert wst["survivors"] == n * (n - 1) // 2
    with Selector(0) as sel:
        sel.set_param("init_cap", 1024)
        sel.upload(hll, aux, cards)
        got, st = run_c(sel, m // 2, 0.3, MODE_SMH)
        assert sel.last_attempts() > 1
        assert_pass(got, st, want, wst)


# ---- 6. pair lists ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [128, 1024, 100])
def test_pair_lists(oracle, m):
    n, tau = 129, 0.3
    hll, aux, cards, truth = shaped(oracle, n, m, tau, True)
    rng = np.random.default_rng(m)
    x = rng.integers(0, n, size=4000)
    y = rng.integers(0, n, size=4000)
    lst = np.stack([x, y], axis=1)[x != y].astype(np.int32)
    lst = np.concatenate([lst, lst[:300], lst[300:600, ::-1]])              # entries listed twice, in both orders
    lo, hi = lst.min(axis=1), lst.max(axis=1)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        for c_min in thresholds(m):
            all_pairs, _ = truth.expected(c_min)
            j_of = {(i, k): j for i, k, j in M.tuples(all_pairs)}
            want = sorted((int(a), int(b), j_of[(int(a), int(b))]) for a, b in zip(lo, hi) if (int(a), int(b)) in j_of)
            in_e = truth.E[lo, hi]
            surv = int(np.count_nonzero(in_e & (truth.counts[lo, hi] >= c_min)))
            sel.set_criterion(CRIT_SMH_C)
            sel.set_min_matches(c_min)
            got = sel.run_pairs(lst, tau, MODE_CB_SMH, 7, 3)
            assert M.tuples(got) == want, (m, c_min)
            assert sel.stats() == {"evaluated": int(in_e.sum()), "survivors": surv, "selected": len(want), "candidates": surv}
            assert len(want) > 0
        assert sel.get_param("pairs_route_used") == 0
        for bad in ([[0, n]], [[-1, 2]], [[5, 5]]):
            with pytest.raises(SelhipError, match="invalid entries"):
                sel.run_pairs(np.array([[0, 1]] + bad, dtype=np.int32), tau, MODE_CB_SMH, 7, 3)


# ---- 7. query passes ----------------------------------------------------------------------------------------------------------------
_CROSS = {}


def query_case(oracle, n_q, n_d, m, tau, use_cb):
    pool = M.hll_pool(n_q + n_d)
    rows = M.planted_groups(n_q + n_d, m, 3 * m + n_q + n_d)
    pick = np.zeros(n_q + n_d, dtype=bool)
    pick[np.random.default_rng(n_q * 1000 + n_d).choice(n_q + n_d, n_q, replace=False)] = True
    Q, D = M.ranked(oracle, pool[pick], rows[pick]), M.ranked(oracle, pool[~pick], rows[~pick])
    key = (n_q, n_d, tau, use_cb)
    if key not in _CROSS:
        _CROSS[key] = M.cross_none(oracle, Q, D, tau, use_cb)
    return Q, D, _CROSS[key]


@pytest.mark.parametrize("n_q", [1, 5, 7])
def test_queries_equal_cross_pairs(oracle, n_q):
    n_rec = 0
    with Selector(0) as sel:
        for m in (128, 512, 100):
            for n_d in (1, 64, 65, 200):
                for mode in (MODE_CB_SMH, MODE_SMH):
                    tau = 0.3
                    Q, D, (none, E) = query_case(oracle, n_q, n_d, m, tau, mode == MODE_CB_SMH)
                    sel.upload(D[0], D[1], D[2])
                    sel.upload_queries(Q[0], Q[1], Q[2])
                    sel.set_criterion(CRIT_SMH_C)
                    for c_min in thresholds(m):
                        sel.set_min_matches(c_min)
                        got = sel.run_queries(tau, mode, 7, 3)
                        want, wst = M.cross_expected(none, E, Q[1], D[1], c_min)
                        assert_pass(got, sel.stats(), want, wst, what=(n_q, n_d, m, mode, c_min))
                        assert_path(sel, m)
                        n_rec += len(want)
    assert n_rec > 0


def test_queries_top_k(oracle):
    m, tau = 128, -1.0
    Q, D, (none, E) = query_case(oracle, 7, 200, m, tau, False)
    aux_d = D[1].copy()
    aux_d[:, : m // 4] = Q[1][0, : m // 4]                     # every database row shares a quarter of its buckets with query 0
    with Selector(0) as sel:
        sel.upload(D[0], aux_d, D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        sel.set_criterion(CRIT_SMH_C)
        sel.set_min_matches(m // 4)
        whole, _ = M.cross_expected(none, E, Q[1], aux_d, m // 4)
        assert np.count_nonzero(whole["i"] == 0) == 200
        got = sel.run_queries(tau, MODE_SMH, 7, 3, top_k=3)
        assert M.tuples(got) == M.tuples(topk_reference(whole, 3))
        assert sel.stats()["selected"] == len(whole)
        assert M.tuples(sel.fetch()) == M.tuples(merged([topk_reference(whole, 3)]))
        sel.set_query_topk(0)


def test_all_pairs_top_k(oracle):
    n, m, tau = 129, 256, 0.3
    hll, aux, cards, truth = shaped(oracle, n, m, tau, False)
    want, wst = truth.expected(1)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        sel.set_criterion(CRIT_SMH_C)
        sel.set_min_matches(1)
        got = sel.run(tau, MODE_SMH, 7, 3, top_k=2)
        assert M.tuples(got) == M.tuples(nbr_reference(want, 2)) and len(got) > 0
        assert sel.stats() == wst
        sel.set_allpairs_topk(0)


# ---- 8. neighbours and refusals -----------------------------------------------------------------------------------------------------
def test_neighbours_and_nesting(oracle):
    n, m, tau = 200, 256, 0.3
    hll, aux, cards, truth = shaped(oracle, n, m, tau, True)
    r, b = 2, 128
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        sel.set_criterion(CRIT_SMH_A)
        smh_before, smh_st = sel.run(tau, MODE_CB_SMH, r, b), sel.stats()
        sel.set_criterion(CRIT_NONE)
        none_before, none_st = sel.run(tau, MODE_CB_SMH, 1, 1), sel.stats()
        assert M.tuples(none_before) == M.tuples(truth.none) and len(smh_before) > 0
        prev = None
        for c_min in (1, 2, m // 2 - 1, m // 2, m // 2 + 1, m - 1, m):
            got, st = run_c(sel, c_min, tau, MODE_CB_SMH)
            assert_pass(got, st, *truth.expected(c_min), what=c_min)
            if prev is not None:
                assert set(M.tuples(got)) <= prev                        # nested in c_min
            prev = set(M.tuples(got))
            assert prev <= set(M.tuples(none_before))
        sel.set_criterion(CRIT_SMH_A)
        assert M.tuples(sel.run(tau, MODE_CB_SMH, r, b)) == M.tuples(smh_before) and sel.stats() == smh_st
        sel.set_criterion(CRIT_NONE)
        assert M.tuples(sel.run(tau, MODE_CB_SMH, 1, 1)) == M.tuples(none_before) and sel.stats() == none_st
        # a band of r buckets entirely equal has r equal buckets: smh_a's records are among smh_c's at c_min = r
        got, _ = run_c(sel, r, tau, MODE_CB_SMH)
        assert set(M.tuples(smh_before)) <= set(M.tuples(got))


def test_refusals(oracle):
    n, m = 20, 128
    hll, aux, cards, _ = shaped(oracle, n, m, 0.3, False)
    lst = np.array([[0, 1], [2, 3]], dtype=np.int32)
    with Selector(0) as sel:
        sel.set_criterion(CRIT_SMH_C)
        with pytest.raises(SelhipError, match="smh_c"):           # no bucket rows at all
            sel.run(0.3, MODE_SMH, 1, 1, rows=(0, 0))
        sel.upload(hll, aux, cards)
        sel.upload_queries(hll[:3], aux[:3], cards[:3])
        sel.set_criterion(CRIT_NONE)
        before, st_before = sel.run(0.3, MODE_SMH, 1, 1), sel.stats()
        sel.set_criterion(CRIT_SMH_C)
        runs = (lambda: sel.run(0.3, MODE_SMH, 1, 1), lambda: sel.run_queries(0.3, MODE_SMH, 1, 1), lambda: sel.run_pairs(lst, 0.3, MODE_SMH, 1, 1))
        for run in runs:                                           # never set
            with pytest.raises(SelhipError, match="smh_c.*set_min_matches"):
                run()
        for bad in (0, -1, -(1 << 31)):
            with pytest.raises(SelhipError, match="min_matches"):
                sel.set_min_matches(bad)
        for run in runs:                                           # the refused values left it unset
            with pytest.raises(SelhipError, match="smh_c"):
                run()
        sel.set_min_matches(m + 1)
        for run in runs:
            with pytest.raises(SelhipError, match="smh_c.*exceeds"):
                run()
        # a refusal claims no counter set and leaves the context usable
        sel.set_criterion(CRIT_NONE)
        assert M.tuples(sel.run(0.3, MODE_SMH, 1, 1)) == M.tuples(before) and sel.stats() == st_before
        sel.set_criterion(CRIT_SMH_C)
        sel.set_min_matches(m)
        sel.run(0.3, MODE_SMH, 1, 1)
        with pytest.raises(SelhipError):
            sel.set_criterion(6)
    with pytest.raises(SelhipError, match="smh_c"):
        pkg.ooc_select(hll, aux, cards, 0.3, 10, n_rows=1, n_bands=m, criterion=CRIT_SMH_C)
    with pytest.raises(SelhipError, match="smh_c"):
        multi_select([0], hll, aux, cards, 0.3, n_rows=1, n_bands=m, gather=0, criterion=CRIT_SMH_C)


# ---- 9. the other front ends on the influenza fixtures -----------------------------------------------------------------------------
def test_cli_queries_pair_lists_and_top_k(tmp_path, monkeypatch):
    monkeypatch.chdir(GOLDEN)
    names = [l.strip() for l in (GOLDEN / "influenza_filelist.txt").read_text().splitlines() if l.strip()]
    q_names, d_names = names[::3], [x for j, x in enumerate(names) if j % 3]
    (tmp_path / "q.txt").write_text("\n".join(q_names) + "\n")
    (tmp_path / "d.txt").write_text("\n".join(d_names) + "\n")
    q, d = str(tmp_path / "q.txt"), str(tmp_path / "d.txt")
    crit = ["-c", "smh_c", "-C", "21", "-a", "4096", "-h", "-1", "-n"]
    kw = dict(mode=MODE_SMH, criterion="smh_c", min_matches=21)
    union = selection(["-l", "influenza_filelist.txt"] + crit)
    assert len(union.splitlines()) == 13
    # query passes: the cross pairs of the all-pairs output
    want = set()
    for line in union.splitlines():
        a, b, j = line.split(" ")
        if (a in q_names) != (b in q_names):
            want.add((a, b, j) if a in q_names else (b, a, j))
    got = selection(["-l", d, "-q", q] + crit)
    assert {tuple(l.split(" ")) for l in got.splitlines()} == want and len(got.splitlines()) == len(want) > 0
    assert pkg.query_from_filelists(q, d, -1.0, 4096, **kw) == got
    best = selection(["-l", d, "-q", q, "-k", "1"] + crit)
    assert best == pkg.query_from_filelists(q, d, -1.0, 4096, top_k=1, **kw) and 0 < len(best.splitlines()) <= len(q_names)
    # a pair list: one run's output is the next run's list, and a stricter threshold keeps its share of it
    (tmp_path / "p.txt").write_text(union)
    p = str(tmp_path / "p.txt")
    assert selection(["-l", "influenza_filelist.txt", "-p", p] + crit) == union
    strict = selection(["-l", "influenza_filelist.txt", "-p", p, "-c", "smh_c", "-C", "87", "-a", "4096", "-h", "-1", "-n"])
    assert strict == selection(["-l", "influenza_filelist.txt", "-c", "smh_c", "-C", "87", "-a", "4096", "-h", "-1", "-n"]) and len(strict.splitlines()) == 7
    assert pkg.select_pairs_from_filelist("influenza_filelist.txt", p, -1.0, 4096, mode=MODE_SMH, criterion="smh_c", min_matches=87) == strict
    # every genome's best partner
    nbr = selection(["-l", "influenza_filelist.txt", "-K", "1"] + crit)
    assert nbr == pkg.select_from_filelist("influenza_filelist.txt", -1.0, 4096, top_k=1, **kw) and len(nbr.splitlines()) > 0
