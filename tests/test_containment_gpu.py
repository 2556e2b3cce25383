"""The containment measures on the GPU: selhip_ctx_set_measure (max containment in stage 2 of every pass kind) and the matrix measures
SELHIP_MEASURE_INTERSECTION / _CONTAINMENT / _MAX_CONTAINMENT.  Expected values never come from the library: U is oracle.union_size
under oracle.set_fma(flavour), the values are containment_model.py's numpy float64 expressions on the truncated cardinalities, the
stage-1 set of smh_a is the oracle's select at tau = -1 without CB and that of smh_c the bucket count of smh_matrix_model.py.  Records
are compared with == on (i, k, value bits), matrices as uint64 patterns (two NaNs count as equal)."""
import functools
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import containment_model as cm
from smh_matrix_model import match_counts
from test_allpairs_topk_host import nbr_reference
from test_matrix_gpu import assert_bits
from test_matrix_host import read_matrix, same_bits
from test_query_topk_host import topk_reference

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd._lib import check
from cuda_selection_criteria_amd import (ALGO_AUTO, ALGO_HASHJOIN, ALGO_INDEX, ALGO_SIG, ALGO_STREAM, CRIT_HLL_A, CRIT_HLL_A_SMH_A, CRIT_HLL_AN,
                                         CRIT_NONE, CRIT_SMH_A, CRIT_SMH_C, FP_FMA, FP_STRICT, MEASURE_JACCARD, MEASURE_MAX_CONTAINMENT,
                                         MODE_CB_SMH, MODE_SMH, PAIR_DTYPE, SelhipError, Selector)

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
FLAVOURS = [FP_FMA, FP_STRICT]
ROUTES = (1, 0)                                  # "dense_fused": the fused kernel, the list route
MATRIX_MEASURES = ("intersection", "containment", "max_containment")
R, B = 8, 32                                     # the band shape of the smh_a cases: m = 256 buckets in 32 bands of 8
tuples = cm.tuples


class Case:
    """a ranked sketch set with the model's values of every pair"""

    def __init__(self, oracle, hll, aux, fp=FP_FMA, cards=None, cells=None):
        if cards is None:
            self.hll, self.aux, self.cards, self.perm = cm.ranked(oracle, hll, aux, fp)
        else:
            self.hll, self.aux, self.cards, self.perm = hll, aux, np.asarray(cards, dtype=np.float64), np.arange(len(cards))
        self.n, self.fp = len(self.cards), fp
        self.U = cm.union_matrix(oracle, self.hll, self.hll, fp, cells=cells, symmetric=cells is None)
        self.val = cm.values(self.U, self.cards, self.cards)
        self.V = self.val["max_containment"]
        self.E = cm.pair_space(self.cards)

    def expected(self, tau, S=None, rows=None, cand_begin=0, measure="max_containment"):
        """(records, statistics without the candidates) of a MODE_SMH pass whose stage 1 passes the pairs of the bool matrix S"""
        E = self.E
        if rows is not None or cand_begin:
            rb, re = rows if rows is not None else (0, self.n)
            inside = np.zeros_like(E)
            inside[rb:re, cand_begin:] = True
            E = E & inside
        surv = E if S is None else E & S
        rec = cm.select(self.val[measure], surv, tau)
        return rec, {"evaluated": int(E.sum()), "survivors": int(surv.sum()), "selected": len(rec)}


def stats3(sel):
    st = sel.stats()
    return {k: st[k] for k in ("evaluated", "survivors", "selected")}


def assert_pass(sel, got, want, wst, what=""):
    assert tuples(got) == tuples(want), (what, len(got), len(want))
    assert stats3(sel) == wst, (what, sel.stats(), wst)


@functools.lru_cache(maxsize=None)
def spread_case(oracle, n, fp=FP_FMA):
    return Case(oracle, *cm.spread_rows(n), fp)


def run_none(sel, tau, fused=1, rows=None, top_k=None):
    sel.set_criterion(CRIT_NONE)
    sel.set_param("dense_fused", fused)
    got = sel.run(tau, MODE_SMH, 1, 1, rows=rows, top_k=top_k)
    assert sel.get_param("dense_route_used") == fused
    return got


def smh_a_set(oracle, case, r=R, b=B):
    """bool [n, n]: the pairs smh_a passes, from the oracle's select at tau = -1 without CB"""
    oracle.set_fma(case.fp)
    try:
        pairs, _ = oracle.select(case.hll, case.aux, case.cards, -1.0, r, b, use_cb=False, criterion=0)
    finally:
        oracle.set_fma(1)
    S = np.zeros((case.n, case.n), dtype=bool)
    S[pairs["i"], pairs["k"]] = True
    return S


def merged(parts):
    out = np.concatenate(parts) if parts else np.zeros(0, dtype=PAIR_DTYPE)
    return out[np.lexsort((out["k"], out["i"]))]


# ---- 1. the influenza fixtures: Selector, the file-list helpers, the CLI ------------------------------------------------------------
def selection(args, cwd=GOLDEN):
    out = subprocess.run([str(BIN / "selection")] + args, cwd=cwd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return out.stdout


@pytest.mark.parametrize("fused", ROUTES)
@pytest.mark.parametrize("fp", FLAVOURS)
def test_influenza(oracle, monkeypatch, fp, fused):
    monkeypatch.chdir(GOLDEN)
    ds = pkg.load_dataset("influenza_filelist.txt", 0, 0, fp)
    case = Case(oracle, ds.hll, np.zeros((10, 1), dtype=np.uint64), fp, cards=ds.cards)
    flag = "1" if fp == FP_FMA else "0"
    with Selector(0, fp) as sel:
        sel.upload(case.hll, case.aux, case.cards)
        sel.set_measure("max_containment")
        for tau, n_rec in ((0.5, 7), (0.95, 7), (0.99, 1), (1.0, 0)):
            got = run_none(sel, tau, fused)
            want, wst = case.expected(tau)
            print(f"influenza fp={fp} fused={fused} tau={tau}: {sel.stats()} values {got['jaccard'].tolist()}")
            assert len(want) == n_rec
            assert_pass(sel, got, want, wst, tau)
            if fused:
                text = pkg.format_lines(ds.names, got)
                assert pkg.select_from_filelist("influenza_filelist.txt", tau, 0, mode=MODE_SMH, fp_mode=fp, criterion="none",
                                                measure="max_containment") == text
                assert selection(["-l", "influenza_filelist.txt", "-c", "none", "-n", "-h", str(tau), "-F", flag, "-S", "max_containment"]) == text
                assert len(text.splitlines()) == n_rec
        # J selects fewer at 0.95, from the same context
        sel.set_measure("jaccard")
        assert len(run_none(sel, 0.95, fused)) == 5


def test_influenza_other_front_ends(tmp_path, monkeypatch):
    monkeypatch.chdir(GOLDEN)
    names = [l.strip() for l in (GOLDEN / "influenza_filelist.txt").read_text().splitlines() if l.strip()]
    q_names, d_names = names[::3], [x for j, x in enumerate(names) if j % 3]
    (tmp_path / "q.txt").write_text("\n".join(q_names) + "\n")
    (tmp_path / "d.txt").write_text("\n".join(d_names) + "\n")
    q, d = str(tmp_path / "q.txt"), str(tmp_path / "d.txt")
    crit = ["-c", "none", "-n", "-h", "0.95", "-S", "max_containment"]
    kw = dict(mode=MODE_SMH, criterion="none", measure="max_containment")
    union = selection(["-l", "influenza_filelist.txt"] + crit)
    assert len(union.splitlines()) == 7
    want = set()
    for line in union.splitlines():
        a, b, v = line.split(" ")
        if (a in q_names) != (b in q_names):
            want.add((a, b, v) if a in q_names else (b, a, v))
    got = selection(["-l", d, "-q", q] + crit)
    assert {tuple(l.split(" ")) for l in got.splitlines()} == want and len(got.splitlines()) == len(want) > 0
    assert pkg.query_from_filelists(q, d, 0.95, 0, **kw) == got
    best = selection(["-l", d, "-q", q, "-k", "1"] + crit)
    assert best == pkg.query_from_filelists(q, d, 0.95, 0, top_k=1, **kw) and 0 < len(best.splitlines()) <= len(q_names)
    (tmp_path / "p.txt").write_text(union)
    p = str(tmp_path / "p.txt")
    assert selection(["-l", "influenza_filelist.txt", "-p", p] + crit) == union
    strict = selection(["-l", "influenza_filelist.txt", "-p", p, "-c", "none", "-n", "-h", "0.99", "-S", "max_containment"])
    assert len(strict.splitlines()) == 1 and strict in union
    assert pkg.select_pairs_from_filelist("influenza_filelist.txt", p, 0.99, 0, **kw) == strict
    nbr = selection(["-l", "influenza_filelist.txt", "-K", "1"] + crit)
    assert nbr == pkg.select_from_filelist("influenza_filelist.txt", 0.95, 0, top_k=1, **kw) and len(nbr.splitlines()) > 0
    # smh_a and smh_c in front of the containment test: subsets of the exhaustive output, line for line
    for extra in (["-c", "smh_a", "-a", "4096"], ["-c", "smh_c", "-C", "21", "-a", "4096"]):
        out = selection(["-l", "influenza_filelist.txt", "-n", "-h", "0.95", "-S", "max_containment"] + extra)
        assert set(out.splitlines()) <= set(union.splitlines())
    # the matrix table of the CLI equals the helper's tensor
    for name in MATRIX_MEASURES:
        path = tmp_path / f"{name}.tsv"
        selection(["-l", "influenza_filelist.txt", "-M", str(path), "-S", name])
        rows, cols, vals = read_matrix(path)
        got_names, M = pkg.matrix_from_filelist("influenza_filelist.txt", measure=name)
        assert rows == cols == got_names == names and same_bits(vals, M.cpu().numpy()), name
    path = tmp_path / "qm.tsv"
    selection(["-l", d, "-q", q, "-M", str(path), "-S", "containment"])
    rows, cols, vals = read_matrix(path)
    qn, dn, M = pkg.query_matrix_from_filelists(q, d, measure="containment")
    assert rows == qn == q_names and cols == dn == d_names and same_bits(vals, M.cpu().numpy())


# ---- 2. small shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", ROUTES)
@pytest.mark.parametrize("fp", FLAVOURS)
def test_small_shapes(oracle, fp, fused):
    n_rec = 0
    with Selector(0, fp) as sel:
        sel.set_measure(MEASURE_MAX_CONTAINMENT)
        for n in (1, 2, 3, 5, 63, 64, 65, 129):
            case = spread_case(oracle, n, fp)
            sel.upload(case.hll, case.aux, case.cards)
            for tau in (0.1, 0.8, -1.0):
                got = run_none(sel, tau, fused)
                want, wst = case.expected(tau)
                assert_pass(sel, got, want, wst, (n, tau))
                n_rec += len(want)
                if n == 129 and tau == 0.1 and fp == FP_FMA:
                    assert (len(want), len(case.expected(tau, measure="jaccard")[0])) == (667, 576)
    assert n_rec > 0


# ---- 3. more than eight spans, a row count that is no multiple of 4 ------------------------------------------------------------------
@pytest.mark.parametrize("fused", ROUTES)
def test_530_genomes(oracle, fused):
    n, tau = 530, 0.3
    hll, aux, cards, _ = cm.ranked(oracle, *cm.spread_rows(n))
    rows = sorted({0, 1, 2, 3, 63, 64, 65, 255, 256, 300, 511, 512, 526, 527, 528, 529} | set(np.random.default_rng(7).integers(0, n, 8).tolist()))
    case = Case(oracle, hll, aux, cards=cards, cells=[(i, k) for i in rows for k in range(i + 1, n)])
    picked = np.zeros((n, n), dtype=bool)
    picked[rows] = True
    want = cm.select(case.V, case.E & picked, tau)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        sel.set_measure("max_containment")
        got = run_none(sel, tau, fused)
        assert sel.stats()["evaluated"] == n * (n - 1) // 2 == sel.stats()["survivors"]
        assert tuples(got[np.isin(got["i"], rows)]) == tuples(want) and len(want) > 50
        assert np.all(got["i"] < got["k"]) and len(np.unique(got["i"].astype(np.int64) * n + got["k"])) == len(got)
        # every record, whatever its row, is the matrix cell
        M = sel.matrix("max_containment").cpu().numpy()
        assert np.array_equal(M[got["i"], got["k"]].view(np.uint64), got["jaccard"].view(np.uint64))
        with np.errstate(invalid="ignore"):
            assert int((np.triu(M, 1) >= np.float64(np.float32(tau)))[case.E].sum()) == len(got)


# ---- 4. the nested set ---------------------------------------------------------------------------------------------------------------
def plant_bands(case, pairs, skip):
    """random bucket rows in which every listed pair but `skip` shares one whole band of R buckets (a band of its own on both rows:
    greedy edge colouring), and nothing else is equal"""
    rng = np.random.default_rng(99)
    aux = rng.integers(1, 1 << 62, size=(case.n, R * B), dtype=np.uint64)
    used = [set() for _ in range(case.n)]
    for i, k in pairs:
        if (i, k) == skip:
            continue
        band = min(set(range(B)) - used[i] - used[k])
        used[i].add(band); used[k].add(band)
        aux[k, band * R:(band + 1) * R] = aux[i, band * R:(band + 1) * R]
    return aux


@pytest.mark.parametrize("fp", FLAVOURS)
def test_nested_set(oracle, fp):
    hll, aux, cards, perm, members = cm.nested_set(oracle, fp)
    case = Case(oracle, hll, aux, fp, cards=cards)
    tau = 0.9
    none, nst = case.expected(tau)
    if fp == FP_FMA:
        assert (len(none), len(case.expected(tau, measure="jaccard")[0])) == (79, 55)
    # one nested pair keeps different buckets: the criterion drops it
    top, below = members[1]
    skip = (min(top, below[0]), max(top, below[0]))
    chosen = list(zip(none["i"].tolist(), none["k"].tolist()))
    assert skip in chosen
    case.aux = plant_bands(case, chosen, skip)
    S_a = smh_a_set(oracle, case)
    S_c = match_counts(case.aux, case.aux) >= R
    assert int(np.triu(S_a, 1).sum()) == len(none) - 1 == int(np.triu(S_c, 1).sum()) and not S_a[skip] and not S_c[skip]
    with Selector(0, fp) as sel:
        sel.upload(case.hll, case.aux, case.cards)
        sel.set_measure("max_containment")
        for fused in ROUTES:
            assert_pass(sel, run_none(sel, tau, fused), none, nst, ("none", fused))
        want_minus = [t for t in tuples(none) if t[:2] != skip]
        for algo in (ALGO_AUTO, ALGO_SIG, ALGO_STREAM, ALGO_HASHJOIN):
            sel.set_criterion(CRIT_SMH_A)
            got = sel.run(tau, MODE_SMH, R, B, algo=algo)
            want, wst = case.expected(tau, S_a)
            assert_pass(sel, got, want, wst, ("smh_a", algo))
            assert tuples(got) == want_minus and len(got) == len(none) - 1
        sel.set_criterion(CRIT_SMH_C)
        sel.set_min_matches(R)
        got = sel.run(tau, MODE_SMH, 7, 3)
        want, wst = case.expected(tau, S_c)
        assert_pass(sel, got, want, wst, "smh_c")
        assert tuples(got) == want_minus
        assert sel.stats()["candidates"] == wst["survivors"]
        # pairs of unequal size are among them: the CB bound would have cut these
        e = cm.trunc(case.cards)
        assert int((e[got["i"]] / e[got["k"]] < np.float64(np.float32(tau))).sum()) >= 9
        # the matrix: containment is directed, its transpose is the model's transpose, max containment equals the none records at tau = -1
        C = sel.matrix("containment").cpu().numpy()
        want_c = cm.matrix_model(case.U, case.cards, case.cards, "containment", True)
        assert_bits(C, want_c, "containment")
        assert_bits(np.ascontiguousarray(C.T), np.ascontiguousarray(want_c.T), "transpose")
        assert not np.array_equal(C.view(np.uint64), C.T.view(np.uint64))
        V = sel.matrix("max_containment").cpu().numpy()
        rec = run_none(sel, -1.0)
        assert len(rec) == int(case.E.sum())
        assert np.array_equal(V[rec["i"], rec["k"]].view(np.uint64), rec["jaccard"].view(np.uint64))
        assert np.array_equal(V.view(np.uint64), V.T.view(np.uint64)) and np.all(np.diagonal(V) == 1.0)


# ---- 5. empty sketches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp", FLAVOURS)
def test_empty_sketch(oracle, fp):
    hll, aux = cm.spread_rows(6)
    hll[2] = 0
    case = Case(oracle, hll, aux, fp)
    n = case.n
    assert case.cards[0] == 0 and case.cards[1] > 0 and not case.hll[0].any()
    with Selector(0, fp) as sel:
        sel.upload(case.hll, case.aux, case.cards)
        sel.set_measure("max_containment")
        for fused in ROUTES:
            for tau in (-1.0, -1e30, 0.5):
                got = run_none(sel, tau, fused)
                want, wst = case.expected(tau)
                assert_pass(sel, got, want, wst, (fused, tau))
                assert not np.any(got["i"] == 0) and wst["evaluated"] == n * (n - 1) // 2         # d == 0: evaluated, a survivor, never selected
        mats = {name: sel.matrix(name).cpu().numpy() for name in MATRIX_MEASURES}
    for name in MATRIX_MEASURES:
        assert_bits(mats[name], cm.matrix_model(case.U, case.cards, case.cards, name, True), name)
    for name in ("containment", "max_containment"):
        assert mats[name][0, 0] == 1.0 and np.isnan(mats[name][0, 1:]).all()
    assert not np.isnan(mats["containment"][1:, 0]).any() and np.isnan(mats["max_containment"][1:, 0]).all()
    assert not np.isnan(mats["intersection"]).any()


# ---- 6. a boundary pair ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", ROUTES)
@pytest.mark.parametrize("fp", FLAVOURS)
def test_boundary_pair(oracle, fp, fused):
    """cardinalities forged onto the threshold: V(a, b) < tau <= V(a, b + 1) for integers a <= b -- the first is dropped, the second kept"""
    hll, aux = cm.spread_rows(2)
    tau = 0.9
    tau_d = np.float64(np.float32(tau))
    U = cm.union_matrix(oracle, hll, hll, fp, symmetric=True)[0, 1]

    def v(a, b):
        return ((np.float64(a) + np.float64(b)) - U) / np.float64(min(a, b))

    a = int(U // 2)
    b = int(np.ceil(tau_d * a + U - a)) - 3
    while not v(a, b + 1) >= tau_d:
        b += 1
    assert a <= b and v(a, b) < tau_d <= v(a, b + 1)
    with Selector(0, fp) as sel:
        sel.set_measure("max_containment")
        for bb, keep in ((b, False), (b + 1, True)):
            cards = np.array([a, bb], dtype=np.float64)
            sel.upload(hll, aux, cards)
            got = run_none(sel, tau, fused)
            print(f"boundary fp={fp} fused={fused}: a={a} b={bb} V={v(a, bb)!r} tau={tau_d!r} -> {len(got)} records")
            assert stats3(sel) == {"evaluated": 1, "survivors": 1, "selected": int(keep)}
            want = [(0, 1, np.float64(v(a, bb)).view(np.uint64).item())] if keep else []
            assert tuples(got) == want


# ---- 7. row ranges, interleave parts, candidate begin, pipeline, overflow -------------------------------------------------------------
def test_partitions_pipeline_overflow(oracle):
    n, tau = 300, 0.3
    case = spread_case(oracle, n)
    want, wst = case.expected(tau)
    aux = case.aux.copy()
    aux[:, :R] = aux[0, :R]                                     # every pair shares band 0: smh_a passes everything
    assert len(want) > 100
    with Selector(0) as sel:
        sel.upload(case.hll, aux, case.cards)
        sel.set_measure("max_containment")
        for fused in ROUTES:
            parts, ev = [], 0
            for rb, re in ((0, 1), (1, 130), (130, 130), (130, 299), (299, n)):
                got = run_none(sel, tau, fused, rows=(rb, re))
                assert_pass(sel, got, *case.expected(tau, rows=(rb, re)), what=(fused, rb, re))
                parts.append(got); ev += sel.stats()["evaluated"]
            assert tuples(merged(parts)) == tuples(want) and ev == wst["evaluated"]
            parts, ev = [], 0
            for part in range(3):
                sel.set_row_interleave(32, 3, part)
                parts.append(run_none(sel, tau, fused)); ev += sel.stats()["evaluated"]
            sel.set_row_interleave(32, 1, 0)
            assert tuples(merged(parts)) == tuples(want) and ev == wst["evaluated"]
            h = 133
            sel.set_candidate_begin(h)
            got = run_none(sel, tau, fused, rows=(0, h))
            sel.set_candidate_begin(0)
            assert_pass(sel, got, *case.expected(tau, rows=(0, h), cand_begin=h), what="cand_begin")
        # two chunk lanes (an smh_a pass: criterion none has one chain)
        sel.set_criterion(CRIT_SMH_A)
        sel.set_pipeline(2)
        got = sel.run(tau, MODE_SMH, R, B, algo=ALGO_SIG)
        assert sel.get_param("chunks") == 2
        assert_pass(sel, got, want, wst, "pipeline")
        sel.set_pipeline(-1)
        sel.run_async(tau, MODE_SMH, R, B)
        with pytest.raises(SelhipError, match="pending"):
            sel.set_measure("jaccard")
        sel.finish()
        assert tuples(sel.fetch()) == tuples(want)
    # a result list that overflows and grows
    for fused in ROUTES:
        with Selector(0) as sel:
            sel.set_param("init_cap", 1024)
            sel.upload(case.hll, aux, case.cards)
            sel.set_measure("max_containment")
            got = run_none(sel, -1.0, fused)
            assert sel.last_attempts() > 1
            assert_pass(sel, got, *case.expected(-1.0), what=("overflow", fused))
            assert len(got) == n * (n - 1) // 2


# ---- 8. query passes ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def query_case(oracle, n_q, n_d):
    """(Q, D, all-pairs case over Q u D, rank -> (is query, rank in its set)): the buckets give every genome one band shared with the
    genomes of its group of five, so that smh_a passes a proper subset of the cross pairs"""
    n = n_q + n_d
    hll, _ = cm.spread_rows(n)
    rng = np.random.default_rng(n_q * 1000 + n_d)
    aux = rng.integers(1, 1 << 62, size=(n, R * B), dtype=np.uint64)
    for g in range(n):
        band = (g // 5) % B
        aux[g, band * R:(band + 1) * R] = aux[g - g % 5, band * R:(band + 1) * R]
    pick = np.zeros(n, dtype=bool)
    pick[rng.choice(n, n_q, replace=False)] = True
    Q = cm.ranked(oracle, hll[pick], aux[pick])
    D = cm.ranked(oracle, hll[~pick], aux[~pick])
    both = Case(oracle, np.concatenate([Q[0], D[0]]), np.concatenate([Q[1], D[1]]))
    return Q, D, both


def cross_records(all_pairs, perm, n_q):
    """the cross pairs of an all-pairs result over Q u D as (query rank, database rank, value), sorted by (i, k)"""
    g1, g2 = perm[all_pairs["i"]], perm[all_pairs["k"]]
    cross = (g1 < n_q) != (g2 < n_q)
    out = np.zeros(int(cross.sum()), dtype=PAIR_DTYPE)
    out["i"] = np.where(g1 < n_q, g1, g2)[cross]
    out["k"] = np.where(g1 < n_q, g2, g1)[cross] - n_q
    out["jaccard"] = all_pairs["jaccard"][cross]
    return out[np.lexsort((out["k"], out["i"]))]


@pytest.mark.parametrize("n_q", [1, 5, 7])
def test_queries_equal_cross_pairs(oracle, n_q):
    n_rec = n_dropped = 0
    tau = 0.3
    with Selector(0) as sel:
        sel.set_measure("max_containment")
        for n_d in (1, 64, 65, 200):
            Q, D, both = query_case(oracle, n_q, n_d)
            S = smh_a_set(oracle, both)
            S_c = match_counts(both.aux, both.aux) >= R
            sel.upload(D[0], D[1], D[2])
            sel.upload_queries(Q[0], Q[1], Q[2])
            want_none = cross_records(both.expected(tau)[0], both.perm, n_q)
            for fused in ROUTES:
                sel.set_criterion(CRIT_NONE)
                sel.set_param("dense_fused", fused)
                got = sel.run_queries(tau, MODE_SMH, 1, 1)
                assert tuples(got) == tuples(want_none), (n_q, n_d, fused)
                assert sel.stats()["evaluated"] == n_q * n_d and sel.stats()["selected"] == len(want_none)
            want = cross_records(both.expected(tau, S | S.T)[0], both.perm, n_q)
            sel.set_criterion(CRIT_SMH_A)
            for algo in (ALGO_SIG, ALGO_STREAM, ALGO_INDEX):
                got = sel.run_queries(tau, MODE_SMH, R, B, algo)
                assert tuples(got) == tuples(want), (n_q, n_d, algo)
                assert sel.stats()["evaluated"] == n_q * n_d and sel.stats()["selected"] == len(want)
            sel.set_criterion(CRIT_SMH_C)
            sel.set_min_matches(R)
            got = sel.run_queries(tau, MODE_SMH, 7, 3)
            assert tuples(got) == tuples(cross_records(both.expected(tau, S_c)[0], both.perm, n_q)), (n_q, n_d, "smh_c")
            n_rec += len(want)
            n_dropped += len(want_none) - len(want)
    assert n_rec > 0 and n_dropped > 0


# ---- 9. pair lists ------------------------------------------------------------------------------------------------------------------
def test_pair_lists(oracle):
    n, tau = 129, 0.3
    case = spread_case(oracle, n)
    rng = np.random.default_rng(11)
    x, y = rng.integers(0, n, size=4000), rng.integers(0, n, size=4000)
    lst = np.stack([x, y], axis=1)[x != y].astype(np.int32)
    lst = np.concatenate([lst, lst[:300], lst[300:600, ::-1]])              # entries listed twice, in both rank orders
    lo, hi = lst.min(axis=1), lst.max(axis=1)
    all_pairs, _ = case.expected(tau)
    v_of = {(i, k): v for i, k, v in tuples(all_pairs)}
    want = sorted((int(a), int(b), v_of[(int(a), int(b))]) for a, b in zip(lo, hi) if (int(a), int(b)) in v_of)
    aux = case.aux.copy()
    aux[:, :R] = aux[0, :R]                                                 # smh_a passes every pair
    with Selector(0) as sel:
        sel.upload(case.hll, aux, case.cards)
        sel.set_measure("max_containment")
        for crit, algo, r, b in ((CRIT_NONE, ALGO_AUTO, 1, 1), (CRIT_SMH_A, ALGO_SIG, R, B), (CRIT_SMH_A, ALGO_STREAM, R, B), (CRIT_SMH_C, ALGO_AUTO, 7, 3)):
            sel.set_criterion(crit)
            if crit == CRIT_SMH_C:
                sel.set_min_matches(R)
            got = sel.run_pairs(lst, tau, MODE_SMH, r, b, algo=algo)
            assert tuples(got) == want and len(want) > 100, (crit, algo)
            assert stats3(sel) == {"evaluated": len(lst), "survivors": len(lst), "selected": len(want)}
            both = sel.run_pairs(np.array([[3, 100], [100, 3]], dtype=np.int32), -1.0, MODE_SMH, r, b, algo=algo)
            assert len(both) == 2 and both["jaccard"][0].view(np.uint64) == both["jaccard"][1].view(np.uint64) == case.V[3, 100].view(np.uint64)
        for bad in ([[0, n]], [[-1, 2]], [[5, 5]]):
            with pytest.raises(SelhipError, match="invalid entries"):
                sel.run_pairs(np.array([[0, 1]] + bad, dtype=np.int32), tau, MODE_SMH, 1, 1)
        sel.run_pairs_async(lst, tau, MODE_SMH, 7, 3)
        sel.finish()
        assert tuples(sel.fetch()) == want


# ---- 10. both top-ks ----------------------------------------------------------------------------------------------------------------
def test_top_ks(oracle):
    case = spread_case(oracle, 129)
    whole, wst = case.expected(-1.0)
    with Selector(0) as sel:
        sel.upload(case.hll, case.aux, case.cards)
        sel.set_measure("max_containment")
        for k in (1, 3):
            got = run_none(sel, -1.0, top_k=k)
            assert tuples(got) == tuples(nbr_reference(whole, k)) and len(got) == 129 * k
            assert stats3(sel) == wst
        sel.set_allpairs_topk(0)
    Q, D, both = query_case(oracle, 7, 200)
    whole = cross_records(both.expected(-1.0)[0], both.perm, 7)
    assert len(whole) == 7 * 200
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        sel.set_measure("max_containment")
        sel.set_criterion(CRIT_NONE)
        for k in (1, 4):
            got = sel.run_queries(-1.0, MODE_SMH, 1, 1, top_k=k)
            assert tuples(got) == tuples(topk_reference(whole, k)) and len(got) == 7 * k
            assert sel.stats()["selected"] == len(whole)
        # ranked by V, not by J: the two orders differ somewhere
        sel.set_measure("jaccard")
        by_j = sel.run_queries(-1.0, MODE_SMH, 1, 1, top_k=4)
        assert [t[:2] for t in tuples(by_j)] != [t[:2] for t in tuples(got)]
        sel.set_query_topk(0)


# ---- 11. matrices ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp", FLAVOURS)
def test_matrix_small_shapes(oracle, fp):
    with Selector(0, fp) as sel:
        for n in (1, 2, 3, 4, 5, 63, 64, 65, 129):
            case = spread_case(oracle, n, fp)
            sel.upload(case.hll, case.aux, case.cards)
            for name in MATRIX_MEASURES:
                got = sel.matrix(name)
                assert got.shape == (n, n) and got.dtype == torch.float64
                assert_bits(got, cm.matrix_model(case.U, case.cards, case.cards, name, True), (n, name))
            # the existing measures, from the same context, as before
            assert_bits(sel.matrix("jaccard"), cm.matrix_model(case.U, case.cards, case.cards, "jaccard", True), (n, "jaccard"))
            assert_bits(sel.matrix("union"), case.U, (n, "union"))
            V = sel.matrix("max_containment").cpu().numpy()
            assert np.array_equal(V.view(np.uint64), V.T.view(np.uint64))


def test_matrix_forms(oracle):
    n = 129
    case = spread_case(oracle, n)
    SENTINEL = -12345.5
    with Selector(0) as sel:
        sel.upload(case.hll, case.aux, case.cards)
        for name in MATRIX_MEASURES:
            want = cm.matrix_model(case.U, case.cards, case.cards, name, True)
            # f32: (float) of the f64 value
            got = sel.matrix(name, dtype=torch.float32).cpu().numpy()
            w32 = want.astype(np.float32)
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), w32.view(np.uint32)), name
            # slabs
            for r0, r1 in ((0, 3), (3, 70), (70, n)):
                assert_bits(sel.matrix(name, rows=(r0, r1)), want[r0:r1], (name, r0, r1))
            # positions and ld: a permuted matrix inside a wider buffer
            perm = np.random.default_rng(3).permutation(n).astype(np.int32)
            out = torch.full((n, n + 7), SENTINEL, dtype=torch.float64, device="cuda")
            sel.matrix(name, row_pos=perm, col_pos=perm, out=out[:, :n])
            res = out.cpu().numpy()
            placed = np.empty_like(want)
            placed[np.ix_(perm, perm)] = want
            assert_bits(res[:, :n], placed, (name, "positions"))
            assert np.all(res[:, n:] == SENTINEL)
            # no mirrored stores: the upper triangle of a slab only
            sel.set_param("matrix_mirror", 0)
            out = torch.full((n, n), SENTINEL, dtype=torch.float64, device="cuda")
            sel.matrix(name, out=out)
            sel.set_param("matrix_mirror", 1)
            res = out.cpu().numpy()
            upper = np.triu(np.ones((n, n), dtype=bool))
            assert_bits(np.where(upper, res, 0.0), np.where(upper, want, 0.0), (name, "mirror 0"))
            assert np.all(res[~upper] == SENTINEL)
        # raw codes: 32-34 are accepted, 2, 15, 18, -1 and 35 are unknown
        lib = pkg.hip_lib()
        out = torch.empty((n, n), dtype=torch.float64, device="cuda")
        for code in (32, 33, 34):
            assert lib.selhip_ctx_matrix(sel._ctx, code, 0, 0, n, out.data_ptr(), n, n, n, None, None) == 0
        for code in (2, 15, 18, -1, 35):
            assert lib.selhip_ctx_matrix(sel._ctx, code, 0, 0, n, out.data_ptr(), n, n, n, None, None) == -1
            assert b"bad measure" in lib.selhip_last_error(sel._ctx)


def test_query_matrix(oracle):
    Q, D, _ = query_case(oracle, 7, 200)
    U = cm.union_matrix(oracle, Q[0], D[0])
    with Selector(0) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        for name in MATRIX_MEASURES:
            got = sel.query_matrix(name)
            assert got.shape == (7, 200)
            assert_bits(got, cm.matrix_model(U, Q[2], D[2], name, False), name)           # no diagonal in a query matrix
        # the query inside the database genome / the database genome inside the query: two different tables
        C = sel.query_matrix("containment").cpu().numpy()
        sel.upload(Q[0], Q[1], Q[2])
        sel.upload_queries(D[0], D[1], D[2])
        Ct = sel.query_matrix("containment").cpu().numpy()
        assert_bits(Ct, cm.matrix_model(U.T.copy(), D[2], Q[2], "containment", False), "swapped")
        assert not np.array_equal(C.view(np.uint64), np.ascontiguousarray(Ct.T).view(np.uint64))


def test_matrix_refusals(oracle):
    case = spread_case(oracle, 5)
    with Selector(0) as sel:
        sel.set_param("hist_algo", 0)                            # no resident bit planes
        sel.upload(case.hll, case.aux, case.cards)
        for name in MATRIX_MEASURES:
            with pytest.raises(SelhipError, match="bit planes"):
                sel.matrix(name)
    with Selector(0) as sel:
        rows = np.zeros((3, 1 << 12), dtype=np.uint8)
        sel.upload(rows, np.zeros((3, 8), dtype=np.uint64), np.array([1.0, 2.0, 3.0]), p_hll=12)
        for name in MATRIX_MEASURES:
            with pytest.raises(SelhipError, match="p_hll = 14"):
                sel.matrix(name)
        sel.matrix("smh_matches")                                # the SuperMinHash measures are untouched


# ---- 12. every refusal, and the J passes around them ----------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(oracle):
    n, tau = 65, 0.3
    case = spread_case(oracle, n)
    aux_hll = np.zeros((n, 1 << 8), dtype=np.uint8)
    lst = np.array([[0, 1], [2, 3]], dtype=np.int32)
    with Selector(0) as sel:
        sel.upload(case.hll, case.aux, case.cards)
        sel.upload_aux_hll(aux_hll, 8)
        sel.upload_queries(case.hll[:3], case.aux[:3], case.cards[:3])
        sel.upload_queries_aux_hll(aux_hll[:3], 8)

        def j_passes():
            out = []
            sel.set_criterion(CRIT_NONE)
            out.append((tuples(sel.run(tau, MODE_CB_SMH, 1, 1)), sel.stats()))
            out.append((tuples(sel.run(tau, MODE_SMH, 1, 1)), sel.stats()))
            sel.set_criterion(CRIT_SMH_A)
            out.append((tuples(sel.run(tau, MODE_CB_SMH, 4, 64)), sel.stats()))
            out.append((tuples(sel.run_queries(tau, MODE_CB_SMH, 4, 64)), sel.stats()))
            out.append((tuples(sel.run_pairs(lst, -1.0, MODE_CB_SMH, 4, 64)), sel.stats()))
            sel.set_criterion(CRIT_HLL_A)
            out.append((tuples(sel.run(tau, MODE_CB_SMH, 1, 1)), sel.stats()))
            return out

        before = j_passes()
        assert len(before[1][0]) > 0
        # the J records are the model's J
        assert before[1][0] == tuples(case.expected(tau, measure="jaccard")[0])
        for bad in (1, 2, 16, 17, 32, 33, 35, -1):
            with pytest.raises(SelhipError, match="SELHIP_MEASURE_MAX_CONTAINMENT"):
                check(sel._lib.selhip_ctx_set_measure(sel._ctx, bad), sel._ctx)
        assert j_passes() == before                              # the refused codes left the measure alone
        sel.set_measure("max_containment")
        runs = (lambda mode, r, b: sel.run(tau, mode, r, b), lambda mode, r, b: sel.run_queries(tau, mode, r, b),
                lambda mode, r, b: sel.run_pairs(lst, tau, mode, r, b))
        for crit in (CRIT_NONE, CRIT_SMH_A, CRIT_SMH_C):
            sel.set_criterion(crit)
            for run in runs:
                with pytest.raises(SelhipError, match="max_containment.*SELHIP_MODE_CB_SMH"):
                    run(MODE_CB_SMH, 4, 64)
        for crit in (CRIT_HLL_A, CRIT_HLL_AN, CRIT_HLL_A_SMH_A):
            sel.set_criterion(crit)
            for run in runs:
                for mode in (MODE_SMH, MODE_CB_SMH):
                    with pytest.raises(SelhipError, match="max_containment"):
                        run(mode, 4, 64)
        # nothing was claimed or left pending: a containment pass, then J again with the records and statistics of before
        got = run_none(sel, tau)
        assert_pass(sel, got, *case.expected(tau), what="after the refusals")
        sel.set_measure(MEASURE_JACCARD)
        assert j_passes() == before


# ---- 13. the one-launch pass of a small set ------------------------------------------------------------------------------------------
def test_small_pass_is_jaccard_only(oracle):
    n, tau = 200, 0.9
    case = spread_case(oracle, n)
    r, b = pkg.banding(256, tau)
    S = smh_a_set(oracle, case, r, b)
    with Selector(0) as sel:
        sel.set_param("small_pass", -1)                          # (the suite's default switches the one-launch pass off)
        sel.upload(case.hll, case.aux, case.cards)
        sel.set_criterion(CRIT_SMH_A)
        j_rec = sel.run(tau, MODE_SMH, r, b)
        assert sel.get_param("small_pass_used") == 1
        assert tuples(j_rec) == tuples(case.expected(tau, S, measure="jaccard")[0])
        sel.set_measure("max_containment")
        got = sel.run(tau, MODE_SMH, r, b)
        assert sel.get_param("small_pass_used") == 0
        assert_pass(sel, got, *case.expected(tau, S), what="regular pass")
        assert len(got) > len(j_rec)
        sel.set_measure("jaccard")
        assert tuples(sel.run(tau, MODE_SMH, r, b)) == tuples(j_rec)
        assert sel.get_param("small_pass_used") == 1
