"""Forged band-signature collisions through every stage-1 route that joins signatures and then verifies (tests/sig_model.py).

"A signature collision can never produce a pair" is what verify_kernel, verify16_kernel, the queue check of small_pass_kernel,
run_emit_kernel and query_verify_kernel (behind the signature join and behind the index probe) exist for; random 64-bit buckets never
show them a collision.  Here every pass meets pairs whose band signatures are equal and whose contents are not -- alone, before and
after a truly equal band, in every band at once, on the edge values of the signature, in a crowd of 70 -- and must return the oracle's
pairs and J bits, the oracle's survivor count and the MODEL's candidate count: the pairs inside the pass's windows with at least one
equal band signature, each once.  The sketches' HLL registers and cardinalities come from the generator, the buckets from planted_set."""
import numpy as np
import pytest

import sig_model as S
from test_gpu_parity import assert_same_pairs, sorted_set
from test_query_gpu import assert_same, union_reference

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import (ALGO_AUTO, ALGO_HASHJOIN, ALGO_INDEX, ALGO_SIG, ALGO_STREAM, FP_FMA, MODE_CB_SMH, MODE_SMH, Selector,
                                         SynthConfig)

pytestmark = pytest.mark.gpu

N = 200                                          # 256 columns in the band-major signature layouts: the padding lanes are live
N_STALE = 130
ROWS = (64, 137)
RUNS = {"smh": (0.0, MODE_SMH, False), "cb": (0.5, MODE_CB_SMH, True)}
FORBIDDEN = ("C1", "C4", "C5", "C6", "C7", "C8")
SHAPE_IDS = [f"{r}x{nb}" for _, r, nb in S.SHAPES]
_CACHE = {}


class Case:
    """one band shape: the planted set, its signatures under the model, and what every pass over it must report"""

    def __init__(self, oracle, m, r, nb):
        if "base" not in _CACHE:
            # spread cardinalities, so that the CB windows of the tau = 0.5 passes cut the pair space
            cfg = SynthConfig("sig-collisions", N, 128, 0.9, 0x5EED0C01, mode=1, n_sh_lo=3000, n_sh_hi=40000)
            hll, _, cards, _, _ = sorted_set(cfg, oracle)
            # rank pairs whose HLL-Jaccard estimate is >= 0, i.e. listed at tau = 0 once they survive stage 1 (the inclusion-exclusion
            # estimate of nearly disjoint sets can fall below 0): the oracle over sketches equal in their one band
            allp, _ = oracle.select(hll, np.zeros((N, 8), dtype=np.uint64), cards, 0.0, 8, 1, use_cb=False)
            good = np.zeros((N, N), dtype=bool)
            good[allp["i"], allp["k"]] = True
            _CACHE["base"] = (hll, cards, good)
        self.hll, self.cards, good = _CACHE["base"]
        self.oracle, self.m, self.r, self.nb = oracle, m, r, nb
        n_d = N - len(range(0, N, 3))
        self.P = S.planted_set(N, m, r, nb, seed=0x51C0 + r, dir_bits=S.index_dir_bits(n_d), good=good, stale_cut=N_STALE)
        self.aux = self.P.aux
        self.sg = S.band_sigs(self.aux, r, nb)
        self.lit = S.literal_matrix(self.aux, self.aux, r, nb)
        self._exp = {}

    def expect(self, run, n=N, rows=None):
        """(oracle's pairs, oracle's evaluated or None, survivors, candidates) of a pass over the first n genomes, rows = (begin, end)"""
        key = (run, n, rows)
        if key not in self._exp:
            tau, _, use_cb = RUNS[run]
            want, st = self.oracle.select(self.hll[:n], self.aux[:n], self.cards[:n], tau, self.r, self.nb, use_cb=use_cb)
            lo, hi = S.allpairs_windows(self.cards[:n], tau, use_cb)
            # the model's windows and literal predicate against the oracle's own counts
            assert int(S.window_mask(lo, hi, n).sum()) == st["evaluated"]
            assert int((self.lit[:n, :n] & S.window_mask(lo, hi, n)).sum()) == st["survivors"]
            if rows is not None:
                want = want[(want["i"] >= rows[0]) & (want["i"] < rows[1])]
            self._exp[key] = (want, None if rows is not None else st["evaluated"], int((self.lit[:n, :n] & S.window_mask(lo, hi, n, rows)).sum()),
                              S.expected_candidates(self.sg[:n], lo, hi, rows))
        return self._exp[key]


def case(oracle, m, r, nb):
    if (m, r, nb) not in _CACHE:
        _CACHE[(m, r, nb)] = Case(oracle, m, r, nb)
    return _CACHE[(m, r, nb)]


def check_pass(sel, c, algo, run, n=N, rows=None, candidates=True):
    tau, mode, _ = RUNS[run]
    want, evaluated, survivors, cand = c.expect(run, n, rows)
    got = sel.run(tau, mode, c.r, c.nb, rows=rows, algo=algo)
    st = sel.stats()
    print(f"{c.r}x{c.nb} {run} n={n} rows={rows}: listed {len(got)} / {len(want)}, survivors {st['survivors']} / {survivors}, "
          f"candidates {st['candidates']} / {cand}, attempts {sel.last_attempts()}")
    assert_same_pairs(got, want)
    assert st["survivors"] == survivors
    if evaluated is not None:
        assert st["evaluated"] == evaluated
    if candidates:
        assert st["candidates"] == cand
    listed = set(zip(got["i"].tolist(), got["k"].tolist()))
    assert len(listed) == len(got)                                            # no pair twice
    assert not listed & set(c.P.of(*FORBIDDEN))
    if run == "smh":
        inside = lambda p: p[1] < n and (rows is None or rows[0] <= p[0] < rows[1])      # noqa: E731
        assert {p for p in c.P.of("C2", "C3") if inside(p)} <= listed
    return got


# ---- all-pairs passes ------------------------------------------------------------------------------------------------------------
SIG16 = {f"sig16-form{f}-q{q}-db{d}": (ALGO_SIG, {"join_bits": 16, "join_form": f, "join_q": q, "join_db": d})
         for f in (0, 1) for q in (0, 1) for d in (0, 1)}
ROUTES = {
    "sig32": (ALGO_SIG, {"join_bits": 32}),                                   # sig_join_kernel -> verify_kernel
    **SIG16,                                                                  # sig16_join_kernel / sigl_join_kernel -> verify16_kernel
    "sig16-sliced": (ALGO_SIG, {"join_bits": 16, "join_form": 2}),            # (the bit-sliced form where the tiled build writes it)
    "sig15": (ALGO_SIG, {"join_bits": 15}),
    "sig15-q0": (ALGO_SIG, {"join_bits": 15, "join_q": 0}),
    "sig32-tile0": (ALGO_SIG, {"join_bits": 32, "sig_tile": 0}),              # the per-bucket build against the tiled build
    "sig16-tile0": (ALGO_SIG, {"join_bits": 16, "sig_tile": 0}),
    "sig16-tile1": (ALGO_SIG, {"join_bits": 16, "sig_tile": 1}),
    "hashjoin": (ALGO_HASHJOIN, {}),                                          # run_emit_kernel
    "auto-small1": (ALGO_AUTO, {"small_pass": 1}),                            # small_pass_kernel where it takes the shape
    "auto-small0": (ALGO_AUTO, {"small_pass": 0}),
    "stream": (ALGO_STREAM, {}),                                              # the control: reads no signatures
    "sig16-fb": (ALGO_SIG, {"verify_fb": 1}),                                 # every candidate through the literal fallback
    "sig15-fb": (ALGO_SIG, {"join_bits": 15, "verify_fb": 1}),
    "auto-small1-fb": (ALGO_AUTO, {"small_pass": 1, "verify_fb": 1}),
}


def small_pass_takes(r):
    return 2 <= r <= 32                                                       # the tiled build's rows (8 .. 128 bands: every shape here)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("m,r,nb", S.SHAPES, ids=SHAPE_IDS)
def test_allpairs_routes(oracle, m, r, nb, route):
    c = case(oracle, m, r, nb)
    algo, params = ROUTES[route]
    with Selector(0) as sel:
        for name, value in params.items():
            sel.set_param(name, value)
        sel.upload(c.hll, c.aux, c.cards)
        for run in RUNS:
            check_pass(sel, c, algo, run, candidates=algo != ALGO_STREAM)
            if "small_pass" in params:
                assert sel.get_param("small_pass_used") == (1 if params["small_pass"] and small_pass_takes(r) else 0)


@pytest.mark.parametrize("route", ["sig32", "sig16-sliced", "sig16-form0-q0-db1", "sig15", "hashjoin"])
@pytest.mark.parametrize("m,r,nb", S.SHAPES, ids=SHAPE_IDS)
def test_allpairs_list_overflow(oracle, m, r, nb, route):
    """"init_cap" at its smallest: the lists overflow on the crowd's pure collisions, grow and the pass repeats; the counts stay exact"""
    c = case(oracle, m, r, nb)
    algo, params = ROUTES[route]
    with Selector(0) as sel:
        sel.set_param("init_cap", 1)
        for name, value in params.items():
            sel.set_param(name, value)
        sel.upload(c.hll, c.aux, c.cards)
        check_pass(sel, c, algo, "smh")
        assert sel.last_attempts() >= 2
        check_pass(sel, c, algo, "cb")


STALE_ROUTES = ["sig32", "sig16-sliced", "sig16-form0-q0-db1", "sig16-form0-q1-db0", "sig15", "sig16-tile0", "hashjoin", "auto-small1"]


@pytest.mark.parametrize("m,r,nb", S.SHAPES, ids=SHAPE_IDS)
def test_allpairs_stale_columns_and_row_range(oracle, m, r, nb):
    """one context per route: all 200 genomes, a row sub-range of them, then only the first 130 -- the columns 130 .. 199 of the
    band-major layouts still hold the signatures of the first upload (one of the zero-signature triple among them)"""
    c = case(oracle, m, r, nb)
    zero = c.P.triples[0][2]
    assert c.P.triples[0][0] == 0 and sum(g < N_STALE for g in zero) == 2
    for route in STALE_ROUTES + ["stream"]:
        algo, params = ROUTES[route]
        with Selector(0) as sel:
            for name, value in params.items():
                sel.set_param(name, value)
            sel.upload(c.hll, c.aux, c.cards)
            for run in RUNS:
                check_pass(sel, c, algo, run, candidates=algo != ALGO_STREAM)
                check_pass(sel, c, algo, run, rows=ROWS, candidates=algo != ALGO_STREAM)
            sel.upload(c.hll[:N_STALE], c.aux[:N_STALE], c.cards[:N_STALE])
            for run in RUNS:
                got = check_pass(sel, c, algo, run, n=N_STALE, candidates=algo != ALGO_STREAM)
                assert len(got) == 0 or got["k"].max() < N_STALE


# ---- query passes ----------------------------------------------------------------------------------------------------------------
class QueryCase:
    """the planted set of a shape split into queries and database, each side in its own rank order"""

    def __init__(self, c, pick):
        self.c = c
        ids = np.arange(N)
        sides = []
        for mask in (pick, ~pick):
            cards = c.oracle.cards(c.hll[mask])
            perm = pkg.sort_by_card(cards)
            sides.append(((c.hll[mask][perm], c.aux[mask][perm], cards[perm]), ids[mask][perm]))
        (self.Q, self.q_ids), (self.D, self.d_ids) = sides
        self.sig_q, self.sig_d = S.band_sigs(self.Q[1], c.r, c.nb), S.band_sigs(self.D[1], c.r, c.nb)
        q_rank = {int(g): t for t, g in enumerate(self.q_ids)}
        d_rank = {int(g): t for t, g in enumerate(self.d_ids)}

        def cross(*classes):
            out = set()
            for i, k in c.P.of(*classes):
                if i in q_rank and k in d_rank:
                    out.add((q_rank[i], d_rank[k]))
                if k in q_rank and i in d_rank:
                    out.add((q_rank[k], d_rank[i]))
            return out
        self.cross = cross
        self._exp = {}

    def expect(self, run):
        if run not in self._exp:
            tau, _, use_cb = RUNS[run]
            c = self.c
            want, wst = union_reference(c.oracle, self.Q, self.D, tau, c.r, c.nb, use_cb, FP_FMA)
            lo, hi = S.query_windows(self.Q[2], self.D[2], tau, use_cb)
            mask = S.window_mask(lo, hi, len(self.d_ids))
            assert int(mask.sum()) == wst["evaluated"]
            assert int((S.literal_matrix(self.Q[1], self.D[1], c.r, c.nb) & mask).sum()) == wst["survivors"]
            self._exp[run] = (want, wst, S.expected_candidates_qd(self.sig_q, self.sig_d, lo, hi))
        return self._exp[run]


def query_case(oracle, m, r, nb, split):
    key = (m, r, nb, split)
    if key not in _CACHE:
        c = case(oracle, m, r, nb)
        pick = np.zeros(N, dtype=bool)
        if split == "third":
            pick[::3] = True
        else:
            # five queries: fewer than a tile of the signature join, whose empty slots hold signature 0 in every band -- as two
            # database genomes do in one band (and the third zero-signature genome is a query)
            P = c.P
            zero = [g for g in P.triples[0][2] if g % 3 == 0]
            c2 = [p for p in P.of("C2") if (p[0] % 3 == 0) != (p[1] % 3 == 0)][0]
            pick[[zero[0], c2[0] if c2[0] % 3 == 0 else c2[1], 0, 15, [g for g in P.crowd_equal if g % 3 == 0][0]]] = True
            assert pick.sum() == 5
        _CACHE[key] = QueryCase(c, pick)
    return _CACHE[key]


QUERY_ROUTES = {
    "sig": (ALGO_SIG, {}),                                                    # query_sig_join_kernel -> query_verify_kernel
    "sig-tile32": (ALGO_SIG, {"query_join_tile": 32}),
    "sig-buildtile0": (ALGO_SIG, {"sig_tile": 0}),
    "index": (ALGO_INDEX, {"query_index_dir": 1}),                            # query_index_probe_kernel (query_index_take) -> query_verify_kernel
    "index-nodir": (ALGO_INDEX, {"query_index_dir": 0}),
    "stream": (ALGO_STREAM, {}),                                              # the control
}


@pytest.mark.parametrize("route", list(QUERY_ROUTES))
@pytest.mark.parametrize("split", ["third", "five"])
@pytest.mark.parametrize("m,r,nb", S.SHAPES, ids=SHAPE_IDS)
def test_query_routes(oracle, m, r, nb, split, route):
    qc = query_case(oracle, m, r, nb, split)
    c = qc.c
    algo, params = QUERY_ROUTES[route]
    # the split separates pairs of every class; the crowd stays in the database but for three members (one, among five queries)
    for cls in ("C1", "C2", "C3", "C4", "C5", "C6", "C7", "C8", "C8="):
        assert qc.cross(cls) or split == "five", cls
    assert len(qc.cross("C8", "C8=")) == (3 * (S.CROWD - 3) if split == "third" else S.CROWD - 1) and len(qc.cross("C8=")) == 1
    with Selector(0) as sel:
        for name, value in params.items():
            sel.set_param(name, value)
        sel.upload(qc.D[0], qc.D[1], qc.D[2])
        sel.upload_queries(qc.Q[0], qc.Q[1], qc.Q[2])
        for run in RUNS:
            tau, mode, _ = RUNS[run]
            want, wst, cand = qc.expect(run)
            got = sel.run_queries(tau, mode, c.r, c.nb, algo=algo)
            st = sel.stats()
            print(f"{c.r}x{c.nb} {split} {run}: listed {len(got)} / {len(want)}, survivors {st['survivors']} / {wst['survivors']}, "
                  f"candidates {st['candidates']} / {cand}")
            assert_same(got, want)
            assert st["evaluated"] == wst["evaluated"] and st["survivors"] == wst["survivors"] and st["selected"] == len(want)
            if algo != ALGO_STREAM:
                assert st["candidates"] == cand
            listed = set(zip(got["i"].tolist(), got["k"].tolist()))
            assert len(listed) == len(got)
            assert not listed & qc.cross(*FORBIDDEN)
            if run == "smh":
                assert qc.cross("C2", "C3") <= listed

