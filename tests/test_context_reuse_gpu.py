"""One live context, one database after another, of other shapes (include/selection_hip.h, selhip_ctx_upload: what a replacement resets,
what it keeps, what a refused one leaves).  The sets, the operations and their expected values are
tests/context_reuse_model.py's, whose premises tests/test_context_reuse_host.py pins: every step changes every answer, and the bytes a
larger set leaves in the grow-only buffers are true partners of the smaller set's rows.

Every comparison is bit for bit (stream_harness.same): records, statistics, matrices, labels, merged rows.  Expected values come from
the oracle and the models, never from a second context.

  test_transition   every operation on X (warm-up: every buffer sized, every cached product X's), the database replaced by Y with Y's
                    queries and auxiliary sketches, every operation on Y against expected(Y, op)
  test_walk         60 random steps from a seed: replace the database (upload / attach), replace the queries, flip a route knob that
                    changes no answer, run an operation; the log goes into the assertion message
  test_refused_upload_leaves_the_context_alone, test_settings_survive_a_replacement   the contract of the header"""
import ctypes as C

import numpy as np
import pytest
import torch

import context_reuse_model as R
import stream_harness as H

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import (ALGO_AUTO, ALGO_HASHJOIN, ALGO_INDEX, ALGO_SIG, ALGO_STREAM, CRIT_HLL_A, CRIT_HLL_A_SMH_A,
                                         CRIT_NONE, CRIT_SMH_A, CRIT_SMH_C, MODE_CB_SMH, PAIR_DTYPE, Selector, SelhipError)
from cuda_selection_criteria_amd._lib import Linkage
from cuda_selection_criteria_amd._lib import check as lib_check

pytestmark = pytest.mark.gpu

K = R.K
Q_CUT = 25                                    # the second query set of a set: the first Q_CUT of its queries (a prefix in rank order)
POISON = -7.0
# what every context of these tests starts from (the suite's own defaults, tests/conftest.py, said aloud) unless a flavour says otherwise
BASE_KNOBS = {"sig_cache": 1, "small_pass": 0, "group_min_n": 0}


@pytest.fixture(scope="module")
def lib(oracle):
    return R.Library(oracle)


def dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


class Live:
    """a context that lives through the test, the set it holds and how it was handed over"""

    def __init__(self, lib, knobs=None, inplace_rows=0):
        self.lib, self.knobs = lib, dict(BASE_KNOBS, **(knobs or {}))
        self.sel = Selector(0)
        for name, value in self.knobs.items():
            if name == "pipeline":
                self.sel.set_pipeline(value)
            else:
                self.sel.set_param(name, value)
        self.S, self.q_rows, self.log = None, None, []
        # attach into the SAME tensors, rewritten in place (inplace_rows rows of BIG's shape): views of their first n rows are attached
        self.buf = None
        if inplace_rows:
            B = lib["BIG"]
            self.buf = {"hll": torch.zeros((inplace_rows, 1 << 14), dtype=torch.uint8, device="cuda"),
                        "aux": torch.zeros((inplace_rows, B.m), dtype=torch.int64, device="cuda"),
                        "cards": torch.zeros(inplace_rows, dtype=torch.float64, device="cuda")}
        self.held = {}

    def close(self):
        torch.cuda.synchronize()
        self.sel.close()

    def knob(self, name, value):
        self.knobs[name] = value
        if name == "pipeline":
            self.sel.set_pipeline(value)
        else:
            self.sel.set_param(name, value)

    # -- replacements -------------------------------------------------------------------------------------------------------------
    def replace(self, name, how="upload", device_cards=False, queries=True):
        """the database of set `name` through upload or attach, then its queries (the same way)"""
        S, sel = self.lib[name], self.sel
        self.log.append(("db", name, how))
        D = S.D
        if how == "upload":
            sel.upload(D.hll, D.aux, None if device_cards else D.cards, p_hll=S.p_hll)
        else:
            if self.buf is not None and S.p_hll == 14 and S.m == self.buf["aux"].shape[1] and S.n_d <= self.buf["aux"].shape[0]:
                t = {k: v[:S.n_d] for k, v in self.buf.items()}
                t["hll"].copy_(dev(D.hll)), t["aux"].copy_(dev(D.aux)), t["cards"].copy_(dev(D.cards))
                torch.cuda.synchronize()
            else:
                t = {"hll": dev(D.hll), "aux": dev(D.aux), "cards": dev(D.cards)}
            self.held["db"] = t
            sel.attach(t["hll"], t["aux"], None if device_cards else t["cards"], p_hll=S.p_hll)       # (EMPTY: null pointers, n = 0)
        self.S, self.q_rows = S, None
        if queries:
            self.queries(S.n_q, how)

    def queries(self, rows, how="upload"):
        """the first `rows` queries of the set; a set at p_hll != 14 must refuse them"""
        S, sel, Q = self.S, self.sel, self.S.Q
        self.log.append(("queries", S.name, rows, how))
        if S.p_hll != 14:
            with pytest.raises(SelhipError) as e:
                sel.upload_queries(Q.hll, Q.aux, Q.cards)
            assert e.value.code == R.BADARG
            self.q_rows = None
            return
        if how == "upload":
            sel.upload_queries(Q.hll[:rows], Q.aux[:rows], Q.cards[:rows])
        else:
            t = {"hll": dev(Q.hll[:rows]), "aux": dev(Q.aux[:rows]), "cards": dev(Q.cards[:rows])}
            self.held["q"] = t
            sel.attach_queries(t["hll"], t["aux"], t["cards"])
        self.q_rows = rows

    # -- settings -----------------------------------------------------------------------------------------------------------------
    def settle(self, criterion=CRIT_SMH_A, estimator="hll", topk=0, rounds=0):
        """every answer-changing setting, set by every operation for itself and left for whoever comes next"""
        sel = self.sel
        sel.set_criterion(criterion)
        sel.set_measure("jaccard")
        sel.set_estimator(estimator)
        sel.set_allpairs_topk(topk)
        sel.set_query_topk(0)
        sel.set_topk_rounds(rounds)
        sel.set_min_matches(self.S.c_min)
        sel.set_min_containment(None)
        sel.set_candidate_begin(0)
        sel.set_row_interleave(128, 1, 0)

    def run(self, algo=ALGO_AUTO, **kw):
        S = self.S
        return self.sel.run(S.tau, MODE_CB_SMH, S.r, S.b, algo=algo, **kw)

    def small_expected(self):
        """whether an smh_a signature pass of the set takes the one-launch small pass (host_pass.hpp, small_pass_ok), None = not pinned"""
        S = self.S
        if self.knobs["small_pass"] == 0 or self.knobs.get("hist_algo") == 0 or S.p_hll != 14 or S.n_d < 2 or S.planes > 5:
            return 0
        return 1 if S.m == 128 else None

    def aux(self, how):
        S, sel = self.S, self.sel
        if how == "fold":
            sel.fold_aux_hll(S.p_aux)
        elif S.n_d and how == "upload":
            sel.upload_aux_hll(S.D.aux_hll, S.p_aux)
        elif S.n_d:
            self.held["aux_hll"] = dev(S.D.aux_hll)
            sel.attach_aux_hll(self.held["aux_hll"], S.p_aux)


# ---- the operations: op(live) -> the value on the host ---------------------------------------------------------------------------------
RUN = {}


def op(*names):
    def register(fn):
        for name in names:
            assert name in R.OPS and name not in RUN, name
            RUN[name] = (lambda f, n: lambda live: f(live, n))(fn, name)
        return fn
    return register


@op("smh_a-sig", "smh_a-stream", "smh_a-hashjoin", "smh_a-small_pass", "smh_a-chunks2")
def _smh_a(live, name):
    sel, S = live.sel, live.S
    live.settle()
    algo = {"smh_a-stream": ALGO_STREAM, "smh_a-hashjoin": ALGO_HASHJOIN, "smh_a-small_pass": ALGO_AUTO}.get(name, ALGO_SIG)
    if name == "smh_a-small_pass":
        sel.set_param("small_pass", 1)
    if name == "smh_a-chunks2":
        sel.set_pipeline(2)
    try:
        got = live.run(algo)
        used = sel.get_param("small_pass_used")
        if name == "smh_a-small_pass" and S.p_hll == 14 and S.m == 128 and S.n_d >= 2:
            assert used == (1 if S.planes <= 5 and live.knobs.get("hist_algo") != 0 else 0), "small_pass_used"
        if name in ("smh_a-sig", "smh_a-chunks2") and S.n_d >= 2:
            want = live.small_expected()
            assert want is None or used == want, f"small_pass_used {used}, the set and the knobs say {want}"
            if not used and S.m == 128:
                assert sel.get_param("join_form_used") == {2: 3, 1: 2, 0: 0}[live.knobs.get("join_form", 2)], "the join of the knob did not run"
            if name == "smh_a-chunks2":
                assert sel.get_param("chunks") == (1 if used else 2)
    finally:
        sel.set_param("small_pass", live.knobs["small_pass"])
        sel.set_pipeline(live.knobs.get("pipeline", -1))
    # which rows stage 2a read: the clamped four-plane image wherever the set holds one and the knobs allow it (the one-launch small pass
    # has its own stage 2 and reports 0)
    image = sel.get_param("hist_image")
    image_want = 0 if sel.get_param("small_pass_used") else S.hist_image(live.knobs)
    assert image == image_want, f"{name} on {S.name}: get_param('hist_image') {image}, the set (threshold {S.sparse_t}) and the knobs say {image_want}"
    if name == "smh_a-sig":
        # a pad column that is joined and filtered later shows in the statistics alone
        st = sel.stats()
        want = R.stats_expected(S)
        assert (st["evaluated"], st["survivors"], st["selected"]) == (want["evaluated"], want["survivors"], want["selected"]), (st, want)
        if not sel.get_param("small_pass_used"):
            assert st["candidates"] == want["candidates"], (st, want)
    return got


@op("hll_a-uploaded", "hll_a-folded", "hll_a+smh_a")
def _aux(live, name):
    live.settle(CRIT_HLL_A_SMH_A if name == "hll_a+smh_a" else CRIT_HLL_A)
    live.aux({"hll_a-uploaded": "upload", "hll_a-folded": "fold", "hll_a+smh_a": "attach"}[name])
    return live.run()


@op("none-list_route", "none-fused")
def _none(live, name):
    sel = live.sel
    live.settle(CRIT_NONE)
    fused = int(name == "none-fused")
    sel.set_param("dense_fused", fused)
    got = live.run()
    if live.S.n_d >= 2:
        assert sel.get_param("dense_route_used") == fused
    return got


@op("smh_c", "smh_c-smh_estimator")
def _smh_c(live, name):
    live.settle(CRIT_SMH_C, estimator="smh" if name == "smh_c-smh_estimator" else "hll")
    return live.run()


def unframe(rec):
    cnt = int(rec[0, 0])
    return H.by_ik(rec[1:1 + cnt].reshape(-1).view(PAIR_DTYPE))


@op("run_async-framed-finish")
def _async(live, name):
    sel, S = live.sel, live.S
    live.settle()
    frame = torch.zeros((2048 + 1, 2), dtype=torch.int64, device="cuda")
    sel.run_async(S.tau, MODE_CB_SMH, S.r, S.b, algo=ALGO_SIG)
    if S.n_d >= 2:
        sel.copy_results_framed_async(frame)
    sel.finish()
    assert sel.result_count() <= 2048
    if S.n_d < 2:
        return sel.fetch()
    got = unframe(frame.cpu().numpy())
    assert H.same(sel.fetch(), got)
    return got


@op("query-sig", "query-stream", "query-index", "query-topk")
def _query(live, name):
    sel, S = live.sel, live.S
    live.settle()
    algo = {"query-stream": ALGO_STREAM, "query-index": ALGO_INDEX}.get(name, ALGO_SIG)
    got = sel.run_queries(S.tau, MODE_CB_SMH, S.r, S.b, algo=algo, top_k=K if name == "query-topk" else 0)
    if name == "query-index" and S.n_d and live.q_rows:
        assert sel.get_param("query_db_index_builds") == 1, "the index is built once per database"
    return got


@op("allpairs-topk")
def _topk(live, name):
    live.settle(topk=K)
    return live.run(ALGO_SIG, top_k=K)


@op("allpairs-topk-rounds")
def _topk_rounds(live, name):
    live.settle(CRIT_SMH_C, estimator="smh", topk=K, rounds=H.ROUND_ROWS)
    got = live.run(top_k=K, rounds=H.ROUND_ROWS)
    if live.S.n_d:
        assert live.sel.get_param("topk_rounds_used") == -(-live.S.n_d // H.ROUND_ROWS)
    return got


@op("pairs-signature_route", "pairs-direct_route")
def _pairs(live, name):
    sel, S = live.sel, live.S
    live.settle()
    route = int(name == "pairs-signature_route")
    got = sel.run_pairs(S.pair_list, S.tau, MODE_CB_SMH, S.r, S.b, algo=ALGO_SIG if route else ALGO_STREAM)
    if len(S.pair_list):
        assert sel.get_param("pairs_route_used") == route
    return got


@op("matrix-jaccard", "matrix-smh_matches")
def _matrix(live, name):
    out = torch.full((live.S.n_d, live.S.n_d), POISON, dtype=torch.float64, device="cuda")
    live.sel.matrix(name.split("-")[1], out=out)
    return out.cpu().numpy()


@op("query_matrix-containment")
def _query_matrix(live, name):
    S = live.S
    out = torch.full((S.n_q, S.n_d), POISON, dtype=torch.float64, device="cuda")
    live.sel.query_matrix("containment", row_pos=S.row_pos[:live.q_rows], col_pos=S.col_pos, out=out)
    return out.cpu().numpy()


@op("cluster", "cluster_greedy-priority")
def _cluster(live, name):
    sel, S = live.sel, live.S
    live.settle()
    live.run(ALGO_SIG, fetch=False)
    if name == "cluster":
        return sel.cluster(rep="max_degree")
    res = sel.cluster_greedy(order="priority", priority=S.prio)
    res.pop("rounds")
    return res


@op("forest")
def _forest(live, name):
    """the smh_a signature pass, then its maximum spanning forest: GraphScratch, which cluster and cluster_greedy size too"""
    live.settle()
    live.run(ALGO_SIG, fetch=False)
    res = live.sel.spanning_forest()
    assert res["n_edges"] == len(res["edges"]) == live.sel.get_param("forest_edges_last")
    return {"edges": res["edges"], "labels": res["labels"]}


def kept_of_the_last_pass(sel):
    """the result list, its count and the statistics as the context gives them now, or the refusal where it holds no finished pass"""
    try:
        return sel.result_count(), sel.fetch().tobytes(), sel.stats()
    except SelhipError as e:
        return "refused", e.code


@op(*R.LINKAGE_OPS)
def _linkage(live, name):
    """selhip_ctx_linkage into poisoned arrays: the merges, the sizes and the rounds; "linkage_merges_last" and "linkage_rounds_last" are
    the model's, and the result list, stats() and result_count() are what they were before the call"""
    sel, S = live.sel, live.S
    measure, method, capped = H.LINKAGE_CASES[name]
    want = R.expected(S, name, live.knobs.get("hist_algo") != 0)
    cap = float("inf") if not capped else 0.5 if isinstance(want, int) or S.trivial else S.linkage_cap      # (0.5: a call that is refused)
    room = max(S.n_d - 1, 0)
    merges = torch.full((room, PAIR_DTYPE.itemsize), 0xA5, dtype=torch.uint8, device="cuda")
    sizes = torch.full((room,), int(POISON), dtype=torch.int32, device="cuda")
    before = kept_of_the_last_pass(sel)
    out, cnt = Linkage(merges.data_ptr() if room else None, sizes.data_ptr() if room else None), C.c_int64(-5)
    lib_check(sel._lib.selhip_ctx_linkage(sel._ctx, pkg.measure_code(measure), pkg.linkage_code(method), cap, C.byref(out), C.byref(cnt)), sel._ctx)
    f = cnt.value
    m, s = merges.cpu().numpy(), sizes.cpu().numpy()
    assert 0 <= f <= room and np.all(m[f:] == 0xA5) and np.all(s[f:] == int(POISON)), f"{name} on {S.name}: the entries from F = {f} on were written"
    got = {"merges": np.ascontiguousarray(m[:f]).reshape(-1).view(PAIR_DTYPE), "sizes": s[:f], "rounds": sel.get_param("linkage_rounds_last")}
    assert (sel.get_param("linkage_merges_last"), got["rounds"]) == (len(want["merges"]), want["rounds"]), \
        f"{name} on {S.name}: merges and rounds {sel.get_param('linkage_merges_last'), got['rounds']}, the model's {len(want['merges']), want['rounds']}"
    assert kept_of_the_last_pass(sel) == before, f"{name} on {S.name}: the call changed the result list, its count or the statistics"
    return got


@op("merge_groups")
def _merge(live, name):
    S = live.S
    live.aux("upload")
    res = live.sel.merge(S.groups, R.N_GROUPS, to_host=True)
    if S.n_d == 0:                                             # (no auxiliary sketches can be handed to an empty set: whatever an
        res.pop("aux_hll")                                     #  earlier fold left is merged into rows of zeros, or nothing is)
    return res


@op("cards")
def _cards(live, name):
    return live.sel.cards()


def test_every_operation_has_a_body():
    assert set(RUN) == set(R.OPS)


def want_of(live, name):
    """expected(S, op) for the queries the context holds"""
    S, want = live.S, R.expected(live.S, name, live.knobs.get("hist_algo") != 0)
    if name == "merge_groups" and S.n_d == 0:                     # (whatever queries the context holds: _merge drops the rows there)
        want = {k: v for k, v in want.items() if k != "aux_hll"}
    if isinstance(want, int) or live.q_rows is None or live.q_rows == S.n_q:
        return want
    if R.OPS[name][1] == "qlist":
        return want[want["i"] < live.q_rows]
    if name == "query_matrix-containment":
        want = want.copy()
        want[S.row_pos[live.q_rows:]] = POISON
    return want


def check(live, name):
    """run one operation on the set the context holds and compare it with the expected value, or with the refusal code"""
    live.log.append(("op", live.S.name, name))
    want = want_of(live, name)
    if isinstance(want, int):
        with pytest.raises(SelhipError) as e:
            if name in R.QUERY_OPS and live.S.p_hll != 14:
                live.sel.upload_queries(live.S.Q.hll, live.S.Q.aux, live.S.Q.cards)
            else:
                RUN[name](live)
        assert e.value.code == want, f"{name} on {live.S.name}: refused with {e.value.code}, documented {want}\n{live.log[-12:]}"
        return
    got = RUN[name](live)
    assert H.same(got, want), f"{name} on {live.S.name}: {H.describe(got, want)}\nlast steps: {live.log[-12:]}"


# ---- (a) transitions -----------------------------------------------------------------------------------------------------------------
# flavour -> (how the first set is handed over, how the next ones are, knobs, extras)
FLAVOURS = {
    "upload-upload": ("upload", "upload", {}, {}),
    "upload-attach": ("upload", "attach", {}, {}),
    "attach-upload": ("attach", "upload", {}, {}),
    "attach-inplace": ("attach", "attach", {}, {"inplace": True}),
    "sig_cache0-device_cards": ("upload", "upload", {"sig_cache": 0}, {"device_cards": True}),
    "hist_algo0": ("upload", "upload", {"hist_algo": 0}, {}),
    "small_pass_auto": ("upload", "upload", {"small_pass": -1}, {}),
    "init_cap128": ("upload", "upload", {"init_cap": 128}, {}),
}
CASES = [(t, f) for t in R.TRANSITIONS[:2] for f in FLAVOURS] + [(t, "upload-upload") for t in R.TRANSITIONS[2:]]
# (two sets of one shape without bit planes: the query side's own planes of the database are the only product that tells them apart)
CASES.append((("HIGHREG", "BIG"), "hist_algo0"))
# the warm-up runs everything, as the checked half does: every buffer is sized, every cached product is X's.  Under "init_cap" the lists
# start at 128 entries and the warm-up runs what needs no list: the second set's first pass then meets lists of 128 entries, outgrows
# them (PREFIX selects 270 pairs, BIG 1 330) and is repeated -- the lists grow on the second set only
WARM_UP = tuple(R.OPS)
WARM_UP_SHORT = ("cards", "matrix-smh_matches", "merge_groups")


@pytest.mark.parametrize("names,flavour", CASES, ids=["->".join(t) + "-" + f for t, f in CASES])
def test_transition(lib, names, flavour):
    first, then, knobs, extra = FLAVOURS[flavour]
    live = Live(lib, knobs, inplace_rows=330 if extra.get("inplace") else 0)
    try:
        live.replace(names[0], first, extra.get("device_cards", False))
        for name in WARM_UP_SHORT if flavour == "init_cap128" else WARM_UP:
            check(live, name)
        for y in names[1:]:
            live.replace(y, then, extra.get("device_cards", False))
            sel, S = live.sel, live.S
            if flavour == "init_cap128":
                check(live, "smh_a-sig")
                assert sel.last_attempts() > 1, "the lists did not grow on the second set"
            for name in R.OPS:
                check(live, name)
            if S.p_hll == 14 and S.n_d >= 2:
                assert sel.get_param("query_db_sig_builds") == 1 and sel.get_param("query_db_index_builds") == 1, \
                    "the database's signatures and index are built once behind a replacement"
            assert sel.get_param("hll_khi") == (0 if knobs.get("hist_algo") == 0 or S.p_hll != 14 or not S.n_d
                                                else R.bitplane_model.khi(S.D.hll))
    finally:
        live.close()


# ---- (b) random walks ----------------------------------------------------------------------------------------------------------------
KNOB_FLIPS = {"sig_cache": (0, 1), "small_pass": (0, -1), "pipeline": (0, 2), "group_min_n": (0, 2048), "hist_sparse": (-1, 0, 1),
              "hist_image": (-1, 0, 1), "query_index_dir": (0, 1), "join_form": (0, 1, 2)}


@pytest.mark.parametrize("seed", [11, 12, 13, 14])
def test_walk(lib, seed):
    rng = np.random.default_rng(seed)
    live = Live(lib)
    ops = sorted(R.OPS)
    try:
        live.replace("BIG", "upload")
        for step in range(60):
            kind = rng.choice(["db", "queries", "knob", "op", "op", "op"])
            if kind == "db":
                live.replace(str(rng.choice(R.NAMES)), str(rng.choice(["upload", "attach"])))
            elif kind == "queries":
                if live.S.p_hll == 14:
                    live.queries(int(rng.choice([Q_CUT, live.S.n_q])), str(rng.choice(["upload", "attach"])))
            elif kind == "knob":
                name = str(rng.choice(sorted(KNOB_FLIPS)))
                value = int(rng.choice(KNOB_FLIPS[name]))
                live.log.append(("knob", name, value))
                live.knob(name, value)
            else:
                try:
                    check(live, str(rng.choice(ops)))
                except AssertionError as e:
                    raise AssertionError(f"seed {seed}, step {step}: {e}\nthe walk: {live.log}") from None
    finally:
        live.close()


# ---- (c) a refused upload ------------------------------------------------------------------------------------------------------------
def bad_cards(cards):
    nan, neg = cards.copy(), cards.copy()
    nan[len(nan) // 2] = np.nan
    neg[0] = -1.0
    return {"reversed": cards[::-1].copy(), "one NaN": nan, "one negative": neg}


def test_refused_upload_leaves_the_context_alone(lib):
    B, P = lib["BIG"], lib["PREFIX"]
    live = Live(lib)
    try:
        live.replace("PREFIX", "upload")
        live.aux("upload")
        check(live, "smh_a-sig")
        for what, cards in bad_cards(B.D.cards).items():
            with pytest.raises(SelhipError) as e:
                live.sel.upload(B.D.hll, B.D.aux, cards)
            assert e.value.code == R.BADARG, what
            assert live.sel.n == R.CUT == P.n_d
            # the results of the last pass are still there, then everything else is PREFIX's
            assert H.same(live.sel.fetch(), P.smh_a), what
            for name in ("cards", "smh_a-sig", "query-sig", "query_matrix-containment"):
                check(live, name)
            live.settle(CRIT_HLL_A)
            assert H.same(live.run(), P.hll_a), what + ": the auxiliary sketches are still there"
            live.settle()
            assert H.same(live.run(ALGO_SIG), P.smh_a) and H.same(live.sel.fetch(), P.smh_a), what
    finally:
        live.close()
    with Selector(0) as sel:                                       # a fresh context stays fresh: no set, no shape, no queries
        for what, cards in bad_cards(B.D.cards).items():
            with pytest.raises(SelhipError) as e:
                sel.upload(B.D.hll, B.D.aux, cards)
            assert e.value.code == R.BADARG and sel.n == 0
            # a pass that needs no band shape selects nothing and says SELHIP_OK; one that does is refused for the shape (m is still 0)
            sel.set_criterion(CRIT_HLL_A)
            assert len(sel.run(B.tau, MODE_CB_SMH, B.r, B.b)) == 0 and sel.result_count() == 0 and len(sel.cards()) == 0
            sel.set_criterion(CRIT_SMH_A)
            with pytest.raises(SelhipError) as e:
                sel.run(B.tau, MODE_CB_SMH, B.r, B.b)
            assert e.value.code == R.BADARG and "!= m (0)" in str(e.value)
            with pytest.raises(SelhipError) as e:
                sel.run_queries(B.tau, MODE_CB_SMH, B.r, B.b)
            assert e.value.code == R.STATE


# ---- (d) what a replacement resets and what it keeps -----------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["upload", "attach"])
def test_settings_survive_a_replacement(lib, how):
    P = lib["PREFIX"]
    live = Live(lib, {"join_form": 1, "matrix_smh_form": 3})
    sel = live.sel
    try:
        live.replace("BIG", "upload")
        live.aux("upload")
        check(live, "smh_c-smh_estimator")
        sel.set_criterion(CRIT_SMH_C)
        sel.set_measure("max_containment")
        sel.set_estimator("smh")
        sel.set_allpairs_topk(K)
        sel.set_query_topk(2)
        sel.set_topk_rounds(H.ROUND_ROWS)
        sel.set_min_matches(101)
        sel.set_row_interleave(64, 2, 1)
        sel.set_pipeline(2)
        sel.set_candidate_begin(40)
        live.replace("PREFIX", how, queries=False)
        # reset: results, queries, auxiliary sketches, candidate begin
        for call in (sel.result_count, sel.fetch, sel.stats):
            with pytest.raises(SelhipError) as e:
                call()
            assert e.value.code == R.STATE
        # kept: the settings, read back where the interface reads them back ...
        assert sel.get_param("allpairs_topk") == K and sel.get_param("query_topk") == 2 and sel.get_param("topk_rounds") == H.ROUND_ROWS
        # ... and seen at work where it does not: a pass under the kept criterion, measure, estimator, top-k, rounds and interleave
        # gives what the models say for exactly those settings, over every candidate (the candidate begin is 0 again)
        sel.run(P.tau, pkg.MODE_SMH, P.r, P.b, fetch=False)
        got = sel.fetch_ranked()
        assert sel.get_param("topk_rounds_used") >= 1
        want = kept_settings_answer(P)
        assert H.same(got, want), H.describe(got, want)
        sel.set_topk_rounds(0)
        sel.set_allpairs_topk(0)
        sel.set_estimator("hll")
        sel.set_measure("jaccard")
        sel.set_row_interleave(128, 1, 0)
        sel.set_criterion(CRIT_HLL_A)
        with pytest.raises(SelhipError) as e:                      # the auxiliary sketches are gone ...
            sel.run(P.tau, MODE_CB_SMH, P.r, P.b)
        assert e.value.code == R.STATE
        queries_gone(sel, P)
        assert sel.get_param("query_db_sig_builds") == 0 and sel.get_param("query_db_index_builds") == 0
        # two set_param values: one read back, one seen at work ("join_form" 1 is the zero-half join, kernel FORM 2), and the pipeline
        assert sel.get_param("matrix_smh_form") == 3
        live.settle()
        assert H.same(live.run(ALGO_SIG), P.smh_a) and sel.get_param("join_form_used") == 2 and sel.get_param("chunks") == 2
    finally:
        live.close()


def queries_gone(sel, P):
    """a query pass answers SELHIP_E_STATE without queries (include/selection_hip.h), a query matrix SELHIP_E_BADARG ("no queries attached")"""
    for call, code in ((lambda: sel.run_queries(P.tau, MODE_CB_SMH, P.r, P.b), R.STATE), (lambda: sel.query_matrix("containment"), R.BADARG)):
        with pytest.raises(SelhipError) as e:
            call()
        assert e.value.code == code


def kept_settings_answer(P):
    """smh_c at c_min 101 under max containment with the SuperMinHash estimator, MODE_SMH, rows of part 1 of 2 in blocks of 64, every
    genome's K best partners: smhv_model and topk_rounds_model"""
    import smhv_model
    import topk_rounds_model
    from cuda_selection_criteria_amd.distributed import interleave_owner
    rec = smhv_model.expected(P.D.aux, P.D.cards, P.tau, use_cb=False, measure="max_containment", c_min=101, counts=P.counts)[0]
    mine = interleave_owner(rec["i"], 64, 2) == 1
    return topk_rounds_model.ranked_cut(topk_rounds_model.both_members(H.by_ik(rec[mine])), K)
