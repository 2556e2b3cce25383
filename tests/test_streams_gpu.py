"""Every entry point on a caller's NON-BLOCKING stream (include/selection_hip.h: selhip_ctx_set_stream, and the launchers that are
"asynchronous on hip_stream").  Each case runs three times on one context -- warm-up on a decoy set, run A with the caller's stream
late, run B with the null stream blocked -- as tests/stream_harness.py describes; the expected values are the oracle's and the
models', pinned to differ between the two sets by tests/test_streams_host.py.

The stream is a torch pool stream (non-blocking) that was SEEN to run beside a blocked null stream: with 4 hardware queues two streams
can share one.  If none of 8 candidates does, the tests fail and name that premise; they do not skip.

Known exceptions
  * selhip_hll_bitslice, selhip_hll_union_hist_planes, selhip_components and selhip_greedy_representatives (behind components() and
    greedy_representatives()) allocate and free their scratch in every call; they have no context to keep it in.  hipFree waits for the
    whole device, the blocked null stream included, so they get run A only.
  * selhip_spanning_forest, selhip_linkage and selhip_ctx_linkage (its n * n cells of scratch) allocate and free in every call too: run A,
    and run B for its ANSWER alone -- the null stream held by a fixed delay, which the call's hipFree waits out, and no question whether
    it is still held afterwards.  Their rounds are launched one after the other from words the host has just read back; with the
    stream idle in between, a launch left on the null stream shows only while that stream is held.  selhip_ctx_spanning_forest keeps
    its scratch in the context and gets all three runs.
  * A pass that outgrows its lists ("init_cap") frees the old ones and allocates larger ones before it repeats: the same wait.  It
    gets run A only, on a fresh context whose lists are still small.
  * SELHIP_ALGO_INDEX builds its index in the first pass behind an attach of the database, in sort scratch (20 bytes per genome and
    band plus rocPRIM's) that it frees as soon as the index stands -- twice the index's own size, not worth keeping for a build that
    runs once per database.  Found by run B.  Run A covers the build; run B runs the probe against the index HELD: its database is
    attached before the null stream is blocked and only the queries change (index_held_in_run_b).
  * A context's second chunk lane is a stream the library creates.  If it shares the null stream's hardware queue, its work waits
    behind run B's delay whatever the library does; the chunk-lane case therefore takes the first of up to 4 contexts whose warmed
    pass is seen to finish beside a blocked null stream, and fails naming that premise if there is none.
  * Out of scope: the drop-in launchers of section 1 (null stream by contract), selhip_multi_select and selhip_ooc_select (they own
    their streams and free at the end), the CLI."""
import ctypes as C

import numpy as np
import pytest
import torch

import stream_harness as H
from stream_harness import K, M, N_BLOCK, N_D, N_Q, P_AUX, TAU

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import (ALGO_AUTO, ALGO_HASHJOIN, ALGO_INDEX, ALGO_SIG, ALGO_STREAM, CRIT_HLL_A, CRIT_HLL_A_SMH_A,
                                         CRIT_NONE, CRIT_SMH_A, CRIT_SMH_C, FP_FMA, MODE_CB_SMH, PAIR_DTYPE, Selector)
from cuda_selection_criteria_amd._lib import Forest, Linkage, check

pytestmark = pytest.mark.gpu

R, B = H.banding()
NO_STREAM = "no torch pool stream of 8 candidates completed a tiny op while the null stream was held by a delay: the premise of these " \
            "tests (a non-blocking stream that runs beside the null stream) does not hold on this machine"


class Rig:
    def __init__(self, oracle):
        self.sets = {name: H.Sets(oracle, name) for name in ("real", "decoy")}
        self.clock = H.Clock()
        self.streams = H.pick_streams(self.clock)


@pytest.fixture(scope="module")
def rig(oracle):
    return Rig(oracle)


@pytest.fixture
def env(rig):
    assert rig.streams, NO_STREAM
    e = H.Env(rig.clock, rig.streams[0], rig.sets)
    e.selectors = []
    yield e
    torch.cuda.synchronize()
    for sel in e.selectors:
        sel.close()


def selector(env, stream="own", **params):
    sel = Selector(0, stream=(env.s if stream == "own" else stream).cuda_stream if stream is not None else None)
    for name, value in params.items():
        sel.set_param(name, value)
    env.selectors.append(sel)
    return sel


def attach(env, sel, queries=False):
    """attach waits for the stream and takes its snapshots (bit planes, cards) of what the working tensors hold by then"""
    T = env.T
    sel.attach(T["hll"], T["aux"], T["cards"])
    if queries:
        sel.attach_queries(T["q_hll"], T["q_aux"], T["q_cards"])


def index_held_in_run_b(env):
    """ALGO_INDEX builds its index in the first pass behind an attach of the database, in scratch it frees when the index stands (known
    exceptions).  Runs warm-up and A attach the database and so build the index on the stream; run B does not: its restore run holds the
    REAL database already (and the decoy's queries), the index of that database is held, and only the queries change under the delay"""
    env.real_in_restore = {"hll", "aux", "cards"}


def attach_for_queries(env, sel, algo):
    if algo == ALGO_INDEX and env.phase == "B":
        sel.attach_queries(env.T["q_hll"], env.T["q_aux"], env.T["q_cards"])
    else:
        attach(env, sel, queries=True)


def ptr(stream):
    return C.c_void_p(stream.cuda_stream)


# ---- the cases: setup(env) -> body, or (body, keyword arguments of three_runs) -------------------------------------------------------
SETUP = {}


def case(*ids):
    def register(fn):
        for case_id in ids:
            assert case_id in H.CASES and case_id not in SETUP, case_id
            SETUP[case_id] = (lambda f, c: lambda env: f(env, c))(fn, case_id)
        return fn
    return register


ALLPAIRS = {
    # id: (criterion, algo, context parameters, preparation behind attach, check behind the pass)
    "smh_a-sig": (CRIT_SMH_A, ALGO_SIG, {}, None, None),
    "smh_a-stream": (CRIT_SMH_A, ALGO_STREAM, {}, None, None),
    "smh_a-hashjoin": (CRIT_SMH_A, ALGO_HASHJOIN, {}, None, None),
    "smh_a-small_pass": (CRIT_SMH_A, ALGO_AUTO, {"small_pass": 1}, None, lambda sel: sel.get_param("small_pass_used") == 1),
    "hll_a-uploaded": (CRIT_HLL_A, ALGO_AUTO, {}, lambda sel, env: sel.upload_aux_hll(env.data.D.aux_hll, P_AUX), None),
    "hll_a-folded": (CRIT_HLL_A, ALGO_AUTO, {}, lambda sel, env: sel.fold_aux_hll(P_AUX), None),
    "hll_a+smh_a": (CRIT_HLL_A_SMH_A, ALGO_AUTO, {}, lambda sel, env: sel.attach_aux_hll(env.T["aux_hll"], P_AUX), None),
    "none-list_route": (CRIT_NONE, ALGO_AUTO, {"dense_fused": 0}, None, lambda sel: sel.get_param("dense_route_used") == 0),
    "none-fused": (CRIT_NONE, ALGO_AUTO, {"dense_fused": 1}, None, lambda sel: sel.get_param("dense_route_used") == 1),
    "smh_c": (CRIT_SMH_C, ALGO_AUTO, {}, lambda sel, env: sel.set_min_matches(H.C_MIN), None),
    "smh_c-smh_estimator": (CRIT_SMH_C, ALGO_AUTO, {}, lambda sel, env: (sel.set_min_matches(H.C_MIN), sel.set_estimator("smh")), None),
}


def allpairs_body(sel, case_id):
    crit, algo, _, prepare, holds = ALLPAIRS[case_id]

    def body(env):
        attach(env, sel)
        sel.set_criterion(crit)
        if prepare:
            prepare(sel, env)
        env.stall()
        got = sel.run(TAU, MODE_CB_SMH, R, B, algo=algo)
        assert sel.last_attempts() == 1
        assert holds is None or holds(sel), case_id
        if env.phase == "A":
            # selhip_ctx_run returns when the pass is complete: the list on the device may be read from any stream -- here by a
            # plain hipMemcpy, which goes through the null stream (run B cannot: its null stream is blocked)
            where, count = sel.result_device()
            raw = np.zeros(count, dtype=PAIR_DTYPE)
            check(pkg.hip_lib().selhip_memcpy_d2h(raw.ctypes.data, where, raw.nbytes))
            assert H.same(H.by_ik(raw), got), "the result list read through the null stream behind selhip_ctx_run"
        return got
    return body


@case(*ALLPAIRS)
def _allpairs(env, case_id):
    env.database(aux_hll=case_id == "hll_a+smh_a")
    return allpairs_body(selector(env, **ALLPAIRS[case_id][2]), case_id)


@case("smh_a-chunks2")
def _chunks(env, case_id):
    """two chunk lanes: lane 1 is the library's own stream, started by an event of the context's stream and joined by another"""
    env.database()

    def body_of(sel):
        def body(env):
            attach(env, sel)
            env.stall()
            got = sel.run(TAU, MODE_CB_SMH, R, B, algo=ALGO_SIG)
            assert sel.get_param("chunks") == 2
            return got
        return body

    for _ in range(4):
        sel = selector(env)
        sel.set_pipeline(2)
        if H.runs_beside_null(env, body_of(sel)):
            return body_of(sel)
    pytest.fail("none of 4 contexts finished a warmed two-lane pass while the null stream was held by a delay: either every context's "
                "second lane shares the null stream's hardware queue (a limit of the machine's queues), or the two-lane pass waits "
                "for the null stream or the device")


@case("grown_lists")
def _grown(env, case_id):
    """lists that start too small: the pass is repeated (selhip_ctx_finish enqueues it again) after they grew"""
    env.database()
    ctx = {}

    def fresh():
        ctx["sel"] = selector(env, init_cap=64)

    def body(env):
        sel = ctx["sel"]
        attach(env, sel)
        env.stall()
        got = sel.run(TAU, MODE_CB_SMH, R, B, algo=ALGO_SIG)
        assert sel.last_attempts() > 1
        return got
    fresh()
    return body, {"fresh": fresh}


def unframe(rec):
    cnt = int(rec[0, 0])
    return H.by_ik(rec[1:1 + cnt].reshape(-1).view(PAIR_DTYPE))


@case("run_async-framed-finish")
def _async(env, case_id):
    env.database()
    sel = selector(env)
    frame = torch.zeros((2048 + 1, 2), dtype=torch.int64, device="cuda")
    env.poison(frame)

    def body(env):
        attach(env, sel)
        env.stall()
        sel.run_async(TAU, MODE_CB_SMH, R, B, algo=ALGO_SIG)
        env.still_running("selhip_ctx_run_async")
        sel.copy_results_framed_async(frame)
        env.still_running("selhip_ctx_copy_results_framed_async")
        sel.finish()
        assert sel.last_attempts() == 1 and sel.result_count() <= 2048
        got = unframe(env.host(frame))
        assert H.same(sel.fetch(), got)
        return got
    return body


QUERY = {"query-sig": (ALGO_SIG, None), "query-stream": (ALGO_STREAM, None), "query-index": (ALGO_INDEX, None), "query-topk": (ALGO_SIG, K)}


@case(*QUERY)
def _query(env, case_id):
    env.database(queries=True)
    sel = selector(env)
    algo, top_k = QUERY[case_id]
    if algo == ALGO_INDEX:
        index_held_in_run_b(env)

    def body(env):
        attach_for_queries(env, sel, algo)
        env.stall()
        got = sel.run_queries(TAU, MODE_CB_SMH, R, B, algo=algo, top_k=top_k)
        assert algo != ALGO_INDEX or sel.get_param("query_db_index_builds") == 1
        return got
    return body


@case("allpairs-topk")
def _topk(env, case_id):
    env.database()
    sel = selector(env)

    def body(env):
        attach(env, sel)
        env.stall()
        return sel.run(TAU, MODE_CB_SMH, R, B, algo=ALGO_SIG, top_k=K)
    return body


@case("allpairs-topk-rounds")
def _topk_rounds(env, case_id):
    env.database()
    sel = selector(env)

    def body(env):
        attach(env, sel)
        sel.set_criterion(CRIT_SMH_C)
        sel.set_min_matches(H.C_MIN)
        sel.set_estimator("smh")
        env.stall()
        got = sel.run(TAU, MODE_CB_SMH, R, B, top_k=K, rounds=H.ROUND_ROWS)
        assert sel.get_param("topk_rounds_used") == -(-N_D // H.ROUND_ROWS)
        return got
    return body


@case("pairs-signature_route", "pairs-direct_route")
def _pairs(env, case_id):
    env.database(extra=lambda S: {"pairs": S.pair_list}, late=("pairs",))
    sel = selector(env)
    route = 1 if case_id == "pairs-signature_route" else 0

    def body(env):
        attach(env, sel)
        env.stall()                                     # (run A: the list is written here, behind the second delay)
        sel.run_pairs_async(env.T["pairs"], TAU, MODE_CB_SMH, R, B, algo=ALGO_SIG if route else ALGO_STREAM)
        env.still_running("selhip_ctx_run_pairs_async")
        sel.finish()
        assert sel.get_param("pairs_route_used") == route and sel.last_attempts() == 1
        return sel.fetch()
    return body


@case("matrix-jaccard", "matrix-smh_matches")
def _matrix(env, case_id):
    measure = case_id.split("-")[1]
    env.database(extra=(lambda S: {"aux": S.dense_aux}) if measure == "smh_matches" else None)
    sel = selector(env)
    out = torch.empty((N_D, N_D), dtype=torch.float64, device="cuda")
    env.poison(out)

    def body(env):
        attach(env, sel)
        env.stall()
        assert sel.matrix(measure, out=out) is out
        return env.host_any_stream(out)                 # (the call returns when the matrix is complete: any stream may read it)
    return body


@case("query_matrix-containment")
def _query_matrix(env, case_id):
    env.database(queries=True)
    sel = selector(env)
    out = torch.empty((N_Q, N_D), dtype=torch.float64, device="cuda")
    env.poison(out)

    def body(env):
        attach(env, sel, queries=True)
        env.stall()
        sel.query_matrix("containment", row_pos=env.data.row_pos, col_pos=env.data.col_pos, out=out)
        return env.host_any_stream(out)
    return body


@case("cluster", "cluster_greedy-priority")
def _cluster(env, case_id):
    greedy = case_id != "cluster"
    env.database(extra=(lambda S: {"prio": S.prio}) if greedy else None, late=("prio",) if greedy else ())
    sel = selector(env)

    def body(env):
        attach(env, sel)
        env.stall(late=False)
        sel.run(TAU, MODE_CB_SMH, R, B, algo=ALGO_SIG, fetch=False)
        env.stall()                                     # (run A: another delay in front of the cluster call; the priorities are written behind it)
        if greedy:
            res = sel.cluster_greedy(order="priority", priority=env.T["prio"], to_host=False)
            res.pop("rounds")
        else:
            res = sel.cluster(rep="max_degree", to_host=False)
        first = next(iter(res))
        return {k: env.host_any_stream(v) if k == first else (v if k == "n_clusters" else env.host(v)) for k, v in res.items()}
    return body


def record_outputs(n):
    """the two caller-owned arrays of a hierarchy call for n vertices (records as bytes, int32 words), poisoned in front of every call"""
    rec = torch.empty((n - 1, PAIR_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    words = torch.empty(n - 1, dtype=torch.int32, device="cuda")
    return rec, words


def first_records(env, rec, f, what):
    """the first f records of a poisoned record array, read behind a call that returns when they are complete; the entries from f on
    still hold the poison"""
    raw = env.host_any_stream(rec)
    assert 0 <= f <= len(raw) and np.all(raw[f:] == 0xA5), f"{what}: the entries from F = {f} on are not the poison any more"
    return np.ascontiguousarray(raw[:f]).reshape(-1).view(PAIR_DTYPE)


@case("forest")
def _forest(env, case_id):
    """the smh_a signature pass, then the maximum spanning forest of its list (scratch the context holds: run B too)"""
    env.database()
    sel = selector(env)
    edges = torch.empty((N_D - 1, PAIR_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    labels = torch.empty(N_D, dtype=torch.int32, device="cuda")
    env.poison(edges, labels)

    def body(env):
        attach(env, sel)
        env.stall(late=False)
        sel.run(TAU, MODE_CB_SMH, R, B, algo=ALGO_SIG, fetch=False)
        env.stall()                                     # (run A: another delay in front of the forest call)
        out, cnt = Forest(edges.data_ptr(), labels.data_ptr()), C.c_int64(-5)
        check(sel._lib.selhip_ctx_spanning_forest(sel._ctx, float("-inf"), C.byref(out), C.byref(cnt)), sel._ctx)
        assert sel.get_param("forest_edges_last") == cnt.value
        return {"edges": first_records(env, edges, cnt.value, case_id), "labels": env.host(labels)}
    return body


@case(*H.LINKAGE_CASES)
def _linkage(env, case_id):
    """selhip_ctx_linkage: n * n cells of scratch taken and released in the call, the matrix kernels, then up to 2 (n - 1) + 1 rounds
    whose launch shapes the host reads back from the stream"""
    measure, method, capped = H.LINKAGE_CASES[case_id]
    env.database(extra=(lambda S: {"aux": S.dense_aux}) if measure == "smh_jaccard" else None)
    sel = selector(env)
    merges, sizes = record_outputs(N_D)
    env.poison(merges, sizes)

    def body(env):
        attach(env, sel)
        env.stall()
        out, cnt = Linkage(merges.data_ptr(), sizes.data_ptr()), C.c_int64(-5)
        cap = env.data.linkage_cap if capped else float("inf")
        check(sel._lib.selhip_ctx_linkage(sel._ctx, pkg.measure_code(measure), pkg.linkage_code(method), cap, C.byref(out), C.byref(cnt)), sel._ctx)
        f = cnt.value
        assert sel.get_param("linkage_merges_last") == f
        got_sizes = env.host(sizes)
        assert np.all(got_sizes[f:] == -7), f"{case_id}: the sizes from F = {f} on are not the poison any more"
        return {"merges": first_records(env, merges, f, case_id), "sizes": got_sizes[:f], "rounds": sel.get_param("linkage_rounds_last")}
    return body


@case("two_contexts")
def _two_contexts(env, case_id):
    """two contexts on two streams over the same attached tensors; both passes are enqueued before either is finished"""
    env.database()
    assert len(env.rig_streams) > 1, NO_STREAM + " (a second one)"
    s2 = env.rig_streams[1]
    one, two = selector(env), selector(env, stream=s2)

    def body(env):
        attach(env, one)
        with torch.cuda.stream(s2):
            attach(env, two)
            two.set_criterion(CRIT_SMH_C)
            two.set_min_matches(H.C_MIN)
            if env.phase == "A":
                env.clock.sleep(H.DELAY_MS)
        env.stall()
        one.run_async(TAU, MODE_CB_SMH, R, B, algo=ALGO_SIG)
        two.run_async(TAU, MODE_CB_SMH, R, B)
        env.still_running("selhip_ctx_run_async")
        assert env.phase != "A" or not s2.query(), "selhip_ctx_run_async returned with the second stream idle under run A"
        two.finish()
        one.finish()
        got2 = two.fetch()
        assert H.same(got2, H.expected(env.data, "smh_c")), "the second context (smh_c, second stream): " + H.describe(got2, env.data.smh_c)
        return one.fetch()
    return body, {"streams": (s2,)}


# ---- block launchers and Python helpers ------------------------------------------------------------------------------------------------
def launcher(env, make, outputs, call, result, asynchronous=True, late=()):
    """a launcher case: make(Sets) -> its input arrays, outputs -> its output tensors (poisoned on the stream in front of every call),
    call(T, stream pointer), result() -> the outputs on the host.  late: the inputs written behind run A's second delay"""
    env.tensors(make, late)
    env.poison(*outputs)

    def body(env):
        env.stall()
        call(env.T, ptr(env.s))
        if asynchronous:
            env.still_running("the launcher")
        return result()
    return body


@case("selhip_smh_a_pairs")
def _b_smh_a(env, case_id):
    out = torch.empty(N_BLOCK, dtype=torch.uint8, device="cuda")
    return launcher(env, lambda S: {"aux": S.D.aux, "pairs": S.block_pairs}, [out],
                    lambda T, st: check(pkg.hip_lib().selhip_smh_a_pairs(T["aux"].data_ptr(), M, R, B, T["pairs"].data_ptr(), N_BLOCK, out.data_ptr(), st)),
                    lambda: env.host(out))


@case("selhip_hll_union_hist")
def _b_hist(env, case_id):
    out = torch.empty((N_BLOCK, 64), dtype=torch.int32, device="cuda")
    return launcher(env, lambda S: {"hll": S.D.hll, "pairs": S.block_pairs}, [out],
                    lambda T, st: check(pkg.hip_lib().selhip_hll_union_hist(T["hll"].data_ptr(), 14, T["pairs"].data_ptr(), N_BLOCK, out.data_ptr(), st)),
                    lambda: env.host(out).view(np.uint32))


@case("selhip_ertl_estimate")
def _b_estimate(env, case_id):
    out = torch.empty(N_BLOCK, dtype=torch.float64, device="cuda")
    return launcher(env, lambda S: {"counts": S.block_hist}, [out],
                    lambda T, st: check(pkg.hip_lib().selhip_ertl_estimate(T["counts"].data_ptr(), N_BLOCK, 14, FP_FMA, out.data_ptr(), st)),
                    lambda: env.host(out))


@case("selhip_smh_match_counts")
def _b_matches(env, case_id):
    out = torch.empty(N_BLOCK, dtype=torch.int32, device="cuda")
    return launcher(env, lambda S: {"aux": S.D.aux, "pairs": S.block_pairs}, [out],
                    lambda T, st: check(pkg.hip_lib().selhip_smh_match_counts(T["aux"].data_ptr(), M, T["pairs"].data_ptr(), N_BLOCK, out.data_ptr(), st)),
                    lambda: env.host(out))


@case("selhip_hll_fold")
def _b_fold(env, case_id):
    out = torch.empty((64, 1 << P_AUX), dtype=torch.uint8, device="cuda")
    return launcher(env, lambda S: {"hll": S.D.hll[:64]}, [out],
                    lambda T, st: check(pkg.hip_lib().selhip_hll_fold(T["hll"].data_ptr(), 64, 14, P_AUX, out.data_ptr(), st)),
                    lambda: env.host(out))


@case("selhip_synth_generate")
def _b_synth(env, case_id):
    """no device input: what is late here is the stream's own earlier write to the outputs (the poison)"""
    n = 48
    hll = torch.empty((n, 1 << 14), dtype=torch.uint8, device="cuda")
    aux = torch.empty((n, M), dtype=torch.int64, device="cuda")
    aux_hll = torch.empty((n, 1 << P_AUX), dtype=torch.uint8, device="cuda")

    def call(T, st):
        sp = env.data.synth_cfg.struct()
        check(pkg.hip_lib().selhip_synth_generate(C.byref(sp), 0, n, hll.data_ptr(), aux.data_ptr(), aux_hll.data_ptr(), st))
    return launcher(env, lambda S: {}, [hll, aux, aux_hll], call,
                    lambda: {"hll": env.host(hll), "aux": env.host(aux).view(np.uint64), "aux_hll": env.host(aux_hll)})


@case("selhip_build_sketches")
def _b_build(env, case_id):
    n = 3
    hll = torch.empty((n, 1 << 14), dtype=torch.uint8, device="cuda")
    smh = torch.empty((n, 64), dtype=torch.int64, device="cuda")
    aux_hll = torch.empty((n, 1 << P_AUX), dtype=torch.uint8, device="cuda")
    return launcher(env, lambda S: {"codes": S.build_codes[0], "offsets": S.build_codes[1]}, [hll, smh, aux_hll],
                    lambda T, st: check(pkg.hip_lib().selhip_build_sketches(T["codes"].data_ptr(), T["offsets"].data_ptr(), n, 31, 64, P_AUX,
                                                                            hll.data_ptr(), smh.data_ptr(), aux_hll.data_ptr(), st)),
                    lambda: {"hll": env.host(hll), "smh": env.host(smh).view(np.uint64), "aux_hll": env.host(aux_hll)})


@case("selhip_permute_rows")
def _b_permute(env, case_id):
    out = torch.empty((N_D, M), dtype=torch.int64, device="cuda")
    return launcher(env, lambda S: {"src": S.D.aux, "perm": S.perm}, [out],
                    lambda T, st: check(pkg.hip_lib().selhip_permute_rows(T["src"].data_ptr(), out.data_ptr(), T["perm"].data_ptr(), N_D, M * 8, st)),
                    lambda: env.host(out).view(np.uint64))


@case(*H.PERMUTE_SHAPES)
def _b_permute_shapes(env, case_id):
    """the shapes of selhip_permute_rows no other test reaches, each against src[perm]: rows are staged into buffers at the byte
    offset of the case, so that a 16-byte-multiple row through unaligned pointers takes the byte kernel too"""
    rows, row_bytes, offset = H.PERMUTE_SHAPES[case_id]
    size = rows * row_bytes
    src = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
    dst = torch.empty(size + 16, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0

    def call(T, st):
        src[offset:offset + size].copy_(T["src"].reshape(-1), non_blocking=True)
        check(pkg.hip_lib().selhip_permute_rows(src.data_ptr() + offset, dst.data_ptr() + offset, T["perm"].data_ptr(), rows, row_bytes, st))
    return launcher(env, lambda S: {k: v for k, v in S.permute_data(case_id).items() if k != "want"}, [dst], call,
                    lambda: env.host(dst)[offset:offset + size].reshape(rows, row_bytes))


@case("selhip_hll_bitslice+union_hist_planes")
def _b_planes(env, case_id):
    """both wait for the stream, and both free their scratch before they return (run A only)"""
    planes = torch.empty((N_D, 6, 512), dtype=torch.int32, device="cuda")
    gmax = torch.empty(N_D, dtype=torch.uint8, device="cuda")
    out = torch.empty((N_BLOCK, 64), dtype=torch.int32, device="cuda")

    def call(T, st):
        khi = C.c_int(0)
        lib = pkg.hip_lib()
        check(lib.selhip_hll_bitslice(T["hll"].data_ptr(), N_D, planes.data_ptr(), gmax.data_ptr(), C.byref(khi), st))
        check(lib.selhip_hll_union_hist_planes(planes.data_ptr(), gmax.data_ptr(), khi.value, T["pairs"].data_ptr(), N_BLOCK, out.data_ptr(), st))
    return launcher(env, lambda S: {"hll": S.D.hll, "pairs": S.block_pairs}, [planes, gmax, out], call,
                    lambda: env.host_any_stream(out).view(np.uint32), asynchronous=False)


@case("components")
def _b_components(env, case_id):
    env.tensors(lambda S: {"edges": S.edges})

    def body(env):
        env.stall()
        return env.host_any_stream(pkg.components(env.T["edges"], N_D, to_host=False))       # (under torch.cuda.stream(s): the helper takes torch's current stream)
    return body


@case("greedy_representatives")
def _b_greedy(env, case_id):
    env.tensors(lambda S: {"edges": S.edges})

    def body(env):
        env.stall()
        is_rep, rounds = pkg.greedy_representatives(env.T["edges"], N_D, keys=env.data.keys, to_host=False)
        assert rounds >= 1
        return env.host_any_stream(is_rep)
    return body


@case("selhip_spanning_forest")
def _b_forest(env, case_id):
    """the edge list and its values are late inputs; the entry owns its scratch and waits for the stream"""
    edges = torch.empty((N_D - 1, PAIR_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    labels = torch.empty(N_D, dtype=torch.int32, device="cuda")
    f, rounds = C.c_int64(-5), C.c_int64(-5)

    def call(T, st):
        check(pkg.hip_lib().selhip_spanning_forest(T["edges"].data_ptr(), T["values"].data_ptr(), H.N_EDGES, N_D, edges.data_ptr(), labels.data_ptr(),
                                                   C.byref(f), C.byref(rounds), st))
    return launcher(env, lambda S: {"edges": S.edges, "values": S.forest_values}, [edges, labels], call,
                    lambda: {"edges": first_records(env, edges, f.value, case_id), "labels": env.host(labels)},
                    asynchronous=False, late=("edges", "values"))


@case("selhip_linkage")
def _b_linkage(env, case_id):
    """average linkage of a caller's matrix, a late input, in both layouts of H.LINKAGE_LAYOUTS: the matrix is staged on the stream into a
    buffer of the layout's leading dimension and base (the call consumes it), and each layout has poisoned outputs of its own"""
    n = N_D
    lay = {}
    for tag, (ld_extra, offset) in H.LINKAGE_LAYOUTS.items():
        ld = n + ld_extra
        buf = torch.full((n * ld + 2 + offset,), float("nan"), dtype=torch.float64, device="cuda")
        assert buf.data_ptr() % 16 == 0
        lay[tag] = (buf[offset:offset + n * ld].view(n, ld), ld, *record_outputs(n), C.c_int64(-5), C.c_int64(-5))
    assert lay["wide"][1] % 2 == 0 and lay["wide"][0].data_ptr() % 16 == 0 and lay["narrow"][1] % 2 == 1 and lay["narrow"][0].data_ptr() % 16 == 8

    def call(T, st):
        for view, ld, merges, sizes, f, rounds in lay.values():
            view[:, :n].copy_(T["dist"], non_blocking=True)
            check(pkg.hip_lib().selhip_linkage(view.data_ptr(), n, ld, pkg.LINKAGE_AVERAGE, float("inf"), merges.data_ptr(), sizes.data_ptr(),
                                               C.byref(f), C.byref(rounds), st))

    def result():
        out = {}
        for tag, (_, _, merges, sizes, f, rounds) in lay.items():
            got_sizes = env.host(sizes)
            assert np.all(got_sizes[f.value:] == -7), (case_id, tag)
            out.update({f"merges-{tag}": first_records(env, merges, f.value, case_id), f"sizes-{tag}": got_sizes[:f.value], f"rounds-{tag}": rounds.value})
        return out
    outputs = [t for v in lay.values() for t in v[2:4]]
    return launcher(env, lambda S: {"dist": S.linkage_dist}, outputs, call, result, asynchronous=False, late=("dist",))


SWITCHES = ("switch-sig_cache", "switch-query_index")


def test_every_case_has_a_body():
    assert set(SETUP) | set(SWITCHES) == set(H.CASES)


@pytest.mark.parametrize("case_id", sorted(SETUP))
def test_late_stream_and_blocked_null_stream(rig, env, case_id):
    env.rig_streams = rig.streams
    made = SETUP[case_id](env)
    body, options = made if isinstance(made, tuple) else (made, {})
    H.three_runs(env, body, lambda S: H.expected(S, case_id), run_b_too=case_id not in H.RUN_A_ONLY,
                 answer_only=case_id in H.ANSWER_UNDER_BLOCKED_NULL, **options)


@pytest.mark.parametrize("case_id", SWITCHES)
def test_stream_switches(rig, env, case_id):
    """one context from stream to stream, its cached products with it: a pass on the null stream, selhip_ctx_set_stream(s) and a pass
    under run A, back to the null stream, then a second stream s2 under runs A and B, and at last back to s WITHOUT attaching again,
    behind a delay: the signature cache ("sig_cache" 1) or the query index built on s2 is read on s"""
    assert len(rig.streams) > 1, NO_STREAM + " (a second one)"
    s, s2 = rig.streams[:2]
    null = torch.cuda.default_stream()
    query = case_id == "switch-query_index"
    env.database(queries=query)
    sel = selector(env, stream=None, sig_cache=1)
    want = lambda S: H.expected(S, case_id)             # noqa: E731
    builds = "query_db_index_builds" if query else "query_db_sig_builds"

    def the_pass(env):
        env.stall()
        if query:
            return sel.run_queries(TAU, MODE_CB_SMH, R, B, algo=ALGO_INDEX)
        return sel.run(TAU, MODE_CB_SMH, R, B, algo=ALGO_SIG)

    def body(env):
        if query:
            attach_for_queries(env, sel, ALGO_INDEX)
        else:
            attach(env, sel)
        return the_pass(env)

    if query:
        index_held_in_run_b(env)

    def on(stream):
        sel.set_stream(None if stream is null else stream.cuda_stream)
        env.s = stream

    on(null)
    got = H.plain_run(env, body, "decoy")
    assert H.same(got, want(rig.sets["decoy"])), "on the null stream: " + H.describe(got, want(rig.sets["decoy"]))
    on(s)
    H.run_a(env, body, want)
    on(null)
    got = H.plain_run(env, body, "decoy")
    assert H.same(got, want(rig.sets["decoy"])), "back on the null stream: " + H.describe(got, want(rig.sets["decoy"]))
    on(s2)
    H.run_a(env, body, want)
    H.run_b(env, body, want)
    # the products of the last pass on s2 (real data) are read on s, behind a delay, by a pass that attaches nothing
    before = sel.get_param(builds)
    on(s)
    env.phase = "A"
    try:
        with torch.cuda.stream(s):
            env.loaded = "real"
            got = the_pass(env)
    finally:
        torch.cuda.synchronize()
    assert H.same(got, want(rig.sets["real"])), "on s again, nothing attached: " + H.describe(got, want(rig.sets["real"]))
    if query:
        assert sel.get_param(builds) == before == 1, "the query index was built again although the database was not attached again"
