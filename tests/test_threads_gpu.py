"""Every entry point from several host threads at once (include/selection_hip.h, "Host threads").  Different
contexts may be used from different threads at the same time, and so may the entries that take no context; selhip_ooc_select and
selhip_multi_select rest on that, and until now only the former's narrow path (attach, run, fetch, stats) ever ran beside another context.

Each thread owns one context (tests/test_context_reuse_gpu.py's Live) that holds a set of its OWN -- another n, m and seed, so that
anything crossing between contexts shows as the other set's answer -- on a non-blocking torch pool stream of its own, and makes its torch
calls under torch.cuda.stream(that stream): the threads' device work can really overlap (ctypes releases the GIL during a library call).
The sets, the 32 operations and their expected values are tests/context_reuse_model.py's; the context-free entries and theirs are
tests/thread_entries.py's.  Every comparison is bit for bit with the oracle and the models (stream_harness.same), never with a second
context or a serial run.  The threads run in a thread_harness.Crew: a failure in one is re-raised here with every thread's log, breaks the
barrier and stops the others before their next step; every wait has a time-out; behind a HIP error no test of this file starts another
GPU call.

  test_every_operation_beside_every_operation[a]   X runs a on BIG while Y runs each operation b on NARROW, one barrier per step: every
                      ordered pair meets once on warm contexts.  test_overlap_share_of_the_pairs then holds the share of steps whose two
                      stamped intervals intersect above OVERLAP_FLOOR: threads that ran one after the other would prove nothing
  test_cold_round     the same operations on two fresh contexts: both threads size their buffers at once
  test_same_shape_side_by_side   two contexts that hold sets of ONE shape (BIG, HIGHREG) and swap them: a cache key or a scratch buffer
                      shared between contexts meets a context in which every index and every key of the other one is valid
  test_walks_in_parallel[seed]   four threads, 60 free-running random steps each as test_walk takes them; one of them toggles the
                      process-wide grid hooks "cluster_blocks" and "vertex_blocks" among 0, 1 and 7 between its steps
  test_free_standing_entries_in_parallel   the context-free entries from three threads on three sets, and their first calls in a fresh
                      child process (tests/threads_child.py)
  test_context_churn_beside_work   one thread creates, loads, runs and destroys contexts (hipMalloc / hipFree: device-wide waits) while two work
  test_small_passes_side_by_side   two one-launch small passes (a grid barrier under an ordinary launch) and a regular pass, 50 times
  test_errors_stay_with_their_thread   a refusal on one thread, clean work on the other: whose message selhip_last_error gives whom"""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import context_reuse_model as R
import stream_harness as H
import thread_entries as E
import thread_harness as T
from test_context_reuse_gpu import KNOB_FLIPS, Q_CUT, RUN, Live, bad_cards, check, want_of

from cuda_selection_criteria_amd import ALGO_SIG, SelhipError
from cuda_selection_criteria_amd._lib import hip_lib

pytestmark = pytest.mark.gpu

OPS = tuple(R.OPS)
# The least share of barrier steps of test_every_operation_beside_every_operation whose two intervals must intersect.  A condition of
# the test, not a performance figure: half the lowest share of three runs of this file on an MI355X (784 of 784 steps in each, with the 28 operations of then; the
# 1 024 steps of the 32 of now are measured in DESIGN.md section 29 too), never under a quarter
OVERLAP_FLOOR = 0.50
TALLY = {"cases": 0, "steps": 0, "hits": 0}


@pytest.fixture(autouse=True)
def no_gpu_call_behind_a_hip_error():
    if T.hip_failed():
        pytest.fail(f"an earlier test of this file met a HIP error ({T.hip_failed()}): nothing more is started on the GPU")


@pytest.fixture(scope="module")
def lib(oracle):
    return R.Library(oracle)


@pytest.fixture(scope="module")
def streams():
    """four non-blocking torch pool streams with four handles"""
    out = []
    for _ in range(32):
        s = torch.cuda.Stream()
        if all(s.cuda_stream != o.cuda_stream for o in out):
            out.append(s)
        if len(out) == 4:
            return out
    pytest.fail("torch's pool gave fewer than four streams")


def prime(lib, names, ops=OPS):
    """the expected values, computed here in the calling thread once: the threads only read them"""
    for name in names:
        S = lib[name]
        for o in ops:
            R.expected(S, o)
        R.stats_expected(S)
        S.sparse_t


class Worker:
    """one thread's context: a Live on a stream of its own"""

    def __init__(self, lib, stream, knobs=None):
        self.stream = stream
        with torch.cuda.stream(stream):
            self.live = Live(lib, knobs)
            self.live.sel.set_stream(stream.cuda_stream)

    def close(self):
        if not T.hip_failed():
            self.live.close()


def close_all(workers):
    for w in workers:
        if w is not None:
            w.close()


def step(me, key, live, name):
    """one operation: the library's calls stamped, the answer compared bit for bit behind the stamp"""
    want = want_of(live, name)
    if isinstance(want, int):                                     # (a documented refusal: check() asks for its code)
        me.timed(key, lambda: check(live, name))
        return
    live.log.append(("op", live.S.name, name))
    got = me.timed(key, lambda: RUN[name](live))
    assert H.same(got, want), f"{name} on {live.S.name}: {H.describe(got, want)}"


# the operations whose last pass is the all-pairs smh_a pass without a top-k: what the context keeps of it is known
SMH_A_LAST = ("smh_a-sig", "smh_a-stream", "smh_a-hashjoin", "smh_a-chunks2", "smh_a-small_pass", "run_async-framed-finish", "cluster",
              "cluster_greedy-priority", "forest")


def second_look(live, name):
    """behind a step that BOTH threads have finished: the statistics, the count and the records a context keeps of its last pass are
    still its own -- a result counter or a statistics block that contexts shared would by now hold the other thread's"""
    if name not in SMH_A_LAST or isinstance(want_of(live, name), int):
        return
    sel, S = live.sel, live.S
    st, want, rec = sel.stats(), R.stats_expected(S), R.expected(S, "smh_a-sig")
    assert (st["evaluated"], st["survivors"], st["selected"]) == (want["evaluated"], want["survivors"], want["selected"]), \
        f"behind {name} on {S.name}, once the other thread's step was over: stats() {st}, the oracle's {want}"
    assert sel.result_count() == len(rec) and H.same(sel.fetch(), rec), f"behind {name} on {S.name}: the kept result list is not the pass's"


def share(crew, a, b):
    steps, hits = crew.overlap(a, b)
    return steps, hits, (hits / steps if steps else 0.0)


# ---- (a) every operation beside every operation ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def duo(lib, streams):
    """X holds BIG, Y holds NARROW, and each has run every operation once, serially: every buffer is sized, every cached product is its own"""
    prime(lib, ("BIG", "NARROW"))
    workers = [Worker(lib, streams[0]), Worker(lib, streams[1])]
    for w, name in zip(workers, ("BIG", "NARROW")):
        with torch.cuda.stream(w.stream):
            w.live.replace(name, "upload")
            for o in OPS:
                check(w.live, o)
    torch.cuda.synchronize()
    yield workers
    close_all(workers)


def in_step(crew, x, y, plan):
    """plan: [(what X does, what Y does)], an operation name or a callable(live); one barrier in front of every step and one behind it,
    where both contexts are asked once more for what they keep of the step (second_look)"""
    def body(w, column):
        def run(me):
            me.log = w.live.log
            with torch.cuda.stream(w.stream):
                for j, pair in enumerate(plan):
                    what = pair[column]
                    me.meet()
                    if callable(what):
                        me.timed(j, lambda: what(w.live))
                    else:
                        step(me, j, w.live, what)
                    me.meet()
                    if not callable(what):
                        second_look(w.live, what)
        return run
    crew.run({"X": body(x, 0), "Y": body(y, 1)})


@pytest.mark.parametrize("a", OPS)
def test_every_operation_beside_every_operation(duo, a):
    x, y = duo
    crew = T.Crew(["X", "Y"])
    in_step(crew, x, y, [(a, b) for b in OPS])
    steps, hits, part = share(crew, "X", "Y")
    assert steps == len(OPS)
    TALLY["cases"] += 1
    TALLY["steps"] += steps
    TALLY["hits"] += hits
    print(f"\n{a} beside every operation: the two intervals intersect in {hits} of {steps} steps ({100 * part:.0f} %)")


def test_overlap_share_of_the_pairs():
    """the guard against a vacuous run: over all barrier steps of the cases above, the share whose two intervals intersect"""
    assert TALLY["cases"] == len(OPS), "run behind all cases of test_every_operation_beside_every_operation (the whole file)"
    part = TALLY["hits"] / TALLY["steps"]
    print(f"\noverlap share: {TALLY['hits']} of {TALLY['steps']} steps ({100 * part:.1f} %), floor {100 * OVERLAP_FLOOR:.0f} %")
    assert part >= OVERLAP_FLOOR, f"the threads ran beside each other in {100 * part:.1f} % of the steps only"


def test_cold_round(lib, streams):
    """fresh contexts: both threads create them, load their sets and run every operation for the first time, step by step together (Y
    seven operations ahead of X, so that buffers of different calls are sized at once)"""
    prime(lib, ("BIG", "NARROW"))
    made = [None, None]
    crew = T.Crew(["X", "Y"])

    def body(slot, name, shift):
        def run(me):
            me.meet()
            w = made[slot] = Worker(lib, streams[slot])
            me.log = w.live.log
            with torch.cuda.stream(w.stream):
                me.meet()
                w.live.replace(name, "upload")
                for j in range(len(OPS)):
                    me.meet()
                    step(me, j, w.live, OPS[(j + shift) % len(OPS)])
                    me.meet()
                    second_look(w.live, OPS[(j + shift) % len(OPS)])
        return run
    try:
        crew.run({"X": body(0, "BIG", 0), "Y": body(1, "NARROW", 7)})
        print("\ncold round: the intervals intersect in %d of %d steps" % crew.overlap("X", "Y")[::-1])
    finally:
        close_all(made)


# ---- (b) two contexts of one shape ---------------------------------------------------------------------------------------------------
def swap_to(name):
    return lambda live: live.replace(name, "upload")


# X starts on BIG, Y on HIGHREG (330 genomes of 128 buckets each, p_aux 8, 40 queries: every key a context derives from the shape is
# the same in both, every rank, offset and group id of one is valid in the other).  A replacement on one side is followed by the cached
# passes of the OTHER side and then by its own: a key shared between contexts would now say "built" for arrays that hold the old set
SAME_SHAPE_PLAN = (
    [("smh_a-sig", "smh_a-sig"), ("query-sig", "query-sig"), ("query-index", "query-index"), ("pairs-signature_route", "pairs-signature_route")]
    + [("cards", swap_to("BIG")), ("smh_a-sig", "cards"), ("query-index", "cards"), ("cards", "smh_a-sig"), ("cards", "query-index"),
       ("cards", "query-sig"), ("cards", "pairs-signature_route")]
    + [(swap_to("HIGHREG"), "cards"), ("cards", "smh_a-sig"), ("cards", "query-index"), ("smh_a-sig", "cards"), ("query-index", "cards"),
       ("query-sig", "cards"), ("pairs-signature_route", "cards")]
    # ... and the calls that keep scratch in the context, both sides at once, ten times each: X holds HIGHREG now, Y holds BIG
    + [(o, o) for o in ("cluster", "cluster_greedy-priority", "merge_groups", "allpairs-topk", "hll_a-folded", "smh_a-hashjoin") for _ in range(10)]
    + [("cluster", "cluster_greedy-priority"), ("merge_groups", "cluster"), ("cluster_greedy-priority", "merge_groups")] * 4)


def test_same_shape_side_by_side(lib, streams):
    prime(lib, ("BIG", "HIGHREG"))
    workers = [Worker(lib, streams[2]), Worker(lib, streams[3])]
    try:
        for w, name in zip(workers, ("BIG", "HIGHREG")):
            with torch.cuda.stream(w.stream):
                w.live.replace(name, "upload")
        crew = T.Crew(["X", "Y"])
        in_step(crew, *workers, SAME_SHAPE_PLAN)
        print("\nsame shape: the intervals intersect in %d of %d steps" % crew.overlap("X", "Y")[::-1])
    finally:
        close_all(workers)


# ---- (c) random walks, four at once ------------------------------------------------------------------------------------------------------
WALK_STARTS = ("BIG", "NARROW", "WIDE", "HIGHREG")
CLUSTER_BLOCKS = (0, 1, 7)
VERTEX_BLOCKS = (0, 1, 7)


def walk(me, w, rng, steps, toggles, one_launch):
    """test_walk's steps on one context; toggles: this thread also sets the process-wide "cluster_blocks" and "vertex_blocks" between its
    steps.  one_launch:
    this thread may take the one-launch small pass (the operation smh_a-small_pass, the knob "small_pass").  Two such kernels fit the
    device together (512 block slots for twice 256 blocks); three need not, and the library then answers through the bounded wait of
    the kernel's grid barrier and the regular chain -- rightly, but the operations assert the route they asked for ("small_pass_used")"""
    live = w.live
    ops = sorted(o for o in R.OPS if one_launch or o != "smh_a-small_pass")
    knobs = sorted(k for k in KNOB_FLIPS if one_launch or k != "small_pass")
    for j in range(steps):
        me.go()
        if toggles:
            value = int(rng.choice(CLUSTER_BLOCKS))
            live.log.append(("cluster_blocks", value))
            live.sel.set_param("cluster_blocks", value)
            value = int(rng.choice(VERTEX_BLOCKS))
            live.log.append(("vertex_blocks", value))
            live.sel.set_param("vertex_blocks", value)
        kind = rng.choice(["db", "queries", "knob", "op", "op", "op"])
        if kind == "db":
            live.replace(str(rng.choice(R.NAMES)), str(rng.choice(["upload", "attach"])))
        elif kind == "queries":
            if live.S.p_hll == 14:
                live.queries(int(rng.choice([Q_CUT, live.S.n_q])), str(rng.choice(["upload", "attach"])))
        elif kind == "knob":
            name = str(rng.choice(knobs))
            value = int(rng.choice(KNOB_FLIPS[name]))
            live.log.append(("knob", name, value))
            live.knob(name, value)
        else:
            step(me, j, live, str(rng.choice(ops)))


@pytest.mark.parametrize("seed", [21, 22, 23, 24])
def test_walks_in_parallel(lib, streams, seed):
    prime(lib, R.NAMES)
    names = [f"walk{t}" for t in range(4)]
    made = [None] * 4
    crew = T.Crew(names)

    def body(t):
        def run(me):
            w = made[t] = Worker(lib, streams[t])
            me.log = w.live.log
            with torch.cuda.stream(w.stream):
                w.live.replace(WALK_STARTS[t], "upload")
                me.meet()
                walk(me, w, np.random.default_rng(100 * seed + t), 60, toggles=t == 0, one_launch=t < 2)
        return run
    try:
        crew.run({names[t]: body(t) for t in range(4)})
    finally:
        if not T.hip_failed() and made[0] is not None:
            made[0].live.sel.set_param("cluster_blocks", 0)
            made[0].live.sel.set_param("vertex_blocks", 0)
        close_all(made)


# ---- (d) the entries that take no context ------------------------------------------------------------------------------------------------
FREE_SETS = ("BIG", "NARROW", "HIGHREG")
FREE_ROUNDS = 3
FREE_VALUES = ("block_flags", "block_hist", "block_estimates", "block_matches", "block_fold", "block_synth", "block_build", "block_permute",
               "components", "greedy_reps", "edges", "keys", "perm", "forest_values", "block_forest", "linkage_dist", "block_linkage")


def test_free_standing_entries_in_parallel(lib, streams):
    """three threads, three sets, three streams: every entry three times in each thread, thread t starting t entries further down the list,
    so that calls of different entries -- each owning its scratch for the call -- and of the same entry meet"""
    names = list(E.ENTRIES)
    for set_name in FREE_SETS:                                       # (the models' values, computed here once: the threads read them)
        for attr in FREE_VALUES:
            assert len(R.leaves(getattr(lib[set_name], attr))) > 0
    crew = T.Crew(list(FREE_SETS))

    def body(t):
        S, st = lib[FREE_SETS[t]], streams[t]

        def run(me):
            with torch.cuda.stream(st):
                me.meet()
                for j in range(FREE_ROUNDS * len(names)):
                    me.go()
                    n = names[(j + t * 5) % len(names)]
                    me.log.append(n)
                    got, want = E.ENTRIES[n](S, st)
                    assert H.same(got, want), f"{n} on {S.name}, call {j}: {H.describe(got, want)}"
        return run
    crew.run({FREE_SETS[t]: body(t) for t in range(3)})


def test_first_calls_meet_in_a_fresh_process():
    """selhip_synth_generate, selhip_build_sketches and the split builder raise their kernels' LDS limit in a std::call_once at their first
    call.  In a fresh child process three threads make those first calls at once, and the first calls of selhip_linkage, on three streams
    and three inputs, and compare what they get with the generator's host twin, the builder's oracle and the linkage model (a child
    process: the program of this one is not replaced)"""
    child = Path(__file__).with_name("threads_child.py")
    r = subprocess.run([sys.executable, str(child)], capture_output=True, text=True, timeout=T.TIMEOUT)
    print(r.stdout[-2000:])
    assert r.returncode == 0 and "threads_child ok" in r.stdout, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"


# ---- (e) contexts that come and go beside work -----------------------------------------------------------------------------------------
CHURN = 30
CHURN_SETS = ("PREFIX", "NARROW", "ONE", "TRIMMED", "WIDE")
WORK_OPS = ("smh_a-sig", "query-index", "cluster", "merge_groups", "allpairs-topk-rounds", "none-fused", "matrix-jaccard", "pairs-direct_route",
            "hll_a-folded", "smh_a-hashjoin", "run_async-framed-finish", "query_matrix-containment",
            "linkage-average-jaccard")                    # (a hipMalloc and a hipFree of its own in every call, beside the churn's)


def test_context_churn_beside_work(lib, streams):
    """thirty short-lived contexts -- created, loaded, run, destroyed: hipMalloc and hipFree by the dozen, each hipFree a wait for the whole
    device -- on one thread, while two long-lived contexts work and are checked"""
    prime(lib, CHURN_SETS + ("BIG", "HIGHREG"))
    made = [None, None]
    crew = T.Crew(["churn", "work0", "work1"])
    done = []

    def churn(me):
        me.meet()
        for j in range(CHURN):
            me.go()
            w = Worker(lib, streams[2])
            me.log.append(("context", j))
            try:
                with torch.cuda.stream(w.stream):
                    w.live.replace(CHURN_SETS[j % len(CHURN_SETS)], "upload" if j % 2 else "attach")
                    for o in ("smh_a-sig", "cards", "cluster"):
                        step(me, (j, o), w.live, o)
                me.log.extend(w.live.log[-4:])
            finally:
                w.close()
        done.append(True)

    def work(slot, name):
        def run(me):
            w = made[slot] = Worker(lib, streams[slot])
            me.log = w.live.log
            with torch.cuda.stream(w.stream):
                w.live.replace(name, "upload")
                me.meet()
                j = 0
                while not done or j < len(WORK_OPS):                 # (at least once through the list, and for as long as contexts come and go)
                    me.go()
                    step(me, j, w.live, WORK_OPS[j % len(WORK_OPS)])
                    j += 1
        return run
    try:
        crew.run({"churn": churn, "work0": work(0, "BIG"), "work1": work(1, "HIGHREG")})
        print(f"\nchurn: {CHURN} contexts beside {len(made[0].live.log)} and {len(made[1].live.log)} log entries of work")
    finally:
        close_all(made)


# ---- (f) two one-launch small passes and a regular pass ----------------------------------------------------------------------------------
SMALL_PASSES = 50


def small_pass(me, j, live, used):
    """one smh_a pass with the one-launch small pass armed: records and statistics against the oracle's.  Whether the one launch ran is
    RECORDED (its grid barrier needs all of its blocks resident; beside another context that is not promised, and the library's bounded
    wait then hands the pass to the regular chain -- with the same answer)"""
    sel, S = live.sel, live.S
    live.log.append(("op", S.name, "small", j))
    live.settle()
    sel.set_param("small_pass", 1)                                    # (armed again: a wait that ran out switches it off for the context)
    got = me.timed(j, lambda: live.run(ALGO_SIG))
    used.append(sel.get_param("small_pass_used"))
    st, want = sel.stats(), R.stats_expected(S)
    assert H.same(got, S.smh_a), f"small pass {j} on {S.name} (one launch: {used[-1]}): {H.describe(got, S.smh_a)}"
    assert (st["evaluated"], st["survivors"], st["selected"]) == (want["evaluated"], want["survivors"], want["selected"]), (j, used[-1], st, want)
    if not used[-1]:
        assert st["candidates"] == want["candidates"], (j, st, want)


def test_small_passes_side_by_side(lib, streams):
    sets = {"small70": lib["PREFIX"], "small200": lib._cut("CUT200", 200), "regular": lib["BIG"]}
    assert (sets["small70"].n_d, sets["small200"].n_d) == (70, 200) and all(S.m == 128 for S in sets.values())
    for S in sets.values():
        R.expected(S, "smh_a-sig"), R.stats_expected(S)
    names = list(sets)
    made, used = [None] * 3, {n: [] for n in names}
    crew = T.Crew(names)

    def body(t):
        name = names[t]

        def run(me):
            w = made[t] = Worker(lib, streams[t], {"small_pass": 1} if name != "regular" else {"small_pass": 0})
            live = w.live
            me.log = live.log
            with torch.cuda.stream(w.stream):
                live.lib = {sets[name].name: sets[name]}              # (the set by its own name: CUT200 is not one of the library's)
                live.replace(sets[name].name, "upload", queries=False)
                me.meet()
                for j in range(SMALL_PASSES):
                    me.go()
                    if name == "regular":
                        step(me, j, live, "smh_a-sig")
                    else:
                        small_pass(me, j, live, used[name])
        return run
    try:
        crew.run({names[t]: body(t) for t in range(3)})
        print("\none-launch passes taken: " + ", ".join(f"{n} {sum(used[n])} of {len(used[n])}" for n in names[:2]))
    finally:
        close_all(made)


# ---- (g) whose error is whose ------------------------------------------------------------------------------------------------------------
X_TEXTS = ("no_such_knob", "are not in ascending order", "is not a finite value")


def test_errors_stay_with_their_thread(lib, streams):
    """X provokes refusals (an unknown parameter, an upload with unsorted cards) while Y works.  selhip_last_error(X's context) is X's
    message; selhip_last_error(NULL) is per thread: X's message on X's thread, never X's on Y's thread, which never failed;
    Y's answers are right, and X's context still answers as test_refused_upload_leaves_the_context_alone says it does"""
    prime(lib, ("PREFIX", "NARROW"))
    B, P = lib["BIG"], lib["PREFIX"]
    made = [None, None]
    crew = T.Crew(["X", "Y"])
    clib = hip_lib()
    rounds = 12
    said = []                                                         # what selhip_last_error(NULL) said on Y's thread (printed)
    y_ops = ("smh_a-sig", "cluster", "query-sig", "merge_groups")

    def refuse(live, j):
        if j % 2:
            with pytest.raises(SelhipError) as e:
                live.sel.set_param(f"no_such_knob_{j}", 1)
            return e.value, f"unknown parameter 'no_such_knob_{j}'"
        what, cards = list(bad_cards(B.D.cards).items())[(j // 2) % 3]
        with pytest.raises(SelhipError) as e:
            live.sel.upload(B.D.hll, B.D.aux, cards)
        return e.value, {"reversed": "are not in ascending order", "one NaN": "is not a finite value", "one negative": "is not a finite value"}[what]

    def x(me):
        w = made[0] = Worker(lib, streams[0])
        live = w.live
        me.log = live.log
        with torch.cuda.stream(w.stream):
            live.replace("PREFIX", "upload")
            live.aux("upload")
            check(live, "smh_a-sig")
            for j in range(rounds):
                me.meet()                                             # both act ...
                live.log.append(("refusal", j))
                err, text = refuse(live, j)
                assert err.code == R.BADARG and text in str(err), (j, str(err))
                me.meet()                                             # ... and both read, while neither calls
                mine, here = clib.selhip_last_error(live.sel._ctx).decode(), clib.selhip_last_error(None).decode()
                assert text in mine and text in here, (j, text, mine, here)
            assert live.sel.n == P.n_d and H.same(live.sel.fetch(), P.smh_a), "the results of the last pass are still there"
            for o in ("cards", "smh_a-sig", "query-sig", "query_matrix-containment", "hll_a-uploaded"):
                check(live, o)

    def y(me):
        w = made[1] = Worker(lib, streams[1])
        live = w.live
        me.log = live.log
        with torch.cuda.stream(w.stream):
            live.replace("NARROW", "upload")
            said.append(clib.selhip_last_error(None).decode())
            for j in range(rounds):
                me.meet()
                step(me, j, live, y_ops[j % len(y_ops)])
                me.meet()
                here, mine = clib.selhip_last_error(None).decode(), clib.selhip_last_error(live.sel._ctx).decode()
                said.append(here)
                for text in X_TEXTS:
                    assert text not in here, f"round {j}: selhip_last_error(NULL) on the thread that never failed says {here!r}"
                    assert text not in mine, f"round {j}: the clean context's message is {mine!r}"
    try:
        crew.run({"X": x, "Y": y})
        print(f"\nselhip_last_error(NULL) on the clean thread: {sorted(set(said))}")
    finally:
        close_all(made)
