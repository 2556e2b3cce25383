"""One live context, one database after another, of other shapes: the sets, the operations and their expected values for
tests/test_context_reuse_gpu.py, and the premises tests/test_context_reuse_host.py pins.  A plain helper module like tests/*_model.py;
host only.

A selhip_ctx keeps derived products between calls (bit planes, sparse lists, cached signatures, the query side's database signatures,
index and planes, folded auxiliary sketches), some forty device buffers that only grow, and sticky flags.  A replacement that leaves one
of them behind gives the PREVIOUS set's answer, or reads its bytes behind the new set's.  So every set here has its own answers, and the
sets are shaped so that the old bytes lie where a missing mask or a stale key would read them:

  BIG      330 genomes (padded arrays hold 384 columns), m 128, p_aux 8, 40 queries, clustered: the warm-up set
  PREFIX   the rows [0, 70) of BIG in rank order (pads to 128), BIG's queries: after BIG, the columns 70 .. 127 of every padded array are
           true partners of live rows -- the records of BIG with i < 70 <= k < 128 are what a missing pad mask would add
  NARROW   200 genomes, m 64, p_aux 6, another seed
  WIDE     130 genomes, m 512
  LOWP     150 genomes at p_hll 10, m 64 (precision_model): no bit planes; criterion none, HLL matrices and query passes are refused
  HIGHREG  BIG's shape, another seed, a few registers forged above 32: six bit planes and a sparse threshold (BIG has five)
  EMPTY, ONE   the rows [0, 0) and [0, 1) of BIG
  TRIMMED  the rows [0, 322) of BIG: it pads to 384 as BIG does.  The signature arrays are band-major with a row stride of the padded
           size, so after BIG -> PREFIX (stride 384 -> 128) the bytes in PREFIX's pad columns are BIG's, but of other bands and
           columns; after BIG -> TRIMMED the stride stays and column 322 of every band still holds genome 322 of BIG, a true partner
           of eight live rows: the one column a pad mask that is off by one admits

Expected values come from what the suite trusts already -- the oracle, tests/*_model.py, numpy -- through stream_harness.Sets, whose
shape is an argument; never from a second context.  Each is computed once per set."""
import functools

import numpy as np

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import PAIR_DTYPE

import bitplane_model
import cluster_model
import fold_model
import greedy_model
import merge_model
import precision_model
import sig_model
import stream_harness as H
from smh_matrix_model import match_counts

K = H.K
CUT = 70                                     # PREFIX = BIG's rows [0, CUT); pads to PAD
PAD = 128
TRIM = 322                                   # TRIMMED = BIG's rows [0, TRIM); pads to 384 like BIG
N_GROUPS = 9                                 # groups of the merge (ids -1 .. 8)
BADARG, STATE = -1, -5                       # SELHIP_E_BADARG, SELHIP_E_STATE
SEEDS = {"BIG": 0xC0DE0004, "NARROW": 0xC0DE0012, "WIDE": 0xC0DE0023, "HIGHREG": 0xC0DE0031, "LOWP": 211}
FORGED = (33, 36, 41, 47)                    # HIGHREG: register values written into a few genomes (above 32: a sixth plane)
EMPTY_REC = np.zeros(0, dtype=PAIR_DTYPE)


def forge_high(hll):
    """a few registers above 32 in every seventh genome, as bitplane_model's sets carry them: 12 per genome, far below the 128 entries of
    a sparse list (BIG's threshold is 12; tests/test_context_reuse_host.py pins that the two sets' differ)"""
    hll = hll.copy()
    rng = np.random.default_rng(0xF06E)
    for g in range(0, hll.shape[0], 7):
        hll[g, rng.choice(hll.shape[1], 12, replace=False)] = rng.choice(FORGED, 12)
    # ... and 140 registers of 13 or more in one genome: more than a sparse list holds, so the set's threshold moves up to 16
    at = rng.choice(hll.shape[1], 140, replace=False)
    hll[3, at] = np.maximum(hll[3, at], 13)
    return hll


class Set(H.Sets):
    """stream_harness.Sets plus what the reuse tests add: sets cut from another set's rows or built at another HLL precision, the merge by
    group, and which operations the shape admits"""

    @classmethod
    def of_rows(cls, oracle, name, D, Q, m, p_aux, tau, seed, p_hll=14):
        """a set from two sides that are in rank order already"""
        S = cls.__new__(cls)
        S.oracle, S.name, S.seed, S.p_hll = oracle, name, seed, p_hll
        S.n_d, S.n_q, S.m, S.p_aux, S.tau = len(D.cards), len(Q.cards), m, p_aux, tau
        S._finish(D, Q, np.random.default_rng(seed))
        return S

    @property
    def trivial(self):
        return self.n_d < 2

    @functools.cached_property
    def none(self):
        """the exhaustive loop from the oracle at the set's precision (test_exhaustive_host.flat_oracle_select at p_hll = 14)"""
        aux = np.zeros((self.n_d, 4), dtype=np.uint64)
        pairs, st = self.oracle.select(self.D.hll, aux, self.D.cards, self.tau, 1, 4, use_cb=True, criterion=0, p=self.p_hll)
        assert st["survivors"] == st["evaluated"]
        return H.records(pairs)

    @functools.cached_property
    def pair_list(self):
        return np.zeros((0, 2), dtype=np.int32) if self.trivial else super().pair_list

    @functools.cached_property
    def matrix_smh_matches(self):
        """of the set's OWN bucket rows (stream_harness attaches denser rows of their own; here the database stays what it is)"""
        return match_counts(self.D.aux, self.D.aux).astype(np.float64)

    @functools.cached_property
    def groups(self):
        """int32 [n_d]: ids -1 .. N_GROUPS - 1, about one genome in ten in no group"""
        return np.random.default_rng(self.seed + 9).integers(-1, N_GROUPS, self.n_d).astype(np.int32)

    @functools.cached_property
    def merged(self):
        """what Selector.merge(groups, N_GROUPS, to_host=True) returns with the uploaded auxiliary sketches in place"""
        D = self.D
        res = merge_model.merge_all(D.hll, D.aux, D.aux_hll, self.groups, N_GROUPS)
        return {"hll": res["hll"], "aux": res["smh"], "aux_hll": res["aux_hll"], "sizes": res["sizes"],
                "cards": np.where(res["sizes"] > 0, self.oracle.cards(res["hll"], self.p_hll), 0.0)}

    @functools.cached_property
    def cards(self):
        return self.D.cards

    @functools.cached_property
    def stats_smh_a(self):
        """the oracle's statistics of the smh_a pass: evaluated pairs and survivors of stage 1"""
        D = self.D
        return self.oracle.select(D.hll, D.aux, D.cards, self.tau, self.r, self.b, use_cb=True, p=self.p_hll)[1]

    @functools.cached_property
    def candidates_smh_a(self):
        """the pairs inside the CB windows with at least one band signature equal: what the signature join hands to the verification"""
        lo, hi = sig_model.allpairs_windows(self.D.cards, self.tau, True)
        return sig_model.expected_candidates(sig_model.band_sigs(self.D.aux, self.r, self.b), lo, hi)

    @functools.cached_property
    def planes(self):
        return bitplane_model.planes(bitplane_model.khi(self.D.hll)) if self.p_hll == 14 and self.n_d else 0

    @functools.cached_property
    def sparse_t(self):
        return bitplane_model.sparse_t(self.D.hll, bitplane_model.khi(self.D.hll)) if self.p_hll == 14 and self.n_d else 0

    def hist_image(self, knobs):
        """what get_param("hist_image") says behind an all-pairs smh_a pass of the set that went through stage 2a: 1 where the set holds
        the clamped four-plane image -- its sparse threshold is 4, 8 or 12 -- and the knobs let the pass read it ("hist_image" and
        "hist_sparse" not 0, bit planes kept), else 0.  knobs: the context's, {name: value}; a knob that is not there is automatic"""
        allowed = all(knobs.get(k, -1) != 0 for k in ("hist_image", "hist_sparse", "hist_algo"))
        return int(allowed and self.sparse_t in (4, 8, 12))


# operation -> (the attribute of Set that is its expected value, kind): "list" = all-pairs or pair-list records, "qlist" = query records,
# "matrix", "value".  One per entry of stream_harness.CONTEXT_CASES but the stream-specific ones (NOT_HERE), plus the three below the line
OPS = {k: v for k, v in H.CONTEXT_CASES.items()}
NOT_HERE = {
    "two_contexts": "two contexts on two streams: nothing of ONE context's life",
    "switch-sig_cache": "moves a context between streams", "switch-query_index": "moves a context between streams",
    "grown_lists": "needs lists that are still small: a fresh context; here the flavour init_cap lets the SECOND set grow them",
}
for _k in NOT_HERE:
    del OPS[_k]
for _k in ("query-sig", "query-stream", "query-index", "query-topk"):
    OPS[_k] = (OPS[_k][0], "qlist")
OPS.update({"merge_groups": ("merged", "value"), "cards": ("cards", "value")})    # ("fold_aux_hll, then hll_a" is hll_a-folded)
# (the linkage of an HLL measure is refused as its matrix is; the one over smh_jaccard reads the bucket rows alone and always runs)
LINKAGE_OPS = tuple(H.LINKAGE_CASES)
HLL_LINKAGES = {k for k, v in H.LINKAGE_CASES.items() if v[0] != "smh_jaccard"}
P14_ONLY = {"none-list_route", "none-fused", "matrix-jaccard", "query-sig", "query-stream", "query-index", "query-topk",
            "query_matrix-containment"} | HLL_LINKAGES
NEEDS_PLANES = {"none-list_route", "none-fused", "matrix-jaccard", "query_matrix-containment"} | HLL_LINKAGES
QUERY_OPS = {k for k, v in OPS.items() if v[1] == "qlist"} | {"query_matrix-containment"}


def refusal(S, op, bit_planes=True):
    """the documented refusal code of an operation the set's shape does not admit (include/selection_hip.h, selhip_ctx_upload: criterion
    none, HLL matrices and query passes need p_hll = 14 -- the queries are refused when they are loaded), None where it runs.
    bit_planes False: the context keeps none ("hist_algo" 0), and criterion none and the HLL matrices of a set that is not empty need
    them"""
    if S.p_hll != 14 and op in P14_ONLY:
        return BADARG
    return BADARG if not bit_planes and S.n_d > 0 and op in NEEDS_PLANES else None


def expected(S, op, bit_planes=True):
    """the expected value of an operation on a set: a refusal code, or the value"""
    code = refusal(S, op, bit_planes)
    if code is not None:
        return code
    attr, kind = OPS[op]
    n = S.n_d
    if S.trivial:
        # no pair in the set: every list of pairs of the database is empty; the oracle and the models are not asked
        if kind == "list":
            return EMPTY_REC
        if op == "matrix-jaccard":
            return np.ones((n, n))
        if op == "query_matrix-containment" and n == 0:
            return np.zeros((S.n_q, 0))
        if op == "cluster":
            return cluster_model.clusters(np.zeros((0, 2), dtype=np.int64), n, "max_degree")
        if op == "cluster_greedy-priority":
            res = greedy_model.clusters(EMPTY_REC, n, rule="priority", priority=S.prio.astype(np.int64))
            res.pop("rounds_bound")
            return res
        if op == "forest":
            return {"edges": EMPTY_REC, "labels": np.arange(n, dtype=np.int32)}
        if op in H.LINKAGE_CASES:                                 # (no launch: one slot is scanned once and has no neighbour)
            return {"merges": EMPTY_REC, "sizes": np.zeros(0, dtype=np.int32), "rounds": n}
    return getattr(S, attr)


def stats_expected(S):
    """{"evaluated", "survivors", "selected", "candidates"} of the smh_a signature pass of a set: the oracle's counts and sig_model's"""
    if S.trivial:
        return {"evaluated": 0, "survivors": 0, "selected": 0, "candidates": 0}
    st = S.stats_smh_a
    return {"evaluated": st["evaluated"], "survivors": st["survivors"], "selected": len(S.smh_a), "candidates": S.candidates_smh_a}


def leaves(value):
    """the arrays of an expected value"""
    if isinstance(value, dict):
        return [np.asarray(v) for _, v in sorted(value.items()) if v is not None]
    return [np.asarray(value)]


# ---- the sets -----------------------------------------------------------------------------------------------------------------------
NAMES = ("BIG", "PREFIX", "NARROW", "WIDE", "LOWP", "HIGHREG", "EMPTY", "ONE", "TRIMMED")
TRANSITIONS = (("BIG", "PREFIX"), ("PREFIX", "BIG"), ("BIG", "NARROW"), ("NARROW", "WIDE"), ("BIG", "LOWP"), ("LOWP", "BIG"),
               ("HIGHREG", "BIG"), ("BIG", "HIGHREG"), ("BIG", "EMPTY", "PREFIX"), ("BIG", "ONE", "BIG"), ("BIG", "TRIMMED"),
               ("BIG", "HIGHREG", "BIG"))              # (the clamped image on, off -- HIGHREG's threshold is 16 --, and on again)
# (X, Y, operation) -> reason: the steps X -> Y on which an operation's expected values may be EQUAL, so that the step cannot tell a stale
# answer from the right one.  No operation may stand here for more than two steps (tests/test_context_reuse_host.py)
SAME_ANSWER = {}


def steps():
    """every step X -> Y of the transitions, once"""
    out = []
    for t in TRANSITIONS:
        for x, y in zip(t, t[1:]):
            if (x, y) not in out:
                out.append((x, y))
    return out


class Library:
    """the sets by name, built on first use and kept"""

    def __init__(self, oracle):
        self.oracle, self._sets = oracle, {}

    def __getitem__(self, name):
        if name not in self._sets:
            self._sets[name] = self._make(name)
        return self._sets[name]

    def _cut(self, name, rows):
        B = self["BIG"]
        D = H.Side(*(np.ascontiguousarray(a[:rows]) for a in B.D))
        return Set.of_rows(self.oracle, name, D, B.Q, B.m, B.p_aux, B.tau, B.seed + 1000 + rows)

    def _make(self, name):
        o = self.oracle
        if name == "BIG":
            return Set(o, name, n_d=330, n_q=40, m=128, p_aux=8, seed=SEEDS[name])
        if name == "HIGHREG":
            return Set(o, name, n_d=330, n_q=40, m=128, p_aux=8, seed=SEEDS[name], forge=forge_high)
        if name == "NARROW":
            return Set(o, name, n_d=200, n_q=40, m=64, p_aux=6, seed=SEEDS[name])
        if name == "WIDE":
            return Set(o, name, n_d=130, n_q=40, m=512, p_aux=8, seed=SEEDS[name])
        if name == "LOWP":
            hll, aux, cards, aux_hll = precision_model.sketch_set_aux(10, 150, 64, SEEDS[name], 6)
            # (the queries are p = 14 rows of m = 64: what a caller would hand over, and what the library must refuse)
            return Set.of_rows(o, name, H.Side(hll, aux, cards, aux_hll), self["NARROW"].Q, 64, 6, H.TAU, SEEDS[name], p_hll=10)
        return self._cut(name, {"PREFIX": CUT, "EMPTY": 0, "ONE": 1, "TRIMMED": TRIM}[name])


def pad_partners(rec, cut=CUT, pad=PAD):
    """the records of a list with i < cut <= k < pad: what a join that forgets the pad mask would add to the prefix set's answer"""
    return rec[(rec["i"] < cut) & (rec["k"] >= cut) & (rec["k"] < pad)]
