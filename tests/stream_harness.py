"""Every entry point on a caller's NON-BLOCKING stream: the data, the expected values and the three-run engine of
tests/test_streams_gpu.py (and the premises tests/test_streams_host.py pins).  A plain helper module like tests/*_model.py.

The library promises that all work of a context runs on the stream of selhip_ctx_set_stream and that the block launchers are
asynchronous on the stream they are given (include/selection_hip.h sections 2 - 4b).  On the null stream neither promise can fail
visibly: the null stream waits for every blocking stream and they for it.  A torch pool stream is non-blocking; there a launch, a
memset or a sort left on another stream, or a missing event wait between the context's stream and its second chunk lane, is a silent
race.  Nothing here waits for luck -- every case is arranged so that a wrong stream gives a wrong answer:

  two data sets of one shape, REAL and DECOY (two seeds of the synthetic generator, each side in rank order), with different answers;
  a context is attached to ONE set of device tensors, and the sets are copied into them;

  warm-up   the case on the decoy, fully synchronised: every buffer is sized, every cached product is the decoy's.
  run A     the caller's stream s is LATE: on s a delay (torch.cuda._sleep), then the copies of the real set into the attached
            tensors, `not s.query()`, then the calls on s, outputs read through s.  Whatever the library reads on another stream
            runs ahead of the delay and sees the decoy.  attach takes snapshots (bit planes, cardinalities) and waits for the stream,
            so behind it Env.stall() puts a SECOND delay on s, in front of the pass proper: a kernel of the pass on another stream then
            runs ahead of its predecessors on s and reads the decoy's intermediates of the warm-up.  Inputs that no attach
            snapshots (a pair list, the priorities) and the poison of caller-owned outputs are written behind that second delay.
            An entry documented as asynchronous must leave `s.query()` false when it returns.
  restore   the case on the decoy again, synchronised and timed (the sizing of run B's delay).
  run B     the NULL stream is blocked by a delay that outlasts the call; the real set is copied and the case runs on s, outputs
            read through s only.  Work put on the null stream has not run, so its effect is missing and the decoy's is there
            instead; afterwards `torch.cuda.default_stream().query()` must still be false -- a synchronous null-stream copy or a
            device-wide wait (hipFree, hipDeviceSynchronize) inside a warmed call ends the delay first.

            The hierarchy entries that free their scratch before they return (ANSWER_UNDER_BLOCKED_NULL) get this run for the answer
            alone, under a fixed delay that their hipFree waits out.

The delays only size things (each at most 2 s): the conditions are the query() assertions and the answers.
The linkage cases' expected values take 0.3 s of model time per set at the most (the SuperMinHash case under single linkage, 300 rounds
of one pair on its plateau), so that case stays single linkage.
Expected values come from what the suite trusts already: the oracle, tests/*_model.py, numpy."""
import functools
import tempfile
import time
from collections import namedtuple
from pathlib import Path

import numpy as np

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import FP_FMA, PAIR_DTYPE, SynthConfig

import cluster_model
import containment_model
import fold_model
import forest_model
import greedy_model
import linkage_model
import smhv_model
import topk_rounds_model
import smh_matrix_model
from smh_matrix_model import match_counts
from test_exhaustive_host import flat_oracle_select

N_D, N_Q, M, TAU, P_AUX, K = 300, 40, 128, 0.5, 8, 3
C_MIN = 116                                  # smh_c: at least 116 of the 128 buckets equal (about half of the cluster pairs)
ROUND_ROWS = 64                              # rows per round of the all-pairs top-k in row rounds: 5 rounds over 300 rows
N_LIST = 400                                 # entries of the pair list
N_BLOCK = 200                                # pairs handed to the block launchers
N_EDGES = 300                                # edges handed to components() and greedy_representatives()
SEEDS = {"real": 0x57A10001, "decoy": 0x57A10002}
DELAY_MS = 100.0                             # the delays of run A; far above the host's enqueue time, far below the 2 s bound
MAX_DELAY_MS = 2000.0

Side = namedtuple("Side", "hll aux cards aux_hll")


def banding():
    return pkg.banding(M, TAU)


def records(pairs):
    """oracle records -> PAIR_DTYPE"""
    out = np.zeros(len(pairs), dtype=PAIR_DTYPE)
    out["i"], out["k"] = pairs["i"], pairs["k"]
    out["jaccard"] = pairs["jacc"] if "jacc" in pairs.dtype.names else pairs["jaccard"]
    return out


def by_ik(rec):
    return rec[np.lexsort((rec["k"], rec["i"]))]


def distance_of(similarity):
    """the distance matrix selhip_ctx_linkage builds from a similarity matrix: 1 - v in float64, a NaN cell (two empty sketches) 1.0"""
    d = 1.0 - np.asarray(similarity, dtype=np.float64)
    d[np.isnan(d)] = 1.0
    return d


# the context cases of selhip_ctx_linkage: id -> (measure, method, capped at Sets.linkage_cap)
LINKAGE_CASES = {"linkage-average-jaccard": ("jaccard", "average", False), "linkage-single-smh_jaccard": ("smh_jaccard", "single", False),
                 "linkage-complete-max_containment-capped": ("max_containment", "complete", True)}
# the layouts selhip_linkage is handed its matrix in: tag -> (ld - n, offset of the base behind a 16-byte boundary in doubles).  An even ld
# on a 16-byte base takes lk_scan_kernel<true> (16-byte loads), anything else lk_scan_kernel<false>
LINKAGE_LAYOUTS = {"wide": (0, 0), "narrow": (3, 1)}


class Sets:
    """one seed's data and every expected value of the cases, each computed once (host only).  The shape is an argument (the defaults
    are the constants above, which tests/test_streams_*.py use): n_d database and n_q query genomes of m buckets, auxiliary sketches
    of precision p_aux, the threshold tau, the generator's seed (default SEEDS[name]) and forge(hll) -> hll, a step that rewrites
    registers of the generated sketches before anything is derived from them (tests/context_reuse_model.py)"""

    p_hll = 14

    def __init__(self, oracle, name, n_d=N_D, n_q=N_Q, m=M, p_aux=P_AUX, tau=TAU, seed=None, forge=None):
        self.oracle, self.name, self.seed = oracle, name, SEEDS[name] if seed is None else seed
        self.n_d, self.n_q, self.m, self.p_aux, self.tau = n_d, n_q, m, p_aux, tau
        cfg = SynthConfig("streams-" + name, n_d + n_q, m, tau, self.seed, p_aux=p_aux, mode=1, n_sh_lo=8_000, n_sh_hi=60_000)
        hll, aux, aux_hll = pkg.synth_host(cfg)
        if forge is not None:
            hll = forge(hll)
        rng = np.random.default_rng(self.seed)
        pick = np.zeros(n_d + n_q, dtype=bool)
        pick[rng.choice(n_d + n_q, n_q, replace=False)] = True
        self._finish(self._side(hll[~pick], aux[~pick], aux_hll[~pick]), self._side(hll[pick], aux[pick], aux_hll[pick]), rng)

    def _finish(self, D, Q, rng):
        """the two sides in rank order, and what is drawn for them"""
        self.D, self.Q = D, Q
        self.r, self.b = pkg.banding(self.m, self.tau)
        self.c_min = C_MIN * self.m // M
        # what no attach snapshots: the priorities of the greedy clusters, the positions of the query matrix
        self.prio = rng.integers(0, 1 << 20, self.n_d).astype(np.int32)
        self.row_pos = rng.permutation(self.n_q).astype(np.int32)
        self.col_pos = rng.permutation(self.n_d).astype(np.int32)

    def _side(self, hll, aux, aux_hll):
        cards = self.oracle.cards(hll)
        perm = pkg.sort_by_card(cards)
        return Side(hll[perm], aux[perm], cards[perm], aux_hll[perm])

    def _select(self, crit, aux_hll=None):
        D = self.D
        return records(self.oracle.select(D.hll, D.aux, D.cards, self.tau, self.r, self.b, use_cb=True, criterion=crit,
                                          aux_hll=D.aux_hll if aux_hll is None else aux_hll, p=self.p_hll, p_aux=self.p_aux)[0])

    # -- all-pairs passes ---------------------------------------------------------------------------
    @functools.cached_property
    def smh_a(self):
        return self._select(pkg.CRIT_SMH_A)

    @functools.cached_property
    def hll_a(self):
        return self._select(pkg.CRIT_HLL_A)

    @functools.cached_property
    def hll_a_folded(self):
        return self._select(pkg.CRIT_HLL_A, aux_hll=fold_model.fold(self.D.hll, self.p_aux))

    @functools.cached_property
    def two_stage(self):
        return self._select(pkg.CRIT_HLL_A_SMH_A)

    @functools.cached_property
    def none(self):
        return flat_oracle_select(self.oracle, self.D.hll, self.D.cards, self.tau, True, FP_FMA)[0]

    @functools.cached_property
    def counts(self):
        return match_counts(self.D.aux, self.D.aux)

    @functools.cached_property
    def smh_c(self):
        return self.none[self.counts[self.none["i"], self.none["k"]] >= self.c_min]

    @functools.cached_property
    def smh_c_v(self):
        return by_ik(smhv_model.expected(self.D.aux, self.D.cards, self.tau, use_cb=True, c_min=self.c_min, counts=self.counts)[0])

    @functools.cached_property
    def topk(self):
        return topk_rounds_model.ranked_cut(topk_rounds_model.both_members(self.smh_a), K)

    @functools.cached_property
    def topk_rounds(self):
        return topk_rounds_model.ranked_cut(topk_rounds_model.both_members(self.smh_c_v), K)

    # -- query passes -------------------------------------------------------------------------------
    @functools.cached_property
    def query(self):
        """the cross pairs of the all-pairs oracle over Q u D as {query rank, database rank, J}, sorted by (i, k)"""
        Q, D = self.Q, self.D
        hll, aux, cards = np.concatenate([Q.hll, D.hll]), np.concatenate([Q.aux, D.aux]), np.concatenate([Q.cards, D.cards])
        perm = pkg.sort_by_card(cards)
        pairs = self.oracle.select(hll[perm], aux[perm], cards[perm], self.tau, self.r, self.b, use_cb=True)[0]
        g1, g2 = perm[pairs["i"]], perm[pairs["k"]]
        cross = (g1 < self.n_q) != (g2 < self.n_q)
        out = np.zeros(int(cross.sum()), dtype=PAIR_DTYPE)
        out["i"] = np.where(g1 < self.n_q, g1, g2)[cross]
        out["k"] = np.where(g1 < self.n_q, g2, g1)[cross] - self.n_q
        out["jaccard"] = pairs["jacc"][cross]
        return by_ik(out)

    @functools.cached_property
    def query_topk(self):
        return topk_rounds_model.ranked_cut(self.query, K)

    # -- pair-list passes ---------------------------------------------------------------------------
    @functools.cached_property
    def pair_list(self):
        """int32 [N_LIST, 2]: half of it selected pairs of this set (either order, a few twice), half random valid pairs"""
        rng = np.random.default_rng(self.seed + 1)
        S = self.none[rng.choice(len(self.none), N_LIST // 2)]
        hit = np.stack([S["i"], S["k"]], axis=1)
        flip = rng.random(len(hit)) < 0.5
        hit[flip] = hit[flip][:, ::-1]
        x = rng.integers(0, self.n_d, N_LIST - len(hit))
        y = (x + rng.integers(1, self.n_d, len(x))) % self.n_d
        return rng.permutation(np.concatenate([hit, np.stack([x, y], axis=1)])).astype(np.int32)

    @functools.cached_property
    def listed(self):
        """one record {min, max, J} per entry of the list whose pair the all-pairs smh_a pass selects, sorted by (i, k)"""
        S = {(int(r["i"]), int(r["k"])): r["jaccard"] for r in self.smh_a}
        lo, hi = self.pair_list.min(axis=1), self.pair_list.max(axis=1)
        hits = [(int(a), int(b), S[(int(a), int(b))]) for a, b in zip(lo, hi) if (int(a), int(b)) in S]
        return by_ik(np.array(hits, dtype=PAIR_DTYPE))

    # -- dense matrices -----------------------------------------------------------------------------
    @functools.cached_property
    def matrix_jaccard(self):
        """J of every pair from the oracle's exhaustive loop without a threshold, mirrored, 1.0 on the diagonal"""
        rec = flat_oracle_select(self.oracle, self.D.hll, self.D.cards, -np.inf, False, FP_FMA)[0]
        assert len(rec) == self.n_d * (self.n_d - 1) // 2                       # (no empty sketch in the set: every pair has a record)
        Jm = np.ones((self.n_d, self.n_d))
        Jm[rec["i"], rec["k"]] = rec["jaccard"]
        Jm[rec["k"], rec["i"]] = rec["jaccard"]
        return Jm

    @functools.cached_property
    def dense_aux(self):
        """bucket rows for the SuperMinHash matrix: the generator's unrelated genomes share no bucket, so that both sets' matrices would
        be zero nearly everywhere; these rows share a random part of a base row each (smh_matrix_model.random_rows)"""
        return smh_matrix_model.random_rows(self.n_d, self.m, self.seed + 7)

    @functools.cached_property
    def matrix_smh_matches(self):
        return match_counts(self.dense_aux, self.dense_aux).astype(np.float64)

    @functools.cached_property
    def query_matrix_containment(self):
        """containment of every query in every database genome, scattered to out[row_pos[q], col_pos[d]]"""
        U = containment_model.union_matrix(self.oracle, self.Q.hll, self.D.hll)
        V = containment_model.matrix_model(U, self.Q.cards, self.D.cards, "containment", False)
        out = np.empty_like(V)
        out[np.ix_(self.row_pos, self.col_pos)] = V
        return out

    @functools.cached_property
    def matrix_smh_jaccard(self):
        """the bucket-match counts / m in float64 (smh_matrix_model.expected): of the rows matrix_smh_matches counts"""
        return self.matrix_smh_matches / np.float64(self.m)

    @functools.cached_property
    def matrix_max_containment(self):
        """I / min(e_row, e_col) of every pair from the oracle's union estimates (containment_model), 1.0 on the diagonal"""
        U = containment_model.union_matrix(self.oracle, self.D.hll, self.D.hll, symmetric=True)
        return containment_model.matrix_model(U, self.D.cards, self.D.cards, "max_containment", True)

    # -- hierarchies ----------------------------------------------------------------------------------
    @functools.cached_property
    def forest(self):
        """the maximum spanning forest of the smh_a pass's records: forest_model.kruskal, the definition"""
        edges, labels = forest_model.kruskal(forest_model.records_of_pass(self.smh_a), self.n_d)
        return {"edges": forest_model.as_records(edges), "labels": np.asarray(labels, dtype=np.int32)}

    def _linkage(self, similarity, method, max_height=np.inf):
        """{"merges", "sizes", "rounds"} of linkage_model on the distance selhip_ctx_linkage derives: 1 - v, a NaN cell 1.0"""
        res = linkage_model.linkage_model(distance_of(similarity), method, max_height)
        return {"merges": res["merges"], "sizes": res["sizes"], "rounds": res["rounds"]}

    @functools.cached_property
    def linkage_average_jaccard(self):
        return self._linkage(self.matrix_jaccard, "average")

    @functools.cached_property
    def linkage_single_smh_jaccard(self):
        return self._linkage(self.matrix_smh_jaccard, "single")

    @functools.cached_property
    def linkage_complete_max_containment(self):
        """the whole tree: what the cap of the capped case is read from"""
        return self._linkage(self.matrix_max_containment, "complete")

    @functools.cached_property
    def linkage_cap(self):
        """max_height of the capped case: the median height of the whole tree"""
        h = np.sort(self.linkage_complete_max_containment["merges"]["jaccard"])
        return float(h[len(h) // 2])

    @functools.cached_property
    def linkage_complete_max_containment_capped(self):
        return self._linkage(self.matrix_max_containment, "complete", self.linkage_cap)

    # -- clusters -----------------------------------------------------------------------------------
    @functools.cached_property
    def clusters(self):
        return cluster_model.clusters(cluster_model.record_edges(self.smh_a), self.n_d, "max_degree")

    @functools.cached_property
    def greedy(self):
        res = greedy_model.clusters(self.smh_a, self.n_d, rule="priority", priority=self.prio.astype(np.int64))
        res.pop("rounds_bound")
        return res

    # -- block launchers and Python helpers -----------------------------------------------------------
    @functools.cached_property
    def block_pairs(self):
        """int32 [N_BLOCK, 2]: a quarter of it pairs of one cluster, the rest random"""
        rng = np.random.default_rng(self.seed + 2)
        p = np.stack([rng.integers(0, self.n_d, N_BLOCK), rng.integers(0, self.n_d, N_BLOCK)], axis=1)
        S = self.none[rng.choice(len(self.none), N_BLOCK // 4)]
        p[: len(S), 0], p[: len(S), 1] = S["k"], S["i"]
        return p.astype(np.int32)

    @functools.cached_property
    def block_flags(self):
        a, p = self.D.aux, self.block_pairs
        return np.array([self.oracle.smh_a(a[x], a[y], self.r, self.b) for x, y in p], dtype=np.uint8)

    @functools.cached_property
    def block_hist(self):
        h, p = self.D.hll, self.block_pairs
        return np.stack([self.oracle.union_hist(h[x], h[y]) for x, y in p])

    @functools.cached_property
    def block_estimates(self):
        return np.array([self.oracle.estimate(c, 14, FP_FMA) for c in self.block_hist])

    @functools.cached_property
    def block_matches(self):
        a, p = self.D.aux, self.block_pairs
        return (a[p[:, 0]] == a[p[:, 1]]).sum(-1).astype(np.int32)

    @functools.cached_property
    def block_fold(self):
        return fold_model.fold(self.D.hll[:64], self.p_aux)

    @functools.cached_property
    def synth_cfg(self):
        return SynthConfig("streams-gen-" + self.name, 48, self.m, self.tau, self.seed + 3, p_aux=self.p_aux, mode=1, n_sh_lo=2_000, n_sh_hi=30_000)

    @functools.cached_property
    def block_synth(self):
        hll, aux, aux_hll = pkg.synth_host(self.synth_cfg)
        return {"hll": hll, "aux": aux, "aux_hll": aux_hll}

    @functools.cached_property
    def build_codes(self):
        """(codes u8, offsets i64) of three random genomes of 3 000, 1 500 and 4 500 bases with a few window resets"""
        rng = np.random.default_rng(self.seed + 4)
        lens = (3000, 1500, 4500)
        codes = rng.integers(0, 4, sum(lens)).astype(np.uint8)
        codes[rng.choice(len(codes), 12, replace=False)] = 4
        return codes, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)

    @functools.cached_property
    def block_build(self):
        """the oracle's sketches (HLL p = 14, SuperMinHash m = 64, auxiliary HLL p = 8) of FASTA files written from build_codes"""
        import oracle_py
        bo = oracle_py.BuildOracle()
        codes, off = self.build_codes
        out = {"hll": [], "smh": [], "aux_hll": []}
        with tempfile.TemporaryDirectory() as tmp:
            for g in range(len(off) - 1):
                path = Path(tmp) / f"g{g}.fna"
                seq = "".join("ACGTN"[c] for c in codes[off[g]:off[g + 1]])
                path.write_text(">g%d\n%s\n" % (g, seq))
                hll, aux, smh, _ = bo.sketch(path, m=64, p_aux=self.p_aux)
                out["hll"].append(hll), out["smh"].append(smh), out["aux_hll"].append(aux)
        return {k: np.stack(v) for k, v in out.items()}

    @functools.cached_property
    def perm(self):
        return np.random.default_rng(self.seed + 5).permutation(self.n_d).astype(np.int32)

    @functools.cached_property
    def block_permute(self):
        return self.D.aux[self.perm]

    def permute_data(self, case_id):
        """{"src": u8 [rows, row_bytes], "perm": i32 [rows], "want": src[perm]} of one of PERMUTE_SHAPES"""
        rows, row_bytes, _ = PERMUTE_SHAPES[case_id]
        rng = np.random.default_rng(self.seed + 100 + sorted(PERMUTE_SHAPES).index(case_id))
        src = rng.integers(0, 256, (rows, row_bytes)).astype(np.uint8)
        perm = rng.permutation(rows).astype(np.int32)
        return {"src": src, "perm": perm, "want": src[perm]}

    @functools.cached_property
    def edges(self):
        """the edge list of the Python helpers: N_EDGES selected pairs of the smh_c pass (clusters cut into pieces)"""
        S = self.smh_c[np.random.default_rng(self.seed + 8).choice(len(self.smh_c), N_EDGES, replace=False)]
        return np.stack([S["i"], S["k"]], axis=1).astype(np.int32)

    @functools.cached_property
    def components(self):
        return cluster_model.labels(self.edges, self.n_d).astype(np.int32)

    @functools.cached_property
    def forest_values(self):
        """the values of the edges handed to selhip_spanning_forest: fifty levels, so that many edges tie"""
        return np.random.default_rng(self.seed + 11).integers(0, 50, len(self.edges)) / 50.0

    @functools.cached_property
    def block_forest(self):
        edges, labels = forest_model.kruskal(forest_model.records_of(self.edges, self.forest_values), self.n_d)
        return {"edges": forest_model.as_records(edges), "labels": np.asarray(labels, dtype=np.int32)}

    @functools.cached_property
    def linkage_dist(self):
        """the caller's distance matrix of selhip_linkage: N_D x N_D uniform numbers from the set's seed (whatever the set's own size:
        the entry takes no context and no sketches); only the strict upper triangle counts"""
        return np.random.default_rng(self.seed + 12).random((N_D, N_D))

    @functools.cached_property
    def block_linkage(self):
        """average linkage of linkage_dist, once per layout of LINKAGE_LAYOUTS: the layouts take the two instantiations of the row
        scan and must give the same tree"""
        res = linkage_model.linkage_model(self.linkage_dist, "average")
        return {f"{k}-{tag}": res[k] for tag in LINKAGE_LAYOUTS for k in ("merges", "sizes", "rounds")}

    @functools.cached_property
    def keys(self):
        return np.random.default_rng(self.seed + 6).integers(0, 1 << 40, self.n_d).astype(np.uint64)

    @functools.cached_property
    def greedy_reps(self):
        return greedy_model.representatives(self.edges, self.n_d, [int(k) for k in self.keys]).astype(np.uint8)


# case id -> (the attribute of Sets that is its expected value, kind): kind "list" = a record list (at least 20 records, the two sets'
# differ), "matrix" = a dense matrix (the sets' differ in more than half the cells), "value" = anything else (non-empty, the sets' differ).
# tests/test_streams_host.py pins those premises for every id, tests/test_streams_gpu.py runs every id.
CONTEXT_CASES = {
    "smh_a-sig": ("smh_a", "list"), "smh_a-stream": ("smh_a", "list"), "smh_a-hashjoin": ("smh_a", "list"),
    "smh_a-chunks2": ("smh_a", "list"), "smh_a-small_pass": ("smh_a", "list"),
    "hll_a-uploaded": ("hll_a", "list"), "hll_a-folded": ("hll_a_folded", "list"), "hll_a+smh_a": ("two_stage", "list"),
    "none-list_route": ("none", "list"), "none-fused": ("none", "list"),
    "smh_c": ("smh_c", "list"), "smh_c-smh_estimator": ("smh_c_v", "list"),
    "grown_lists": ("smh_a", "list"),
    "run_async-framed-finish": ("smh_a", "list"),
    "query-sig": ("query", "list"), "query-stream": ("query", "list"), "query-index": ("query", "list"),
    "query-topk": ("query_topk", "list"),
    "allpairs-topk": ("topk", "list"), "allpairs-topk-rounds": ("topk_rounds", "list"),
    "pairs-signature_route": ("listed", "list"), "pairs-direct_route": ("listed", "list"),
    "matrix-jaccard": ("matrix_jaccard", "matrix"), "matrix-smh_matches": ("matrix_smh_matches", "matrix"),
    "query_matrix-containment": ("query_matrix_containment", "matrix"),
    "cluster": ("clusters", "value"), "cluster_greedy-priority": ("greedy", "value"),
    "forest": ("forest", "value"),
    "linkage-average-jaccard": ("linkage_average_jaccard", "value"), "linkage-single-smh_jaccard": ("linkage_single_smh_jaccard", "value"),
    "linkage-complete-max_containment-capped": ("linkage_complete_max_containment_capped", "value"),
    "two_contexts": ("smh_a", "list"),                      # (the second context runs smh_c: checked as "smh_c")
    "switch-sig_cache": ("smh_a", "list"), "switch-query_index": ("query", "list"),
}
BLOCK_CASES = {
    "selhip_smh_a_pairs": ("block_flags", "value"), "selhip_hll_union_hist": ("block_hist", "value"),
    "selhip_ertl_estimate": ("block_estimates", "value"), "selhip_smh_match_counts": ("block_matches", "value"),
    "selhip_hll_fold": ("block_fold", "value"), "selhip_synth_generate": ("block_synth", "value"),
    "selhip_build_sketches": ("block_build", "value"), "selhip_permute_rows": ("block_permute", "value"),
    "selhip_hll_bitslice+union_hist_planes": ("block_hist", "value"),
    "components": ("components", "value"), "greedy_representatives": ("greedy_reps", "value"),
    "selhip_spanning_forest": ("block_forest", "value"), "selhip_linkage": ("block_linkage", "value"),
}
# selhip_permute_rows at the shapes no other test reaches: case id -> (rows, row bytes, byte offset of both pointers).  Row sizes that
# are no multiple of 16 and 16-byte multiples through pointers that are not 16-byte aligned take permute_bytes_kernel; 70 000 rows
# take the grid-stride loop past the 65 536 blocks of the grid
PERMUTE_SHAPES = {"permute-5B": (300, 5, 0), "permute-24B": (300, 24, 0), "permute-32B-offset8": (300, 32, 8),
                  "permute-70000x16B": (70_000, 16, 0), "permute-70000x5B": (70_000, 5, 0)}
BLOCK_CASES.update({k: (k, "value") for k in PERMUTE_SHAPES})
CASES = {**CONTEXT_CASES, **BLOCK_CASES}


def expected(S, case_id):
    """the expected value of a case on the data of S"""
    if case_id in PERMUTE_SHAPES:
        return S.permute_data(case_id)["want"]
    return getattr(S, CASES[case_id][0])
# entries that allocate and free device memory in every call -- hipFree waits for the whole device, the blocked null stream included --
# get run A only (module docstring of tests/test_streams_gpu.py)
RUN_A_ONLY = {"selhip_hll_bitslice+union_hist_planes", "components", "greedy_representatives", "grown_lists",
              "selhip_spanning_forest", "selhip_linkage", *LINKAGE_CASES}
# ... of which the hierarchy entries still run with the null stream blocked, for the ANSWER alone: their host loops launch round after
# round from words just read back, and a round left on the null stream shows only while that stream is held.  The hipFree at their end
# waits the delay out (it is then 300 ms, not sized from the call), so that run does not ask whether the null stream is still blocked
ANSWER_UNDER_BLOCKED_NULL = {"selhip_spanning_forest", "selhip_linkage", *LINKAGE_CASES}
BLOCKED_ANSWER_DELAY_MS = 300.0


def bits(x):
    """a value in a form that == compares bit for bit: records as (i, k, value bits) tuples, float arrays as their bit patterns,
    dicts and tuples element by element"""
    if isinstance(x, dict):
        return {k: bits(v) for k, v in sorted(x.items())}
    if isinstance(x, (tuple, list)):
        return [bits(v) for v in x]
    x = np.asarray(x)
    if x.dtype.names:
        return list(zip(x["i"].tolist(), x["k"].tolist(), np.ascontiguousarray(x["jaccard"], dtype=np.float64).view(np.uint64).tolist()))
    if x.dtype.kind == "f":
        return (x.shape, np.ascontiguousarray(x, dtype=np.float64).view(np.uint64).tolist())
    return (x.shape, x.astype(np.int64 if x.dtype.kind in "iub" and x.dtype != np.uint64 else x.dtype).tolist())


def same(got, want):
    return bits(got) == bits(want)


def describe(got, want):
    """a short account of a mismatch for the assertion message"""
    def size(v):
        if isinstance(v, dict):
            return {k: size(x) for k, x in v.items()}
        return np.asarray(v).shape
    return f"got {size(got)}, want {size(want)}"


# =====================================================================================================================
# the device side: everything below needs torch and a GPU and is used by tests/test_streams_gpu.py alone
# =====================================================================================================================
class Clock:
    """torch.cuda._sleep takes cycles: cycles per millisecond, measured once with two events"""

    def __init__(self):
        import torch
        torch.cuda.synchronize()
        probe = 20_000_000
        torch.cuda._sleep(1000)                                   # (the first launch loads the kernel)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(probe)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        assert 0.5 < ms < MAX_DELAY_MS, f"torch.cuda._sleep({probe}) took {ms} ms: the delay cannot be calibrated"
        self.cycles_per_ms = probe / ms

    def sleep(self, ms):
        """a delay of ms milliseconds (at most 2 s) on the current stream"""
        import torch
        torch.cuda._sleep(int(min(ms, MAX_DELAY_MS) * self.cycles_per_ms))


def pick_streams(clock, want=2, candidates=8):
    """up to `want` non-blocking streams that really run BESIDE a blocked null stream: with 4 hardware queues two streams can share one,
    and a stream that shares the null stream's queue waits behind its delay.  Of up to `candidates` torch pool streams, those whose
    tiny op completes while the null stream's delay is still running"""
    import torch
    good = []
    probe = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(candidates):
        cand = torch.cuda.Stream()
        clock.sleep(50.0)                                         # on the null stream
        with torch.cuda.stream(cand):
            probe.add_(1.0)
        ok = False
        while not torch.cuda.default_stream().query():
            if cand.query():
                ok = not torch.cuda.default_stream().query()
                break
        torch.cuda.synchronize()
        if ok and all(cand.cuda_stream != g.cuda_stream for g in good):
            good.append(cand)
            if len(good) == want:
                break
    return good


class Env:
    """what a case body sees: the stream, the attached tensors T, the data set that is loaded, and the hooks of the current run"""

    def __init__(self, clock, stream, sets):
        self.clock, self.s, self.sets = clock, stream, sets      # sets: {"real": Sets, "decoy": Sets}
        self.T, self.src, self.late = {}, {"real": {}, "decoy": {}}, set()
        self.phase, self.loaded = "warm", None
        self.poisoned = []
        # tensors that hold the REAL set already in the restore run: what a body does not hand over again under run B (a database whose
        # index is held), so that run B meets the products of the right database and the decoy's of everything else
        self.real_in_restore = set()

    # -- tensors ------------------------------------------------------------------------------------
    def tensors(self, make, late=()):
        """make(Sets) -> {name: numpy array}: the device copies of both sets (sources) and one set of working tensors T of the same
        shapes, which is what the library is handed.  late: the names written behind run A's SECOND delay"""
        import torch
        for name in ("real", "decoy"):
            for k, v in make(self.sets[name]).items():
                v = np.ascontiguousarray(v)
                if v.dtype in (np.uint64, np.uint32):          # (torch tensors carry the bit patterns as signed integers)
                    v = v.view(np.int64 if v.dtype == np.uint64 else np.int32)
                self.src[name][k] = torch.from_numpy(v).cuda()
        for k, v in self.src["real"].items():
            assert v.shape == self.src["decoy"][k].shape and v.dtype == self.src["decoy"][k].dtype, k
            self.T[k] = torch.empty_like(v)
        self.late |= set(late)
        torch.cuda.synchronize()

    def database(self, aux_hll=False, queries=False, extra=None, late=()):
        """the usual tensors: the database (and the queries) of the sets, plus extra(Sets) -> {name: array}"""
        def make(S):
            d = {"hll": S.D.hll, "aux": S.D.aux, "cards": S.D.cards}
            if aux_hll:
                d["aux_hll"] = S.D.aux_hll
            if queries:
                d.update(q_hll=S.Q.hll, q_aux=S.Q.aux, q_cards=S.Q.cards)
            if extra:
                d.update(extra(S))
            return d
        self.tensors(make, late)

    def load(self, name, late=False):
        """copy a set into the working tensors on the current stream (run A: the late ones only behind the second delay)"""
        for k, t in self.T.items():
            if self.phase == "A" and (k in self.late) != late:
                continue
            ahead = self.phase == "restore" and k in self.real_in_restore
            t.copy_(self.src["real" if ahead else name][k], non_blocking=True)
        self.loaded = name

    @property
    def data(self):
        """the Sets whose data the working tensors hold"""
        return self.sets[self.loaded]

    # -- hooks of a case body -------------------------------------------------------------------------
    def stall(self, late=True):
        """in front of the pass proper, behind every call that waits for the stream (attach, upload, fold).  Run A: the second delay,
        then the late inputs (late=False: not yet, a later stall of the body writes them); every run: caller-owned outputs registered
        with poison() are overwritten on the stream"""
        import torch
        if self.phase == "A":
            self.clock.sleep(DELAY_MS)
            if late:
                self.load("real", late=True)
        for t in self.poisoned:
            t.fill_(-7 if t.dtype.is_floating_point or t.dtype in (torch.int32, torch.int64) else 0xA5)
        if self.phase == "A":
            assert not self.s.query(), "run A: the stream's delay ended before the calls were made (premise of the test, not a defect)"

    def poison(self, *tensors):
        """caller-owned output tensors: overwritten on the stream in front of every pass, so that a result written ahead of the
        stream's own order is lost"""
        self.poisoned = list(tensors)

    def still_running(self, what):
        """behind an entry documented as asynchronous: under run A it must have returned with the stream's delay still pending"""
        if self.phase == "A":
            assert not self.s.query(), f"{what} is documented as asynchronous but returned with the stream idle under run A"

    def host(self, t):
        """a device tensor on the host, copied on the stream"""
        import torch
        with torch.cuda.stream(self.s):
            return t.cpu().numpy()

    def host_any_stream(self, t):
        """behind an entry documented as 'returns when complete': its output may be read from any stream.  Run A reads it with a plain
        .cpu() on the null stream (run B cannot: its null stream is blocked)"""
        import torch
        if self.phase == "A":
            with torch.cuda.stream(torch.cuda.default_stream()):
                return t.cpu().numpy()
        return self.host(t)


def _on_stream(env, body, name, streams):
    """load a set and run the body on the environment's stream; the body's other streams wait for the copies"""
    import torch
    with torch.cuda.stream(env.s):
        env.load(name)
        for other in streams:
            if other is not env.s:
                other.wait_stream(env.s)
        return body(env)


def plain_run(env, body, name, phase="warm", streams=()):
    """the body on the set `name`, nothing delayed, the device synchronised afterwards"""
    import torch
    env.phase = phase
    try:
        return _on_stream(env, body, name, streams)
    finally:
        torch.cuda.synchronize()


def run_a(env, body, want, streams=()):
    """run A: the caller's stream is late"""
    import torch
    env.phase = "A"
    try:
        with torch.cuda.stream(env.s):
            env.clock.sleep(DELAY_MS)
            env.load("real")
            assert not env.s.query(), "run A: the stream's delay ended before the copies were enqueued (premise of the test, not a defect)"
            for other in streams:
                if other is not env.s:
                    other.wait_stream(env.s)
            got = body(env)
    finally:
        torch.cuda.synchronize()
    assert same(got, want(env.sets["real"])), "run A (the caller's stream is late): the answer is not the real set's -- something ran " \
        "ahead of the stream and read the decoy: " + describe(got, want(env.sets["real"]))


def blocked_run(env, body, name, delay_ms, streams=()):
    """the body on the set `name` with the null stream blocked by a delay -> (outputs, the null stream was still blocked when the
    outputs were on the host and every stream of the body had drained)"""
    import torch
    try:
        env.clock.sleep(delay_ms)                                 # on the null stream
        got = _on_stream(env, body, name, streams)
        for st in {env.s, *streams}:
            st.synchronize()
        return got, not torch.cuda.default_stream().query()
    finally:
        torch.cuda.synchronize()


def run_b(env, body, want, streams=(), answer_only=False):
    """restore the decoy everywhere (timed: the sizing of the delay), then run B: the null stream is blocked.  answer_only: an entry
    that frees its scratch before it returns (ANSWER_UNDER_BLOCKED_NULL) -- a fixed delay, which the entry waits out, and the answer"""
    t0 = time.perf_counter()
    plain_run(env, body, "decoy", "restore", streams)
    wall_ms = (time.perf_counter() - t0) * 1e3
    delay_ms = BLOCKED_ANSWER_DELAY_MS if answer_only else min(MAX_DELAY_MS, 100.0 + 5.0 * wall_ms)
    env.phase = "B"
    got, blocked = blocked_run(env, body, "real", delay_ms, streams)
    assert same(got, want(env.sets["real"])), "run B (the null stream is blocked): the answer is not the real set's -- the effect of " \
        "something put on the null stream is missing: " + describe(got, want(env.sets["real"]))
    if answer_only:
        return
    assert blocked, f"run B: the null stream's delay ({delay_ms:.0f} ms; the same calls took {wall_ms:.1f} ms before) was over when the " \
        "outputs were on the host: the call waited for the null stream or for the whole device"


def runs_beside_null(env, body, streams=()):
    """a context's internal second lane (host_pass.hpp: st_stage1) is a stream of its own, and with 4 hardware queues it may share the
    null stream's: then its work waits behind run B's delay although the library did nothing wrong.  Warm the body up on the decoy,
    then run it once more with the null stream blocked: True if the null stream was still blocked afterwards"""
    plain_run(env, body, "decoy", "warm", streams)
    env.phase = "restore"
    return blocked_run(env, body, "decoy", 150.0, streams)[1]


def three_runs(env, body, want, run_b_too=True, streams=(), fresh=None, answer_only=False):
    """warm-up, run A, restore, run B of one case.  body(env) -> the outputs on the host; want(Sets) -> their expected value.
    streams: the streams the body uses besides the environment's.  fresh: called in front of run A (a case that needs a new context).
    answer_only: run B for its answer alone (run_b)"""
    got = plain_run(env, body, "decoy", "warm", streams)
    assert same(got, want(env.sets["decoy"])), "warm-up (decoy, synchronised): " + describe(got, want(env.sets["decoy"]))
    if fresh:
        fresh()
    run_a(env, body, want, streams)
    if run_b_too or answer_only:
        run_b(env, body, want, streams, answer_only=answer_only and not run_b_too)

