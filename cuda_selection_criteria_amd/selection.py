"""Host-side mirror of the reference's GPU selection driver (src/selection_cuda.cpp:59-189) on top of
the C ABI.  Same steps, same names: load_file_list -> read sketches -> report() -> sort by cardinality
-> banding -> flatten -> upload -> launch -> copy back -> print; all the work happens in
libselhost.so (C++) and libselhip.so (HIP)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import (ALGO_AUTO, BANDING_CPU, CRIT_HLL_A, CRIT_HLL_AN, CRIT_HLL_A_SMH_A, CRIT_NONE, CRIT_SMH_A, CRIT_SMH_C, ESTIMATOR_HLL, ESTIMATOR_SMH, F32, F64, FP_FMA,
                   MEASURE_CONTAINMENT, MEASURE_INTERSECTION, MEASURE_JACCARD, MEASURE_MAX_CONTAINMENT, MEASURE_SMH_JACCARD,
                   MEASURE_SMH_MATCHES, MEASURE_UNION, MODE_CB_SMH, REP_MAX_DEGREE, REP_MAX_RANK, REP_MIN_RANK, REP_PRIORITY, TOPK_ROUNDS_AUTO, LINKAGE_SINGLE, LINKAGE_COMPLETE, LINKAGE_AVERAGE, LINKAGE_WEIGHTED, Clusters, Forest, Greedy, Linkage, Merged, Pair, check, hip_lib,
                   host_lib)

# layout of selhip_pair_t {int32 i, k; double jaccard}
PAIR_DTYPE = np.dtype([("i", "<i4"), ("k", "<i4"), ("jaccard", "<f8")], align=True)
assert PAIR_DTYPE.itemsize == C.sizeof(Pair) == 16


def banding(m: int, tau: float, variant: int = BANDING_CPU) -> Tuple[int, int]:
    """(n_rows, n_bands) of src/selection.cpp:258-267 (CPU variant) or selection_cuda.cpp:119-128."""
    r, b = C.c_int(), C.c_int()
    host_lib().selhost_banding(m, np.float32(tau), variant, C.byref(r), C.byref(b))
    return r.value, b.value


def sort_by_card(cards: np.ndarray) -> np.ndarray:
    """perm[rank] = original index; libstdc++ std::sort with the comparator of selection.cpp:251-256."""
    cards = np.ascontiguousarray(cards, dtype=np.float64)
    perm = np.empty(cards.shape[0], dtype=np.int32)
    rc = host_lib().selhost_sort_by_card(cards.ctypes.data, cards.shape[0], perm.ctypes.data)
    if rc:
        raise RuntimeError(host_lib().selhost_last_error().decode())
    return perm


@dataclass
class Dataset:
    names: list
    hll: np.ndarray        # [n, 16384] u8, rank order
    aux: np.ndarray        # [n, m] u64
    aux_hll: np.ndarray    # [n, 1 << p_aux] u8 (empty when p_aux == 0)
    cards: np.ndarray      # [n] f64 ascending
    order: Optional[np.ndarray] = None   # [n] i32: the line of the file list each rank came from (the sort permutation)


def load_dataset(list_file: str, m: int, p_aux: int = 0, fp_mode: int = FP_FMA, threads: int = 8) -> Dataset:
    """selection_cuda.cpp:90-143: read <name>.hll / <name>.smh<m>, report(), sort, flatten."""
    h = host_lib()
    ds = C.c_void_p()
    rc = h.selhost_dataset_load(C.byref(ds), list_file.encode(), m, p_aux, fp_mode, threads)
    if rc:
        raise RuntimeError(f"selhost error {rc}: {h.selhost_last_error().decode()}")
    try:
        n = h.selhost_dataset_size(ds)
        def arr(ptr, shape, dt):
            count = int(np.prod(shape))
            if n == 0 or count == 0:
                return np.zeros(shape, dtype=dt)
            buf = (C.c_uint8 * (count * np.dtype(dt).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dt).reshape(shape).copy()
        hll = arr(h.selhost_dataset_hll(ds), (n, 16384), np.uint8)
        aux = arr(h.selhost_dataset_aux(ds), (n, m), np.uint64)
        aux_hll = arr(h.selhost_dataset_aux_hll(ds), (n, (1 << p_aux) if p_aux else 0), np.uint8)
        cards = arr(h.selhost_dataset_cards(ds), (n,), np.float64)
        names = [h.selhost_dataset_name(ds, r).decode() for r in range(n)]
        order = np.array([h.selhost_dataset_order(ds, r) for r in range(n)], dtype=np.int32)
    finally:
        h.selhost_dataset_free(ds)
    return Dataset(names, hll, aux, aux_hll, cards, order)


def hll_fold(hll: np.ndarray, p_aux: int) -> np.ndarray:
    """HLL sketches [n, 1 << p] (or one sketch [1 << p]) folded to the lower precision p_aux on the host (selhost_hll_fold): the registers
    of the .hll_<p_aux> files build_sketch writes beside the .hll files, without reading them.  4 <= p_aux <= min(p, 15)."""
    hll = np.ascontiguousarray(hll, dtype=np.uint8)
    rows = hll.reshape(1, -1) if hll.ndim == 1 else hll
    if rows.ndim != 2 or rows.shape[1] < 16 or rows.shape[1] & (rows.shape[1] - 1):
        raise ValueError(f"hll must be [n, 1 << p] with p in 4..20, got shape {hll.shape}")
    p = rows.shape[1].bit_length() - 1
    out = np.zeros((rows.shape[0], 1 << p_aux) if 0 <= p_aux < 31 else (0, 0), dtype=np.uint8)
    if host_lib().selhost_hll_fold(rows.ctypes.data, rows.shape[0], p, p_aux, out.ctypes.data) < 0:
        raise ValueError(host_lib().selhost_last_error().decode())
    return out[0] if hll.ndim == 1 else out


def format_lines(names: Sequence[str], pairs: np.ndarray) -> str:
    """'fn1 fn2 <std::to_string(J)>\\n' per selected pair (selection.cpp:288)."""
    h = host_lib()
    buf = C.create_string_buffer(16384)
    out = []
    for rec in pairs:
        w = h.selhost_format_line(names[rec["i"]].encode(), names[rec["k"]].encode(), float(rec["jaccard"]), buf, len(buf))
        if w < 0:
            raise RuntimeError("line too long")
        out.append(buf.raw[:w].decode())
    return "".join(out)


def write_results(path: str, pairs: np.ndarray, names: Sequence[str], tau: float = 0.0):
    """binary result file of include/selection_host.h (records + the name table their ranks refer to)"""
    h = host_lib()
    rec = np.ascontiguousarray(pairs, dtype=PAIR_DTYPE)
    enc = [n.encode() for n in names]
    arr = (C.c_char_p * len(enc))(*enc)
    rc = h.selhost_write_results(str(path).encode(), rec.ctypes.data if len(rec) else None, len(rec), arr if enc else None, len(enc),
                                 np.float32(tau))
    if rc:
        raise RuntimeError(h.selhost_last_error().decode())


def read_results(path: str):
    """-> (pairs[PAIR_DTYPE], names, tau, text) of a result file; text = the reference's stdout form"""
    h = host_lib()
    r = C.c_void_p()
    rc = h.selhost_read_results(C.byref(r), str(path).encode())
    if rc:
        raise RuntimeError(h.selhost_last_error().decode())
    try:
        cnt = h.selhost_results_count(r)
        nn = h.selhost_results_names(r)
        pairs = np.zeros(cnt, dtype=PAIR_DTYPE)
        if cnt:
            C.memmove(pairs.ctypes.data, h.selhost_results_pairs(r), cnt * PAIR_DTYPE.itemsize)
        names = [h.selhost_results_name(r, g).decode() for g in range(nn)]
        need = h.selhost_results_text(r, None, 0)
        text = ""
        if need > 0:
            buf = C.create_string_buffer(need + 1)
            h.selhost_results_text(r, buf, need + 1)
            text = buf.raw[:need].decode()
        return pairs, names, float(h.selhost_results_tau(r)), text
    finally:
        h.selhost_results_free(r)


class Selector:
    """One selhip context = one GPU (`selhip_ctx_*`, include/selection_hip.h section 2)."""

    DEFAULT_PARAMS: dict = {}      # selhip_ctx_set_param applied to every new context (the test-suite groups small sets too: "group_min_n" = 0)

    def __init__(self, device: int = 0, fp_mode: int = FP_FMA, stream: Optional[int] = None):
        self._lib = hip_lib()
        self._ctx = C.c_void_p()
        check(self._lib.selhip_ctx_create(C.byref(self._ctx), device))
        check(self._lib.selhip_ctx_set_fp_mode(self._ctx, fp_mode), self._ctx)
        for name, value in self.DEFAULT_PARAMS.items():
            check(self._lib.selhip_ctx_set_param(self._ctx, name.encode(), int(value)), self._ctx)
        if stream is not None:
            check(self._lib.selhip_ctx_set_stream(self._ctx, C.c_void_p(stream)), self._ctx)
        self.device = device
        self.n = 0
        self.m = 0
        self.n_q = None             # rows of the loaded query set (None: none; uploading / attaching the database drops it)
        self.p_hll = 14             # precision of the main sketches (upload / attach)
        self.p_aux = 0              # precision of the auxiliary sketches the context holds (0: none; upload / attach drops them)
        self._keep = None

    def close(self):
        if self._ctx:
            self._lib.selhip_ctx_destroy(self._ctx)         # (waits for the stream: a pending list pass is over)
            self._ctx = C.c_void_p()
            self._drop_pairs()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, stream: Optional[int]):
        """all work of this context runs on `stream` from now on (a hipStream_t as an integer, e.g. torch's Stream.cuda_stream; None = the null stream)"""
        check(self._lib.selhip_ctx_set_stream(self._ctx, C.c_void_p(stream)), self._ctx)

    # -- sketches ---------------------------------------------------------------------------------
    def upload(self, hll: np.ndarray, aux: np.ndarray, cards: Optional[np.ndarray] = None, p_hll: int = 14):
        hll = np.ascontiguousarray(hll, dtype=np.uint8)
        aux = np.ascontiguousarray(aux, dtype=np.uint64)
        n, m = aux.shape
        assert hll.shape == (n, 1 << p_hll), (hll.shape, n, p_hll)
        cp = None
        if cards is not None:
            cards = np.ascontiguousarray(cards, dtype=np.float64)
            assert cards.shape == (n,)
            cp = cards.ctypes.data
        check(self._lib.selhip_ctx_upload(self._ctx, hll.ctypes.data, aux.ctypes.data, cp, n, m, p_hll), self._ctx)
        self.n, self.m = n, m
        self.p_hll, self.p_aux = p_hll, 0
        self.n_q = None                                                # (the library dropped the queries)

    def attach(self, hll_t, aux_t, cards_t=None, p_hll: int = 14):
        """torch CUDA tensors: hll uint8 [n, 1<<p], aux int64 [n, m] (bit pattern of the u64 buckets),
        cards float64 [n] ascending or None."""
        n, m = aux_t.shape
        assert hll_t.is_cuda and aux_t.is_cuda and hll_t.is_contiguous() and aux_t.is_contiguous()
        assert tuple(hll_t.shape) == (n, 1 << p_hll) and aux_t.element_size() == 8 and hll_t.element_size() == 1
        cp = None
        if cards_t is not None:
            assert cards_t.is_cuda and cards_t.is_contiguous() and cards_t.element_size() == 8 and cards_t.shape[0] == n
            cp = cards_t.data_ptr()
        check(self._lib.selhip_ctx_attach(self._ctx, hll_t.data_ptr(), aux_t.data_ptr(), cp, n, m, p_hll), self._ctx)
        self._keep = (hll_t, aux_t, cards_t)
        self.n, self.m = n, m
        self.p_hll, self.p_aux = p_hll, 0
        self.n_q = None

    def upload_queries(self, hll: np.ndarray, aux: np.ndarray, cards: Optional[np.ndarray] = None):
        """query sketches (ascending cardinality, the database's m, p = 14) for run_queries; cards None = computed on the device"""
        hll = np.ascontiguousarray(hll, dtype=np.uint8)
        aux = np.ascontiguousarray(aux, dtype=np.uint64)
        n_q = aux.shape[0]
        assert aux.shape == (n_q, self.m) and hll.shape == (n_q, 1 << 14), (hll.shape, aux.shape, self.m)
        cp = None
        if cards is not None:
            cards = np.ascontiguousarray(cards, dtype=np.float64)
            assert cards.shape == (n_q,)
            cp = cards.ctypes.data
        check(self._lib.selhip_ctx_upload_queries(self._ctx, hll.ctypes.data if n_q else None, aux.ctypes.data if n_q else None,
                                                  cp, n_q), self._ctx)
        self.n_q = n_q

    def attach_queries(self, hll_t, aux_t, cards_t=None):
        """torch CUDA tensors of the queries (layout as attach); the caller keeps them alive and unchanged"""
        n_q = aux_t.shape[0]
        assert hll_t.is_cuda and aux_t.is_cuda and hll_t.is_contiguous() and aux_t.is_contiguous()
        assert tuple(hll_t.shape) == (n_q, 1 << 14) and tuple(aux_t.shape) == (n_q, self.m) and aux_t.element_size() == 8
        cp = None
        if cards_t is not None:
            assert cards_t.is_cuda and cards_t.is_contiguous() and cards_t.element_size() == 8 and cards_t.shape[0] == n_q
            cp = cards_t.data_ptr()
        check(self._lib.selhip_ctx_attach_queries(self._ctx, hll_t.data_ptr(), aux_t.data_ptr(), cp, n_q), self._ctx)
        self._keep_q = (hll_t, aux_t, cards_t)
        self.n_q = n_q

    def upload_queries_aux_hll(self, aux_hll: np.ndarray, p_aux: int):
        """auxiliary HLL sketches of the queries (query rank order) for the criteria other than smh_a; after upload_queries /
        attach_queries, which drop them"""
        aux_hll = np.ascontiguousarray(aux_hll, dtype=np.uint8)
        if self.n_q is not None:                                       # (without a query set the library refuses the call)
            assert aux_hll.shape == (self.n_q, 1 << p_aux), (aux_hll.shape, self.n_q, p_aux)
        check(self._lib.selhip_ctx_upload_queries_aux_hll(self._ctx, aux_hll.ctypes.data if aux_hll.size else None, p_aux), self._ctx)

    def attach_queries_aux_hll(self, aux_hll_t, p_aux: int):
        """a torch CUDA uint8 tensor (n_q, 1 << p_aux); the caller keeps it alive and unchanged"""
        assert aux_hll_t.is_cuda and aux_hll_t.is_contiguous()
        if self.n_q is not None:
            assert tuple(aux_hll_t.shape) == (self.n_q, 1 << p_aux), (tuple(aux_hll_t.shape), self.n_q, p_aux)
        check(self._lib.selhip_ctx_attach_queries_aux_hll(self._ctx, aux_hll_t.data_ptr() if aux_hll_t.numel() else None, p_aux), self._ctx)
        self._keep_q_aux = aux_hll_t

    def run_queries(self, tau: float, mode: int = MODE_CB_SMH, n_rows: Optional[int] = None, n_bands: Optional[int] = None,
                    algo: int = ALGO_AUTO, fetch: bool = True, top_k: Optional[int] = None):
        """one query pass (queries x database) under the criterion of set_criterion: records {i = query rank, k = database rank,
        jaccard} sorted by (i, k).  top_k given: set_query_topk(top_k) first (the setting stays), and with top_k > 0 the records come
        in ranked order (fetch_ranked): every query's top_k best, J descending, ties by ascending database rank"""
        if top_k is not None:
            self.set_query_topk(top_k)
        if n_rows is None or n_bands is None:
            n_rows, n_bands = banding(self.m, tau) if self.m else (1, 1)
        check(self._lib.selhip_ctx_run_queries(self._ctx, mode, algo, np.float32(tau), n_rows, n_bands), self._ctx)
        if not fetch:
            return None
        return self.fetch_ranked() if top_k else self.fetch()

    def set_query_topk(self, k: int):
        """the following query passes keep every query's k best records (J descending in the IEEE total order, ties by ascending
        database rank), cut and ordered on the device: 1 .. TOPK_MAX; 0 = off (the default).  The best among the pairs that pass
        the criterion and tau, not an unconditional nearest-neighbour search -- for that: CRIT_NONE, MODE_SMH and a tau below every J
        (e.g. -1).  stats()["selected"] stays the uncut count"""
        check(self._lib.selhip_ctx_set_query_topk(self._ctx, int(k)), self._ctx)

    def set_allpairs_topk(self, k: int):
        """the following all-pairs passes (run, run_async + finish) keep every genome's k best partners: a selected pair (i, k, J)
        counts for both of its genomes, records come as {i = owner, k = partner, jaccard}, ranked like a query's (J descending in the
        IEEE total order, ties by ascending partner rank), cut and ordered on the device: 1 .. TOPK_MAX; 0 = off (the default).  The
        reduced list can be longer than the pass's own (up to twice).  The best among the pairs that pass the criterion and tau -- for
        every genome's exact nearest neighbours: CRIT_NONE, MODE_SMH and a tau below every J (e.g. -1).  stats()["selected"] stays the
        uncut count; query passes ignore the setting"""
        check(self._lib.selhip_ctx_set_allpairs_topk(self._ctx, int(k)), self._ctx)

    def set_topk_rounds(self, rows):
        """the following all-pairs top-k passes of CRIT_SMH_C under set_estimator("smh") run in rounds of `rows` rows: each round is
        merged into a carried list of at most k records per genome, whose k-th values are the next round's admission thresholds --
        the same ranked list, record for record, with n k + one round's admitted records of memory instead of |S|.  0 = off (the
        default), "auto" (or TOPK_ROUNDS_AUTO) = the largest R with R n <= 2^27.  Sticky; query and pair-list passes ignore it, any
        other all-pairs pass is refused while it is on.  get_param("topk_rounds_used"), ("topk_admitted_lo"), ("topk_admitted_hi")"""
        check(self._lib.selhip_ctx_set_topk_rounds(self._ctx, topk_rounds_code(rows)), self._ctx)

    def fetch_ranked(self) -> np.ndarray:
        """the reduced list of the last pass as it lies on the device: query rank (all-pairs: owner rank) ascending, within it best
        first (no host sort); raises unless that pass ran with its top-k on"""
        cnt = self.result_count()
        out = np.zeros(cnt, dtype=PAIR_DTYPE)
        check(self._lib.selhip_ctx_fetch_ranked(self._ctx, out.ctypes.data if cnt else None, cnt), self._ctx)
        return out

    def upload_aux_hll(self, aux_hll: np.ndarray, p_aux: int):
        """auxiliary HLL sketches (.hll_<p> files) for the hll_a / hll_an criteria, rank order"""
        aux_hll = np.ascontiguousarray(aux_hll, dtype=np.uint8)
        assert aux_hll.shape == (self.n, 1 << p_aux)
        check(self._lib.selhip_ctx_upload_aux_hll(self._ctx, aux_hll.ctypes.data, p_aux), self._ctx)
        self.p_aux = p_aux

    def fold_aux_hll(self, p_aux: int):
        """the auxiliary HLL sketches of upload_aux_hll without their files: folded on the device from the main sketches the context
        holds, uploaded or attached (selhip_ctx_fold_aux_hll); p_aux in 4 .. min(p_hll, 15).  A snapshot: fold again after new sketches"""
        check(self._lib.selhip_ctx_fold_aux_hll(self._ctx, p_aux), self._ctx)
        self._keep_aux = None
        self.p_aux = p_aux

    def fold_queries_aux_hll(self, p_aux: int):
        """the same for the query set (selhip_ctx_fold_queries_aux_hll), in place of upload_queries_aux_hll"""
        check(self._lib.selhip_ctx_fold_queries_aux_hll(self._ctx, p_aux), self._ctx)
        self._keep_q_aux = None

    def attach_aux_hll(self, aux_hll_t, p_aux: int):
        assert aux_hll_t.is_cuda and aux_hll_t.is_contiguous() and tuple(aux_hll_t.shape) == (self.n, 1 << p_aux)
        check(self._lib.selhip_ctx_attach_aux_hll(self._ctx, aux_hll_t.data_ptr(), p_aux), self._ctx)
        self._keep_aux = aux_hll_t
        self.p_aux = p_aux

    def set_pipeline(self, chunks: int):
        """-1 auto, 0 off, 2..8 forced: overlap of stage 1 (next row chunk) with stage 2 (previous chunk)"""
        check(self._lib.selhip_ctx_set_pipeline(self._ctx, chunks), self._ctx)

    def set_row_interleave(self, block_rows: int, n_parts: int, part: int):
        """the following runs evaluate only this part's row blocks (of block_rows rows, dealt to the n_parts parts boustrophedon:
        distributed.interleave_owner)"""
        check(self._lib.selhip_ctx_set_row_interleave(self._ctx, block_rows, n_parts, part), self._ctx)

    def set_candidate_begin(self, k_min: int):
        """rectangular passes: the following runs only take candidates k >= k_min (reset by upload/attach)"""
        check(self._lib.selhip_ctx_set_candidate_begin(self._ctx, k_min), self._ctx)

    def set_param(self, name: str, value: int):
        check(self._lib.selhip_ctx_set_param(self._ctx, name.encode(), value), self._ctx)

    def get_param(self, name: str) -> int:
        v = C.c_int(0)
        check(self._lib.selhip_ctx_get_param(self._ctx, name.encode(), C.byref(v)), self._ctx)
        return int(v.value)

    def set_stage2_grouping(self, enable: bool):
        check(self._lib.selhip_ctx_set_stage2_grouping(self._ctx, 1 if enable else 0), self._ctx)

    def set_criterion(self, criterion: int):
        check(self._lib.selhip_ctx_set_criterion(self._ctx, criterion), self._ctx)
        self.criterion = criterion

    def set_min_matches(self, c: int):
        """the count threshold of criterion smh_c (CRIT_SMH_C): a pair survives stage 1 iff at least c of its m SuperMinHash buckets
        are equal (c >= 1; a pass refuses c > m).  min_matches(m, j) gives the c of a SuperMinHash Jaccard estimate j"""
        check(self._lib.selhip_ctx_set_min_matches(self._ctx, int(c)), self._ctx)

    def set_min_containment(self, gamma: Optional[float]):
        """the per-pair count threshold of criterion smh_c for a minimum containment gamma: a pair survives stage 1 iff its equal
        buckets c reach containment_matches(m, gamma, min(e_i, e_k), max(e_i, e_k)) -- the count at which the SuperMinHash estimate of
        the smaller genome's containment is gamma -- and set_min_matches' c, which stays as a floor when set.  Sticky; None (or NaN)
        clears it; +-inf is refused"""
        check(self._lib.selhip_ctx_set_min_containment(self._ctx, float("nan") if gamma is None else float(gamma)), self._ctx)

    def set_measure(self, measure):
        """what stage 2 of the following passes (run, run_queries, run_pairs and their top-ks) tests against tau and records in the
        `jaccard` field: "jaccard" (the default) or "max_containment" -- I / min(e_i, e_k) with I = e_i + e_k - U, the share of the
        smaller genome found in the larger one -- or the MEASURE_* code of either.  Sticky, like the criterion.  Under
        "max_containment" a pass refuses MODE_CB_SMH and the hll_a / hll_an / two-stage criteria (bounds on J): MODE_SMH with
        CRIT_NONE, CRIT_SMH_A or CRIT_SMH_C"""
        code = measure_code(measure)
        check(self._lib.selhip_ctx_set_measure(self._ctx, code), self._ctx)
        self.measure = code

    def set_estimator(self, estimator):
        """which estimate the following passes test against tau and record in the `jaccard` field: "hll" (the default: the HLL
        estimate of stage 2, nothing changes) or "smh" -- the SuperMinHash estimate smh_value(measure, m, c, e_i, e_k) of the count c
        that a CRIT_SMH_C pass computes anyway: c / m under "jaccard", c (a + b) / ((m + c) a) under "max_containment" -- or the
        ESTIMATOR_* code of either.  Sticky, like the measure.  Under "smh" the records leave the count kernel itself (no stage 2, no
        HLL register read), a pair needs c >= its count threshold AND value >= tau, and a pass of any criterion but CRIT_SMH_C is
        refused"""
        code = estimator_code(estimator)
        check(self._lib.selhip_ctx_set_estimator(self._ctx, code), self._ctx)
        self.estimator = code

    def cards(self) -> np.ndarray:
        out = np.empty(self.n, dtype=np.float64)
        check(self._lib.selhip_ctx_get_cards(self._ctx, out.ctypes.data), self._ctx)
        return out

    # -- the hot path -------------------------------------------------------------------------------
    def run(self, tau: float, mode: int = MODE_CB_SMH, n_rows: Optional[int] = None, n_bands: Optional[int] = None,
            rows: Optional[Tuple[int, int]] = None, algo: int = ALGO_AUTO, fetch: bool = True, top_k: Optional[int] = None,
            rounds=None):
        """one all-pairs pass: records {i, k, jaccard}, i < k, sorted by (i, k).  top_k given: set_allpairs_topk(top_k) first (the
        setting stays), and with top_k > 0 the records come in ranked order (fetch_ranked): every genome's top_k best partners as
        {i = owner, k = partner, jaccard}, J descending, ties by ascending partner rank.  rounds given: set_topk_rounds(rounds) first
        (the setting stays)"""
        if top_k is not None:
            self.set_allpairs_topk(top_k)
        if rounds is not None:
            self.set_topk_rounds(rounds)
        if n_rows is None or n_bands is None:
            n_rows, n_bands = banding(self.m, tau) if self.m else (1, 1)
        rb, re = rows if rows is not None else (0, self.n)
        check(self._lib.selhip_ctx_run(self._ctx, mode, algo, np.float32(tau), n_rows, n_bands, rb, re), self._ctx)
        if not fetch:
            return None
        return self.fetch_ranked() if top_k else self.fetch()

    def run_async(self, tau: float, mode: int = MODE_CB_SMH, n_rows: Optional[int] = None, n_bands: Optional[int] = None,
                  rows: Optional[Tuple[int, int]] = None, algo: int = ALGO_AUTO):
        if n_rows is None or n_bands is None:
            n_rows, n_bands = banding(self.m, tau)
        rb, re = rows if rows is not None else (0, self.n)
        check(self._lib.selhip_ctx_run_async(self._ctx, mode, algo, np.float32(tau), n_rows, n_bands, rb, re), self._ctx)

    def finish(self):
        try:
            check(self._lib.selhip_ctx_finish(self._ctx), self._ctx)
        finally:
            self._drop_pairs()

    # -- pair-list passes ---------------------------------------------------------------------------
    @staticmethod
    def _release_pairs(lib, held):
        if held is not None and held[0] == "own" and held[1]:
            lib.selhip_free(C.c_void_p(held[1]))

    def _drop_pairs(self):
        """the list of the last list pass is no longer read: free the device copy of a numpy list, release a caller's tensor"""
        held, self._pairs_held = getattr(self, "_pairs_held", None), None
        self._release_pairs(self._lib, held)

    def _device_pairs(self, pairs):
        """-> (what to keep until finish, device pointer, entries) of a list given as a numpy int32 (P, 2) array (copied to the device)
        or a torch int32 device tensor of that shape (kept referenced: a pass that outgrows a list reads it again)"""
        if isinstance(pairs, np.ndarray) or not hasattr(pairs, "data_ptr"):
            arr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
            ptr = C.c_void_p()
            if len(arr):
                check(self._lib.selhip_malloc(C.byref(ptr), arr.nbytes))
                check(self._lib.selhip_memcpy_h2d(ptr, arr.ctypes.data, arr.nbytes))
            return ("own", ptr.value), ptr.value, len(arr)
        assert pairs.is_cuda and pairs.is_contiguous() and pairs.element_size() == 4 and pairs.dim() == 2 and pairs.shape[1] == 2, \
            "pairs: a contiguous int32 device tensor of shape (P, 2)"
        return ("tensor", pairs), (pairs.data_ptr() if pairs.numel() else None), int(pairs.shape[0])

    def run_pairs_async(self, pairs, tau: float, mode: int = MODE_CB_SMH, n_rows: Optional[int] = None, n_bands: Optional[int] = None,
                        algo: int = ALGO_AUTO):
        """enqueue one pair-list pass (see run_pairs); finish() waits for it"""
        if n_rows is None or n_bands is None:
            n_rows, n_bands = banding(self.m, tau) if self.m else (1, 1)
        held, ptr, cnt = self._device_pairs(pairs)
        try:
            check(self._lib.selhip_ctx_run_pairs_async(self._ctx, ptr, cnt, mode, algo, np.float32(tau), n_rows, n_bands), self._ctx)
        except Exception:
            self._release_pairs(self._lib, held)      # (refused: a pass that is still pending keeps its own list)
            raise
        self._drop_pairs()
        self._pairs_held = held

    def run_pairs(self, pairs, tau: float, mode: int = MODE_CB_SMH, n_rows: Optional[int] = None, n_bands: Optional[int] = None,
                  algo: int = ALGO_AUTO, fetch: bool = True):
        """one pass of the criterion of set_criterion over a list of pairs: `pairs` is a numpy int32 (P, 2) array or a torch int32
        device tensor of ranks {x, y} in either order.  One record {min, max, jaccard} for every entry whose pair an all-pairs pass
        with the same arguments selects (an entry listed twice comes twice), sorted by (i, k); statistics count entries.  An entry
        with x == y or a rank outside [0, n) raises (SELHIP_E_BADARG, the message names one).  algo: ALGO_AUTO, ALGO_SIG (signature
        route) or ALGO_STREAM (direct route, any band shape); get_param("pairs_route_used") tells which ran"""
        self.run_pairs_async(pairs, tau, mode, n_rows, n_bands, algo)
        self.finish()
        return self.fetch() if fetch else None

    # -- dense matrices -----------------------------------------------------------------------------
    def _matrix(self, query: bool, measure, dtype, rows, row_pos, col_pos, out):
        import torch
        code = measure_code(measure)
        if dtype not in (torch.float64, torch.float32):
            raise ValueError("dtype: torch.float64 or torch.float32")
        if query and self.n_q is None:
            check(self._lib.selhip_ctx_query_matrix(self._ctx, code, F64, 0, 0, None, 0, 0, 0, None, None), self._ctx)   # (raises: no queries)
        r0, r1 = rows if rows is not None else (0, self.n_q if query else self.n)
        if out is None:
            n_out_rows = max(r1 - r0, 0) if row_pos is None else int(np.max(row_pos[r0:r1], initial=-1)) + 1
            n_out_cols = self.n if col_pos is None else int(np.max(col_pos, initial=-1)) + 1
            out = torch.empty((max(n_out_rows, 0), max(n_out_cols, 0)), dtype=dtype, device=torch.device("cuda", self.device))
        assert out.is_cuda and out.dim() == 2 and out.dtype == dtype, "out: a 2-D device tensor of the requested dtype"
        assert out.shape[1] <= 1 or out.stride(1) == 1, "out: stride(1) must be 1"
        ld = out.stride(0) if out.shape[0] > 1 else max(out.stride(0), out.shape[1])
        rp = None if row_pos is None else np.ascontiguousarray(row_pos, dtype=np.int32)
        cp = None if col_pos is None else np.ascontiguousarray(col_pos, dtype=np.int32)
        if rp is not None:
            assert rp.ndim == 1 and len(rp) >= r1, "row_pos is indexed by rank: it covers the ranks below rows[1]"
        if cp is not None:
            assert cp.shape == (self.n,), "col_pos: one position per column rank"
        fn = self._lib.selhip_ctx_query_matrix if query else self._lib.selhip_ctx_matrix
        check(fn(self._ctx, code, F32 if dtype == torch.float32 else F64, r0, r1, out.data_ptr() if out.numel() else None,
                 out.shape[0], out.shape[1], ld, None if rp is None else rp.ctypes.data, None if cp is None else cp.ctypes.data), self._ctx)
        return out

    def matrix(self, measure="jaccard", dtype=None, rows: Optional[Tuple[int, int]] = None, row_pos=None, col_pos=None, out=None):
        """the similarity of every pair of the context's sketches as a torch tensor on the device (selhip_ctx_matrix): measure
        "jaccard" (J of the passes, bit for bit; exactly 1.0 on the diagonal; NaN for two empty sketches), "union" (the union
        estimate U, also on the diagonal), "intersection" (I = e_row + e_col - U, also on the diagonal), "containment" (I / e_row, the
        share of the row genome found in the column genome: not symmetric, NaN for an empty row sketch, 1.0 on the diagonal),
        "max_containment" (I / min(e_row, e_col), the value of the passes under set_measure; 1.0 on the diagonal), "smh_matches" (the number of equal SuperMinHash buckets of the pair, 0 .. m) or "smh_jaccard"
        (that count / m: the SuperMinHash estimate of J; both from the bucket rows alone, whatever p_hll), dtype torch.float64 (default) or torch.float32.  rows = (r0, r1): only that slab of rows.
        row_pos / col_pos: host int32 arrays indexed by rank -- the cell of rank-row i and rank-column k goes to
        out[row_pos[i], col_pos[k]] (defaults i - r0 and k).  out: a caller's 2-D tensor (stride(1) == 1; stride(0) is its leading
        dimension), written in place and returned; cells no (row, column) maps to keep their content"""
        import torch
        return self._matrix(False, measure, dtype or torch.float64, rows, row_pos, col_pos, out)

    def query_matrix(self, measure="jaccard", dtype=None, rows: Optional[Tuple[int, int]] = None, row_pos=None, col_pos=None, out=None):
        """as matrix, rows = the attached queries, columns = the database (selhip_ctx_query_matrix): no diagonal, no symmetry"""
        import torch
        return self._matrix(True, measure, dtype or torch.float64, rows, row_pos, col_pos, out)

    # -- clusters of the result list ------------------------------------------------------------------
    def cluster(self, min_value: Optional[float] = None, rep="max_degree", to_host: bool = True) -> dict:
        """the single-linkage clusters of the result list the context holds, computed on the device (selhip_ctx_cluster): the connected
        components of the graph on the n ranks whose edges are the records with value >= min_value (None: every record).  Behind an
        all-pairs pass (any criterion; with top_k the directed list is taken as undirected edges) or a pair-list pass; not behind a
        query pass.  rep picks every cluster's representative: "max_degree" (most records, ties to the smaller rank), "min_rank" (the
        smallest genome = the label) or "max_rank" (the largest), or a REP_* code.  Returns a dict: "labels" [n] (smallest rank of the
        component), "clusters" [n] (dense id, by ascending label), "degrees" [n] (records the genome appears in), "sizes" [C],
        "representatives" [C] -- int32 numpy arrays, or torch tensors on the device with to_host=False -- and "n_clusters" = C"""
        import torch
        code = rep_code(rep)
        mv = float("-inf") if min_value is None else float(min_value)
        bufs = [torch.empty(self.n, dtype=torch.int32, device=torch.device("cuda", self.device)) for _ in range(5)]
        out = Clusters(*[b.data_ptr() if self.n else None for b in bufs])
        cnt = C.c_int64()
        check(self._lib.selhip_ctx_cluster(self._ctx, mv, code, C.byref(out), C.byref(cnt)), self._ctx)
        c = int(cnt.value)
        res = {"labels": bufs[0], "clusters": bufs[1], "degrees": bufs[2], "sizes": bufs[3][:c], "representatives": bufs[4][:c]}
        if to_host:
            res = {k: v.cpu().numpy() for k, v in res.items()}
        res["n_clusters"] = c
        return res

    def cluster_greedy(self, min_value: Optional[float] = None, order="max_degree", priority=None, to_host: bool = True) -> dict:
        """the greedy representative clusters of the result list the context holds (selhip_ctx_cluster_greedy; CD-HIT / UCLUST): the
        genomes are visited in `order` -- "max_degree" (most records first, ties to the smaller rank), "min_rank", "max_rank" (the
        largest sketch first, the CD-HIT order), "priority", or a REP_* code -- and one becomes a representative unless a record with
        value >= min_value (None: every record) already joins it to one; every other genome belongs to the representative it has the
        greatest value with (ties to the smaller rank).  priority: n unsigned 32-bit scores, greater first (a numpy array or a torch
        uint32 / int32 device tensor); it selects the order "priority" and goes with no other.  Behind the passes of Selector.cluster.
        Returns a dict: "rep_of" [n], "values" [n] float64 (1.0 for a representative), "clusters" [n] (dense id, by ascending
        representative rank), "degrees" [n], "sizes" [C], "representatives" [C] -- numpy arrays, or torch tensors on the device with
        to_host=False -- "n_clusters" = C and "rounds" (launch rounds the selection took)"""
        import torch
        if priority is not None and order == "max_degree":
            order = "priority"
        code = order_code(order)
        if (code == REP_PRIORITY) != (priority is not None):
            raise ValueError("priority: the scores of order 'priority', and of no other order")
        dev = torch.device("cuda", self.device)
        prio = None
        if priority is not None:
            if hasattr(priority, "data_ptr"):
                prio = priority.to(dev).contiguous()
                assert prio.dtype in (torch.int32, torch.uint32) and prio.numel() == self.n, "priority: n 32-bit scores"
            else:
                host = np.asarray(priority)
                if host.shape != (self.n,) or host.dtype.kind not in "iu" or (host.size and (host.min() < 0 or host.max() > 0xFFFFFFFF)):
                    raise ValueError("priority: n unsigned 32-bit scores")
                prio = torch.from_numpy(host.astype(np.uint32).view(np.int32)).to(dev)
        mv = float("-inf") if min_value is None else float(min_value)
        bufs = [torch.empty(self.n, dtype=torch.float64 if j == 1 else torch.int32, device=dev) for j in range(6)]
        out = Greedy(*[b.data_ptr() if self.n else None for b in bufs])
        cnt = C.c_int64()
        check(self._lib.selhip_ctx_cluster_greedy(self._ctx, mv, code, prio.data_ptr() if prio is not None and self.n else None, C.byref(out), C.byref(cnt)),
              self._ctx)
        c = int(cnt.value)
        res = {"rep_of": bufs[0], "values": bufs[1], "clusters": bufs[2], "degrees": bufs[3], "sizes": bufs[4][:c], "representatives": bufs[5][:c]}
        if to_host:
            res = {k: v.cpu().numpy() for k, v in res.items()}
        res["n_clusters"] = c
        res["rounds"] = self.get_param("greedy_rounds_last")
        return res

    def spanning_forest(self, min_value: Optional[float] = None, to_host: bool = True) -> dict:
        """the maximum spanning forest of the result list the context holds, computed on the device (selhip_ctx_spanning_forest): the
        single-linkage dendrogram of the graph on the n ranks whose edges are the records with value >= min_value (None: every
        record).  Its F = n - C edges, best first (greater value first, equal values by ascending (a, b)), are the merges of the
        hierarchy: the clusters at any threshold t are the components of the edges with value >= t (forest_cut), their number n minus
        the number of such edges (forest_cluster_counts), and forest_linkage gives SciPy's linkage matrix.  Behind the passes of
        Selector.cluster.  Returns a dict: "edges" [F] PAIR_DTYPE records {i = a < k = b, jaccard = value}, "labels" [n] int32 (smallest
        rank of the component: Selector.cluster's labels at the same min_value) -- numpy arrays; with to_host=False torch tensors on the
        device, the edges as uint8 [F, 16] (the records' bytes) --, "n_edges" = F, "n_clusters" = n - F and "rounds" (launch rounds, the
        empty last one included)"""
        import torch
        mv = float("-inf") if min_value is None else float(min_value)
        dev = torch.device("cuda", self.device)
        edges = torch.empty((max(self.n - 1, 0), PAIR_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        labels = torch.empty(self.n, dtype=torch.int32, device=dev)
        out = Forest(edges.data_ptr() if edges.numel() else None, labels.data_ptr() if self.n else None)
        cnt = C.c_int64()
        check(self._lib.selhip_ctx_spanning_forest(self._ctx, mv, C.byref(out), C.byref(cnt)), self._ctx)
        return _forest_result(edges, labels, int(cnt.value), self.n, self.get_param("forest_rounds_last"), to_host)

    # -- hierarchy of the dense matrix ------------------------------------------------------------------
    def linkage(self, measure="jaccard", method="average", max_height: Optional[float] = None, distance=None, to_host: bool = True) -> dict:
        """the agglomerative hierarchy of the context's set under the distance 1 - measure, computed on the device from the dense
        matrix (selhip_ctx_linkage): measure "jaccard", "max_containment" or "smh_jaccard" (the symmetric similarities; a NaN cell --
        two empty sketches -- is distance 1.0), method "single", "complete", "average" (UPGMA) or "weighted" (WPGMA), max_height: no
        merge above it (None: the whole tree).  distance: a callable applied to the device tensor of Selector.matrix(measure) --
        `lambda j: -torch.log(2 * j / (1 + j)) / 21` is the Mash distance -- whose result goes to `linkage` in place of 1 - measure
        (only its strict upper triangle is read; NaN and -inf there raise).  Returns a dict: "merges" [F] PAIR_DTYPE records {i = a <
        k = b, jaccard = height} in rank indices -- the cluster of a merge lives on as a, the smallest rank among its members --
        in emitted order (children before parents), "sizes" [F] int32 -- numpy arrays; with to_host=False torch tensors on the device,
        the merges as uint8 [F, 16] --, "n_merges" = F and "rounds".  linkage_matrix gives SciPy's matrix, linkage_cut the labels at a
        height (they go into Selector.merge), linkage_newick a tree"""
        import torch
        if distance is not None:
            return linkage(distance(self.matrix(measure)), method, max_height, overwrite=True, device=self.device, to_host=to_host)
        code, mh = linkage_code(method), _max_height(max_height)
        dev = torch.device("cuda", self.device)
        merges = torch.empty((max(self.n - 1, 0), PAIR_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        sizes = torch.empty(max(self.n - 1, 0), dtype=torch.int32, device=dev)
        out = Linkage(merges.data_ptr() if merges.numel() else None, sizes.data_ptr() if sizes.numel() else None)
        cnt = C.c_int64()
        check(self._lib.selhip_ctx_linkage(self._ctx, measure_code(measure), code, mh, C.byref(out), C.byref(cnt)), self._ctx)
        return _linkage_result(merges, sizes, int(cnt.value), self.get_param("linkage_rounds_last"), to_host)

    # -- sketches merged by group ---------------------------------------------------------------------
    def merge(self, groups, n_groups: Optional[int] = None, to_host: bool = False) -> dict:
        """one union sketch per group of the context's set, merged on the device (selhip_ctx_merge_groups): the element-wise maximum of
        the members' HLL registers and the unsigned minimum of their SuperMinHash buckets -- bit for bit the sketches of the members'
        records concatenated.  groups: n int32 ids in rank order, -1 .. n_groups - 1 (-1 = in no group; a numpy array or a torch int32
        device tensor), or the dict Selector.cluster / cluster_greedy returned (its "clusters" and "n_clusters").  n_groups None: the
        largest id + 1.  Returns a dict, rows in group-id order: "hll" [G, 1 << p_hll] uint8, "aux" [G, m] (int64 view of the u64
        buckets as a tensor, uint64 as a numpy array), "aux_hll" [G, 1 << p_aux] uint8 or None where the context holds no auxiliary
        sketches, "cards" [G] float64 (report() of the merged main registers; 0 for an empty group), "sizes" [G] int32 -- torch tensors
        on the device, or numpy arrays with to_host=True.  An id outside [-1, n_groups) raises (SELHIP_E_BADARG)"""
        import torch
        dev = torch.device("cuda", self.device)
        if isinstance(groups, dict):
            n_groups = groups["n_clusters"] if n_groups is None else n_groups
            groups = groups["clusters"]
        if not hasattr(groups, "data_ptr"):
            groups = torch.from_numpy(np.ascontiguousarray(groups, dtype=np.int32)).to(dev)
        groups = groups.to(dev).contiguous()
        assert groups.dtype == torch.int32 and groups.dim() == 1 and groups.numel() == self.n, "groups: n int32 ids in rank order"
        if n_groups is None:
            n_groups = int(groups.max().item()) + 1 if self.n else 0
        g = int(n_groups)
        with torch.cuda.device(dev):
            hll = torch.empty((max(g, 0), 1 << self.p_hll), dtype=torch.uint8, device=dev)
            aux = torch.empty((max(g, 0), self.m), dtype=torch.int64, device=dev)
            aux_hll = torch.empty((max(g, 0), 1 << self.p_aux), dtype=torch.uint8, device=dev) if self.p_aux else None
            cards = torch.empty(max(g, 0), dtype=torch.float64, device=dev)
            sizes = torch.empty(max(g, 0), dtype=torch.int32, device=dev)
            ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
            out = Merged(ptr(hll), ptr(aux), ptr(aux_hll), ptr(cards), ptr(sizes))
            check(self._lib.selhip_ctx_merge_groups(self._ctx, ptr(groups), g, C.byref(out)), self._ctx)
        res = {"hll": hll, "aux": aux, "aux_hll": aux_hll, "cards": cards, "sizes": sizes}
        if to_host:
            res = {k: None if v is None else v.cpu().numpy() for k, v in res.items()}
            res["aux"] = res["aux"].view(np.uint64)
        return res

    def result_count(self) -> int:
        return int(check(self._lib.selhip_ctx_result_count(self._ctx), self._ctx))

    def fetch(self) -> np.ndarray:
        cnt = self.result_count()
        out = np.zeros(cnt, dtype=PAIR_DTYPE)
        check(self._lib.selhip_ctx_fetch(self._ctx, out.ctypes.data if cnt else None, cnt), self._ctx)
        return out

    def result_device(self) -> Tuple[int, int]:
        """(device pointer to the unsorted selhip_pair_t list, count)"""
        p, cnt = C.c_void_p(), C.c_int64()
        check(self._lib.selhip_ctx_result_device(self._ctx, C.byref(p), C.byref(cnt)), self._ctx)
        return (p.value or 0), cnt.value

    def copy_results_to(self, tensor) -> int:
        """D2D copy of the unsorted result records into a torch CUDA uint8/any tensor (>= 16 B per record)."""
        cap = tensor.numel() * tensor.element_size() // PAIR_DTYPE.itemsize
        check(self._lib.selhip_ctx_copy_results(self._ctx, tensor.data_ptr(), cap), self._ctx)
        return min(cap, self.result_count())

    def copy_results_framed(self, tensor) -> int:
        """D2D: tensor[0] (16 B) = {count, 0}, records from tensor[1:]; returns the (host-known) count"""
        cap = tensor.numel() * tensor.element_size() // PAIR_DTYPE.itemsize - 1
        rc = self._lib.selhip_ctx_copy_results_framed(self._ctx, tensor.data_ptr(), cap)
        if rc not in (0, -3):
            check(rc, self._ctx)
        return self.result_count()

    def copy_results_framed_async(self, tensor):
        """the same frame enqueued behind a pass that is still running (between run_async and finish): header from the
        device-side counter, payload = the whole capacity of `tensor`; check result_count() and last_attempts() after finish"""
        cap = tensor.numel() * tensor.element_size() // PAIR_DTYPE.itemsize - 1
        check(self._lib.selhip_ctx_copy_results_framed_async(self._ctx, tensor.data_ptr(), cap), self._ctx)
        return cap

    def last_attempts(self) -> int:
        return int(check(self._lib.selhip_ctx_last_attempts(self._ctx), self._ctx))

    def stats(self) -> dict:
        st = (C.c_int64 * 4)()
        check(self._lib.selhip_ctx_stats(self._ctx, st), self._ctx)
        return {"evaluated": st[0], "survivors": st[1], "selected": st[2], "candidates": st[3]}

    def timing(self, enable=True):
        """False/0 = off, True/1 = every kernel scope, 2 = only the dominant stage-1 kernel (resets the figures)"""
        check(self._lib.selhip_ctx_timing(self._ctx, int(enable)), self._ctx)

    def kernel_ms(self, name: str) -> float:
        """device ms per pass spent in the named kernel (sum over its launches of one pass)"""
        return float(self._lib.selhip_ctx_kernel_ms(self._ctx, name.encode()))

    def kernel_launches(self, name: str) -> float:
        return float(self._lib.selhip_ctx_kernel_launches(self._ctx, name.encode()))


REPS = {"max_degree": REP_MAX_DEGREE, "min_rank": REP_MIN_RANK, "max_rank": REP_MAX_RANK}


def rep_code(rep) -> int:
    """the SELHIP_REP_* code of a representative rule given by name or by code; ValueError for anything else"""
    code = REPS.get(rep) if isinstance(rep, str) else rep
    if isinstance(code, bool) or not isinstance(code, (int, np.integer)) or code not in REPS.values():
        raise ValueError("rep: 'max_degree', 'min_rank' or 'max_rank'")
    return int(code)


ORDERS = dict(REPS, priority=REP_PRIORITY)


def order_code(order) -> int:
    """the SELHIP_REP_* code of a visiting order of the greedy clusters given by name or by code; ValueError for anything else"""
    code = ORDERS.get(order) if isinstance(order, str) else order
    if isinstance(code, bool) or not isinstance(code, (int, np.integer)) or code not in ORDERS.values():
        raise ValueError("order: 'max_degree', 'min_rank', 'max_rank' or 'priority'")
    return int(code)


def _device_pairs(pairs, dev):
    import torch
    if isinstance(pairs, np.ndarray) or not hasattr(pairs, "data_ptr"):
        pairs = torch.from_numpy(np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)).to(dev)
    assert pairs.is_cuda and pairs.is_contiguous() and pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 2, \
        "pairs: a contiguous int32 tensor of shape (P, 2)"
    return pairs


def greedy_representatives(pairs, n: int, keys=None, device: int = 0, to_host: bool = True):
    """(is_rep [n] uint8, rounds): the representatives of the greedy clustering over the undirected graph on the vertices 0 .. n - 1 with
    one edge per row of `pairs` (a numpy int32 (P, 2) array or a torch int32 device tensor of that shape), computed on the device
    (selhip_greedy_representatives): visit the vertices by descending keys[g] (n unsigned 64-bit keys, numpy; equal keys: the smaller
    vertex first; None: key = vertex); a vertex is a representative unless a neighbour already is one.  Self-loops and repeated rows are
    legal; a vertex outside [0, n) raises (SELHIP_E_BADARG).  rounds: the launch rounds the selection took.  is_rep is a numpy array, or
    a torch tensor on the device with to_host=False"""
    import torch
    lib = hip_lib()
    dev = torch.device("cuda", device)
    pairs = _device_pairs(pairs, dev)
    key = None
    if keys is not None:
        host = np.ascontiguousarray(keys, dtype=np.uint64)
        if host.shape != (int(n),):
            raise ValueError("keys: n unsigned 64-bit keys")
        key = torch.from_numpy(host.view(np.int64)).to(dev)
    rounds = C.c_int64(-1)
    with torch.cuda.device(dev):
        is_rep = torch.empty(int(n), dtype=torch.uint8, device=dev)
        check(lib.selhip_greedy_representatives(pairs.data_ptr() if pairs.numel() else None, int(pairs.shape[0]), int(n),
                                                key.data_ptr() if key is not None and n else None, is_rep.data_ptr() if n else None,
                                                C.byref(rounds), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return (is_rep.cpu().numpy() if to_host else is_rep), int(rounds.value)


def merge_sketches(hll=None, smh=None, aux_hll=None, groups=None, n_groups: Optional[int] = None, device: Optional[int] = 0):
    """sketch rows merged by group (selhip_merge_sketches; device=None: the host twin selhost_merge_sketches, no GPU needed): hll [n, 1 << p]
    uint8, smh [n, m] uint64 and aux_hll [n, 1 << p_aux] uint8 -- numpy arrays, any of them None -- reduced to n_groups rows each by
    groups [n] (int32, -1 .. n_groups - 1, -1 = in no group; n_groups None: the largest id + 1): maximum of the registers, unsigned minimum of
    the buckets.  Returns a dict of numpy arrays "hll", "smh", "aux_hll" (None where not given) and "sizes" [n_groups] int32.  An id outside
    [-1, n_groups) raises and writes nothing"""
    if groups is None:
        raise ValueError("groups: one int32 id per row")
    groups = np.ascontiguousarray(groups, dtype=np.int32)
    n = groups.shape[0]
    if n_groups is None:
        n_groups = int(groups.max()) + 1 if n else 0
    g = max(int(n_groups), 0)
    rows = {}
    for key, arr, dt in (("hll", hll, np.uint8), ("smh", smh, np.uint64), ("aux_hll", aux_hll, np.uint8)):
        if arr is not None:
            arr = np.ascontiguousarray(arr, dtype=dt)
            if arr.ndim != 2 or arr.shape[0] != n:
                raise ValueError(f"{key}: a 2-D array of {n} rows, got shape {arr.shape}")
            if dt == np.uint8 and (arr.shape[1] < 16 or arr.shape[1] & (arr.shape[1] - 1)):
                raise ValueError(f"{key} must be [n, 1 << p] with p in 4..20, got shape {arr.shape}")
        rows[key] = arr
    p = rows["hll"].shape[1].bit_length() - 1 if rows["hll"] is not None else 14
    m = rows["smh"].shape[1] if rows["smh"] is not None else 0
    p_aux = rows["aux_hll"].shape[1].bit_length() - 1 if rows["aux_hll"] is not None else 0
    if device is None:
        outs = {k: None if v is None else np.empty((g, v.shape[1]), dtype=v.dtype) for k, v in rows.items()}
        sizes = np.empty(g, dtype=np.int32)
        ptr = lambda a: None if a is None else a.ctypes.data
        rc = host_lib().selhost_merge_sketches(ptr(rows["hll"]), ptr(rows["smh"]), ptr(rows["aux_hll"]), n, p, m, p_aux, groups.ctypes.data, int(n_groups),
                                               ptr(outs["hll"]), ptr(outs["smh"]), ptr(outs["aux_hll"]), sizes.ctypes.data)
        if rc < 0:
            raise ValueError(host_lib().selhost_last_error().decode())
        return {**outs, "sizes": sizes}
    import torch
    dev = torch.device("cuda", device)
    def to_dev(a):                                                           # (one spare row: a kind is present by its pointer, n == 0 included)
        if a is None:
            return None
        a = a.view(np.int64) if a.dtype == np.uint64 else a
        return torch.from_numpy(np.concatenate([a, np.zeros((1, a.shape[1]), dtype=a.dtype)])).to(dev)
    with torch.cuda.device(dev):
        d_in = {k: to_dev(v) for k, v in rows.items()}
        d_out = {k: None if v is None else torch.empty((g + 1, v.shape[1]), dtype=v.dtype, device=dev) for k, v in d_in.items()}
        d_groups = torch.from_numpy(np.concatenate([groups, np.zeros(1, dtype=np.int32)])).to(dev)
        d_sizes = torch.empty(g + 1, dtype=torch.int32, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None
        check(hip_lib().selhip_merge_sketches(ptr(d_in["hll"]), ptr(d_in["smh"]), ptr(d_in["aux_hll"]), n, p, m, p_aux, ptr(d_groups), int(n_groups),
                                              ptr(d_out["hll"]), ptr(d_out["smh"]), ptr(d_out["aux_hll"]), ptr(d_sizes),
                                              C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    res = {k: None if v is None else v[:g].cpu().numpy() for k, v in d_out.items()}
    if res["smh"] is not None:
        res["smh"] = res["smh"].view(np.uint64)
    res["sizes"] = d_sizes[:g].cpu().numpy()
    return res


def selector_from_rows(hll_t, aux_t, cards_t, aux_hll_t=None, device: int = 0, fp_mode: int = FP_FMA):
    """(Selector, order): sketch rows that lie on the device in any order -- the rows Selector.merge returns, in group-id order -- as the
    set of a new Selector: sorted by cards (sort_by_card, the reference's order), gathered with selhip_permute_rows and attached.
    hll_t uint8 [n, 1 << p], aux_t int64 [n, m], cards_t float64 [n], aux_hll_t uint8 [n, 1 << p_aux] or None; order[rank] = the row the
    genome of that rank came from"""
    import torch
    lib = hip_lib()
    dev = torch.device("cuda", device)
    n = int(hll_t.shape[0])
    order = sort_by_card(cards_t.cpu().numpy())
    with torch.cuda.device(dev):
        perm = torch.from_numpy(order).to(dev)
        st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def gather(t):
            out = torch.empty_like(t)
            if n and t.shape[1]:
                check(lib.selhip_permute_rows(t.data_ptr(), out.data_ptr(), perm.data_ptr(), n, t.shape[1] * t.element_size(), st))
            return out
        hll_s, aux_s = gather(hll_t.contiguous()), gather(aux_t.contiguous())
        aux_hll_s = gather(aux_hll_t.contiguous()) if aux_hll_t is not None else None
        cards_s = cards_t[perm.long()].contiguous()
        torch.cuda.current_stream(dev).synchronize()
    sel = Selector(device, fp_mode)
    sel.attach(hll_s, aux_s, cards_s, p_hll=int(hll_t.shape[1]).bit_length() - 1)
    if aux_hll_s is not None:
        sel.attach_aux_hll(aux_hll_s, int(aux_hll_t.shape[1]).bit_length() - 1)
    return sel, order


def read_groups(groups_file: str, names: Sequence[str]):
    """(groups [n] int32 in the order of `names`, group names): a groups file of lines 'path<TAB>group_name' (what `selection -I` reads);
    groups are numbered by first appearance, a genome that is not listed belongs to no group (-1).  ValueError with the line number for a
    path that is not in names, a line without a tab, an empty group name or one containing '/'"""
    rank = {nm: r for r, nm in enumerate(names)}
    groups = np.full(len(names), -1, dtype=np.int32)
    ids: dict = {}
    with open(groups_file) as f:
        for ln, line in enumerate(f, 1):
            line = line.rstrip("\n")
            if not line:
                continue
            path, tab, gname = line.partition("\t")
            if not tab or path not in rank:
                raise ValueError(f"{groups_file}:{ln}: expected 'path<TAB>group_name' with a path of the file list")
            if not gname or "/" in gname:
                raise ValueError(f"{groups_file}:{ln}: a group name is not empty and holds no '/'")
            groups[rank[path]] = ids.setdefault(gname, len(ids))
    return groups, list(ids)


def write_merged(out_dir: str, group_names: Sequence[str], merged: dict, m: int, p_aux: int = 0):
    """writes one sketch set per group of `merged` (Selector.merge(..., to_host=True)) into out_dir the way `selection -P` does:
    <name>.hll, <name>.smh<m> (m > 0), <name>.hll_<p_aux> (p_aux > 0) through selhost_write_hll / selhost_write_smh, and filelist.txt with one
    out_dir/<name> per line in group order"""
    import os
    h = host_lib()
    os.makedirs(out_dir, exist_ok=True)
    hll = np.ascontiguousarray(merged["hll"], dtype=np.uint8)
    lines = []
    for c, gname in enumerate(group_names):
        base = os.path.join(out_dir, gname)
        rc = h.selhost_write_hll((base + ".hll").encode(), hll[c].ctypes.data, hll.shape[1].bit_length() - 1)
        if not rc and m:
            row = np.ascontiguousarray(merged["aux"][c], dtype=np.uint64)
            rc = h.selhost_write_smh((base + f".smh{m}").encode(), row.ctypes.data, m)
        if not rc and p_aux:
            row = np.ascontiguousarray(merged["aux_hll"][c], dtype=np.uint8)
            rc = h.selhost_write_hll((base + f".hll_{p_aux}").encode(), row.ctypes.data, p_aux)
        if rc:
            raise RuntimeError(h.selhost_last_error().decode())
        lines.append(base + "\n")
    with open(os.path.join(out_dir, "filelist.txt"), "w") as f:
        f.writelines(lines)


def cluster_names(n_clusters: int) -> list:
    """the names `selection -L ... -P dir` gives the clusters: cluster_<id>, zero-padded to the width of n_clusters - 1"""
    width = len(str(max(n_clusters - 1, 0)))
    return [f"cluster_{c:0{width}d}" for c in range(n_clusters)]


def merge_from_filelist(list_file: str, aux_bytes: int, groups_file: Optional[str] = None, out_dir: Optional[str] = None, tau: float = 0.9,
                        mode: int = MODE_CB_SMH, device: int = 0, fp_mode: int = FP_FMA, algo: int = ALGO_AUTO, criterion: str = "smh_a",
                        linkage: str = "single", cluster_min: Optional[float] = None, rep="max_degree", fold_aux: bool = False, **pass_args) -> dict:
    """one merged sketch set per group of the genomes of a file list.  groups_file ('path<TAB>group_name' lines, read_groups; what
    `selection -I` reads): no pass runs.  Without it the groups are the clusters of the pass of select_from_filelist (tau, criterion and
    its other arguments), single-linkage (Selector.cluster, rep) or linkage="greedy" (Selector.cluster_greedy, order = rep) at
    cluster_min -- what `selection -L file [-Z greedy] -P dir` merges.  out_dir: the sets are also written as files (write_merged).
    Returns Selector.merge's dict on the host plus "names" (the groups' names), "groups" [n] in rank order and "genomes" (the genome names in
    rank order)"""
    m_crit, p_aux, _ = _criterion_files(criterion, aux_bytes, pass_args.get("min_matches"), pass_args.get("min_containment"))
    m = aux_bytes // 8 if criterion in ("smh_a", "smh_c") else m_crit

    def finish(ds, sel, groups, names):
        res = sel.merge(groups, len(names), to_host=True)
        if out_dir is not None:
            write_merged(out_dir, names, res, sel.m if m else 0, sel.p_aux)
        res.update(names=names, groups=np.asarray(groups), genomes=list(ds.names))
        return res

    if groups_file is not None:
        ds = load_dataset(list_file, m, _aux_files(fold_aux, p_aux, criterion) if p_aux else 0, fp_mode)
        groups, names = read_groups(groups_file, ds.names)
        with Selector(device, fp_mode) as sel:
            sel.upload(ds.hll, ds.aux if m else np.zeros((len(ds.names), 1), dtype=np.uint64), ds.cards)
            if p_aux and fold_aux:
                sel.fold_aux_hll(p_aux)
            elif p_aux:
                sel.upload_aux_hll(ds.aux_hll, p_aux)
            return finish(ds, sel, groups, names)

    def then(ds, sel, pairs):
        res = sel.cluster_greedy(cluster_min, rep) if linkage == "greedy" else sel.cluster(cluster_min, rep)
        return finish(ds, sel, res["clusters"], cluster_names(res["n_clusters"]))
    if linkage not in ("single", "greedy"):
        raise ValueError("linkage: 'single' or 'greedy'")
    return _filelist_pass(then, list_file, tau, aux_bytes, mode, device, fp_mode, algo, criterion, fold_aux=fold_aux, **pass_args)


def greedy_table(names: Sequence[str], order: np.ndarray, res: dict) -> str:
    """the text of `selection -L file -Z greedy`: one line per genome in FILE-LIST order, 'path<TAB>cluster<TAB>cluster_size<TAB>degree
    <TAB>representative_path<TAB>value_to_representative' (the value with six decimals, as std::to_string prints it).  names in rank
    order, order[rank] = the genome's line in the list, res = Selector.cluster_greedy(...) on the host"""
    out = []
    for r in np.argsort(np.asarray(order), kind="stable"):
        c = int(res["clusters"][r])
        out.append(f"{names[r]}\t{c}\t{int(res['sizes'][c])}\t{int(res['degrees'][r])}\t{names[int(res['rep_of'][r])]}\t{float(res['values'][r]):f}\n")
    return "".join(out)


def components(pairs, n: int, device: int = 0, to_host: bool = True):
    """labels [n] int32 of the connected components of the undirected graph on the vertices 0 .. n - 1 with one edge per row of `pairs`
    (a numpy int32 (P, 2) array or a torch int32 device tensor of that shape): labels[g] = the smallest vertex of g's component, computed
    on the device (selhip_components).  Self-loops and repeated rows are legal; a vertex outside [0, n) raises (SELHIP_E_BADARG, the
    message names one such row).  A numpy array, or a torch tensor on the device with to_host=False"""
    import torch
    lib = hip_lib()
    dev = torch.device("cuda", device)
    pairs = _device_pairs(pairs, dev)
    with torch.cuda.device(dev):
        labels = torch.empty(int(n), dtype=torch.int32, device=dev)
        check(lib.selhip_components(pairs.data_ptr() if pairs.numel() else None, int(pairs.shape[0]), int(n),
                                    labels.data_ptr() if n else None, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return labels.cpu().numpy() if to_host else labels


def _forest_result(edges, labels, f: int, n: int, rounds: int, to_host: bool) -> dict:
    """the dict of Selector.spanning_forest / spanning_forest from the device tensors a call filled: its first f edge records and the labels"""
    res = {"edges": edges[:f], "labels": labels}
    if to_host:
        res = {"edges": np.ascontiguousarray(edges[:f].cpu().numpy()).view(PAIR_DTYPE).reshape(-1), "labels": labels.cpu().numpy()}
    res.update(n_edges=f, n_clusters=n - f, rounds=rounds)
    return res


def spanning_forest(pairs, n: int, values=None, device: int = 0, to_host: bool = True) -> dict:
    """the maximum spanning forest of the undirected graph on the vertices 0 .. n - 1 with one edge per row of `pairs` (a numpy int32
    (P, 2) array or a torch int32 device tensor of that shape) and values[e] as its value (P float64 numbers, numpy or a torch device
    tensor; None: every value 1.0, the order is then the pair order), computed on the device (selhip_spanning_forest).  A NaN value is
    no edge; self-loops and repeated rows are legal (a repeated pair counts once, with its greatest value); a vertex outside [0, n)
    raises (SELHIP_E_BADARG).  The dict of Selector.spanning_forest"""
    import torch
    lib = hip_lib()
    dev = torch.device("cuda", device)
    pairs = _device_pairs(pairs, dev)
    vals = None
    if values is not None:
        vals = values if hasattr(values, "data_ptr") else torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64)).to(dev)
        assert vals.is_cuda and vals.is_contiguous() and vals.dtype == torch.float64 and vals.shape == (pairs.shape[0],), "values: P float64 numbers"
    n = int(n)
    f, rounds = C.c_int64(-1), C.c_int64(-1)
    with torch.cuda.device(dev):
        edges = torch.empty((max(n - 1, 0), PAIR_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        labels = torch.empty(max(n, 0), dtype=torch.int32, device=dev)
        check(lib.selhip_spanning_forest(pairs.data_ptr() if pairs.numel() else None, vals.data_ptr() if vals is not None and vals.numel() else None,
                                         int(pairs.shape[0]), n, edges.data_ptr() if edges.numel() else None, labels.data_ptr() if n > 0 else None,
                                         C.byref(f), C.byref(rounds), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return _forest_result(edges, labels, int(f.value), n, int(rounds.value), to_host)


def forest_cluster_counts(edges, n: int, thresholds) -> np.ndarray:
    """the number of single-linkage clusters at every threshold t of `thresholds`, from the forest's edges alone (a PAIR_DTYPE array,
    Selector.spanning_forest's "edges"): n - #{edges with value >= t}, int64"""
    v = np.asarray(edges["jaccard"], dtype=np.float64)
    return np.array([int(n) - int(np.count_nonzero(v >= float(t))) for t in np.atleast_1d(np.asarray(thresholds, dtype=np.float64))], dtype=np.int64)


def forest_cut(edges, n: int, t: float, device: int = 0) -> np.ndarray:
    """labels [n] int32 of the single-linkage clusters at threshold t from the forest's edges (a PAIR_DTYPE array in the forest's order):
    the components (on the device, `components`) of the prefix of edges with value >= t -- Selector.cluster(min_value=t)'s labels"""
    keep = np.asarray(edges["jaccard"], dtype=np.float64) >= float(t)
    pairs = np.stack([np.asarray(edges["i"])[keep], np.asarray(edges["k"])[keep]], axis=1).astype(np.int32).reshape(-1, 2)
    return components(pairs, n, device)


def forest_linkage(edges, n: int, distance=lambda v: 1.0 - v, fill: Optional[float] = None) -> np.ndarray:
    """the linkage matrix Z of scipy.cluster.hierarchy (float64 [n - 1, 4]) from the forest's edges in their order (a PAIR_DTYPE array):
    row s merges the clusters of the edge's two ends into the new cluster n + s -- columns: the smaller id, the larger id,
    distance(value), the size of the new cluster; an original observation g has the id g.  A forest of C > 1 components has only
    n - C merges: ValueError with fill None; otherwise the remaining components are joined in ascending label order (smallest rank),
    each to the cluster that holds the smallest one, at distance `fill`"""
    n = int(n)
    parent, cid, size = list(range(n)), list(range(n)), [1] * n

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    z = []

    def join(a, b, d):
        ra, rb = find(a), find(b)
        if ra == rb:
            raise ValueError("forest_linkage: the edges close a cycle (not a forest)")
        ia, ib = cid[ra], cid[rb]
        lo, hi = min(ra, rb), max(ra, rb)
        parent[hi] = lo
        size[lo] += size[hi]
        cid[lo] = n + len(z)
        z.append([float(min(ia, ib)), float(max(ia, ib)), float(d), float(size[lo])])

    for e in edges:
        join(int(e["i"]), int(e["k"]), distance(float(e["jaccard"])))
    roots = sorted({find(g) for g in range(n)})            # (the root is the smallest rank: the label)
    if len(roots) > 1:
        if fill is None:
            raise ValueError(f"forest_linkage: the forest has {len(roots)} components; give fill, the distance at which they are joined")
        for r in roots[1:]:
            join(roots[0], r, fill)
    return np.array(z, dtype=np.float64).reshape(-1, 4)


def forest_table(names: Sequence[str], edges) -> str:
    """the text of `selection -H`: one line per forest edge in the forest's order, 'path_a<TAB>path_b<TAB>value', the value printed as
    format_lines prints J.  names in rank order, edges = Selector.spanning_forest(...)["edges"] on the host"""
    return "".join(f"{names[int(e['i'])]}\t{names[int(e['k'])]}\t{float(e['jaccard']):f}\n" for e in edges)


LINKAGES = {"single": LINKAGE_SINGLE, "complete": LINKAGE_COMPLETE, "average": LINKAGE_AVERAGE, "weighted": LINKAGE_WEIGHTED}


def linkage_code(method) -> int:
    """the SELHIP_LINKAGE_* code of a method given by name or by code; ValueError for anything else"""
    code = LINKAGES.get(method) if isinstance(method, str) else method
    if isinstance(code, bool) or not isinstance(code, (int, np.integer)) or code not in LINKAGES.values():
        raise ValueError("method: 'single', 'complete', 'average' or 'weighted'")
    return int(code)


def _max_height(max_height) -> float:
    mh = float("inf") if max_height is None else float(max_height)
    if np.isnan(mh):
        raise ValueError("max_height: a number (None builds the whole hierarchy), not NaN")
    return mh


def _linkage_result(merges, sizes, f: int, rounds: int, to_host: bool) -> dict:
    """the dict of Selector.linkage / linkage from the device tensors a call filled: their first f entries"""
    res = {"merges": merges[:f], "sizes": sizes[:f]}
    if to_host:
        res = {"merges": np.ascontiguousarray(merges[:f].cpu().numpy()).view(PAIR_DTYPE).reshape(-1), "sizes": sizes[:f].cpu().numpy()}
    res.update(n_merges=f, rounds=rounds)
    return res


def linkage(dist, method="average", max_height: Optional[float] = None, overwrite: bool = False, device: int = 0, to_host: bool = True) -> dict:
    """the agglomerative hierarchy of an n x n distance matrix, computed on the device (selhip_linkage): dist a numpy float64 array or
    a torch float64 tensor (2-D, square, stride(1) == 1; its stride(0) is the leading dimension) of which only the strict upper
    triangle is read -- a NaN or -inf there raises (SELHIP_E_BADARG), +inf is legal.  The call consumes the matrix it works on: a
    device tensor is cloned first unless overwrite=True.  method, max_height and the dict: Selector.linkage's"""
    import torch
    lib = hip_lib()
    code, mh = linkage_code(method), _max_height(max_height)
    dev = torch.device("cuda", device)
    if hasattr(dist, "data_ptr"):
        d = dist if dist.is_cuda and overwrite else dist.to(dev, copy=True)
    else:
        d = torch.from_numpy(np.ascontiguousarray(dist, dtype=np.float64)).to(dev)
    assert d.dim() == 2 and d.shape[0] == d.shape[1] and d.dtype == torch.float64, "dist: a square float64 matrix"
    n = int(d.shape[0])
    assert n <= 1 or d.stride(1) == 1, "dist: stride(1) must be 1"
    ld = d.stride(0) if n > 1 else max(n, 1)
    f, rounds = C.c_int64(-1), C.c_int64(-1)
    with torch.cuda.device(dev):
        merges = torch.empty((max(n - 1, 0), PAIR_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        sizes = torch.empty(max(n - 1, 0), dtype=torch.int32, device=dev)
        check(lib.selhip_linkage(d.data_ptr() if n else None, n, ld, code, mh, merges.data_ptr() if merges.numel() else None,
                                 sizes.data_ptr() if sizes.numel() else None, C.byref(f), C.byref(rounds),
                                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return _linkage_result(merges, sizes, int(f.value), int(rounds.value), to_host)


def _linkage_order(merges) -> list:
    """the emitted positions of the merges ordered by the key max(own height, children's keys), ties by position: children stay in
    front of their parents even where rounding makes a parent an ulp lower"""
    last, key = {}, []
    for s, e in enumerate(merges):
        a, b = int(e["i"]), int(e["k"])
        k = float(e["jaccard"])
        for c in (last.get(a), last.get(b)):
            if c is not None and key[c] > k:
                k = key[c]
        key.append(k)
        last[a] = s
    return sorted(range(len(key)), key=lambda s: (key[s], s))


def linkage_matrix(merges, sizes, n: int, fill: Optional[float] = None) -> np.ndarray:
    """the linkage matrix Z of scipy.cluster.hierarchy (float64 [n - 1, 4]; what fcluster and dendrogram take) from the merges and
    sizes of Selector.linkage / linkage: row s merges two clusters into the new cluster n + s -- columns: the smaller id, the larger
    id, the height, the size; an original observation g has the id g.  The rows are ordered by the key max(own height, children's
    keys), ties by emitted position.  A capped call leaves C > 1 roots: ValueError with fill None; otherwise they are joined in
    ascending slot order, each to the cluster that holds the smallest one, at height `fill` (as forest_linkage does)"""
    n = int(n)
    cid, size = {}, {}
    z = []

    def join(a, b, h, s):
        ia, ib = cid.get(a, a), cid.get(b, b)
        cid[a] = n + len(z)
        size[a] = s
        z.append([float(min(ia, ib)), float(max(ia, ib)), float(h), float(s)])

    dead = set()
    for s in _linkage_order(merges):
        e = merges[s]
        join(int(e["i"]), int(e["k"]), float(e["jaccard"]), int(sizes[s]))
        dead.add(int(e["k"]))
    roots = [g for g in range(n) if g not in dead]
    if len(roots) > 1:
        if fill is None:
            raise ValueError(f"linkage_matrix: the hierarchy has {len(roots)} roots; give fill, the height at which they are joined")
        for r in roots[1:]:
            join(roots[0], r, fill, size.get(roots[0], 1) + size.get(r, 1))
    return np.array(z, dtype=np.float64).reshape(-1, 4)


def linkage_cut(merges, n: int, max_height: float, device: int = 0) -> np.ndarray:
    """labels [n] int32 (the smallest member) of the clusters of the hierarchy at max_height: the components (on the device,
    `components`) of the merges with height <= max_height.  They go into Selector.merge as they are"""
    keep = np.asarray(merges["jaccard"], dtype=np.float64) <= float(max_height)
    pairs = np.stack([np.asarray(merges["i"])[keep], np.asarray(merges["k"])[keep]], axis=1).astype(np.int32).reshape(-1, 2)
    return components(pairs, n, device)


def _newick_number(x: float) -> str:
    """the shortest of %.15g, %.16g, %.17g that reads back to the same double (what `selection -N` prints)"""
    for p in (15, 16, 17):
        s = "%.*g" % (p, x)
        if float(s) == x:
            break
    return s


def _newick_name(name: str) -> str:
    if name and not any(ch in name for ch in " ()[]':;,\t\n"):
        return name
    return "'" + name.replace("'", "''") + "'"


def linkage_newick(merges, sizes, names: Sequence[str], fill: Optional[float] = None) -> str:
    """the hierarchy as an ultrametric Newick tree, one line ending in ';': a node stands at its merge's height (a leaf at 0) and
    its branch has the length (parent's height - own height) / 2, not below 0; the subtree of a merge's a goes first.  names: the
    leaves' names in the merges' index space (rank order); a name with a blank or one of ()[]':;, is quoted.  A length is printed as
    the shortest of %.15g, %.16g, %.17g that reads back to the same double.  A capped hierarchy: fill, as linkage_matrix"""
    n = len(names)
    node = {g: (None, None, 0.0, g) for g in range(n)}            # slot -> (left, right, height, leaf)
    dead = set()

    def join(a, b, h):
        node[a] = (node[a], node[b], float(h), -1)
        dead.add(b)

    for e in merges:
        join(int(e["i"]), int(e["k"]), float(e["jaccard"]))
    roots = [g for g in range(n) if g not in dead]
    if len(roots) > 1:
        if fill is None:
            raise ValueError(f"linkage_newick: the hierarchy has {len(roots)} roots; give fill, the height at which they are joined")
        for r in roots[1:]:
            join(roots[0], r, fill)
    if n == 0:
        return ";\n"
    out, stack = [], [(node[roots[0]], None)]                    # (node, parent's height) or a literal
    while stack:
        item = stack.pop()
        if isinstance(item, str):
            out.append(item)
            continue
        (left, right, h, leaf), up = item
        tail = "" if up is None else ":" + _newick_number(max((up - h) / 2.0, 0.0))
        if leaf >= 0:
            out.append(_newick_name(str(names[leaf])) + tail)
        else:
            stack.extend([")" + tail, (right, h), ",", (left, h), "("])
    return "".join(out) + ";\n"


def linkage_table(names: Sequence[str], res: dict) -> str:
    """the text of `selection -J`: one line per merge in emitted order, 'path_a<TAB>path_b<TAB>height<TAB>size', the height with six
    decimals as format_lines prints J.  names in rank order, res = Selector.linkage(...) on the host"""
    return "".join(f"{names[int(e['i'])]}\t{names[int(e['k'])]}\t{float(e['jaccard']):f}\t{int(s)}\n" for e, s in zip(res["merges"], res["sizes"]))


def linkage_from_filelist(list_file: str, aux_bytes: int = 0, measure="jaccard", method="average", max_height: Optional[float] = None,
                          fill: Optional[float] = None, fp_mode: int = FP_FMA, device: int = 0) -> dict:
    """the hierarchy of the genomes of a file list -- what `selection -l list -N tree.nwk [-J merges.tsv] [-X method]` computes; no pass
    runs.  The sketches are loaded and sorted as for a selection (the HLL measures read only the .hll files, "smh_jaccard" also the
    .smh<m> files, m = aux_bytes // 8), Selector.linkage runs in rank order, and the ranks' names are the list's paths.  Returns
    Selector.linkage's dict on the host plus "names" (rank order), "order" (order[rank] = the genome's line in the list), "table" (the
    text of -J) and "newick" (the text of -N; None for a capped hierarchy without fill)"""
    code = measure_code(measure)
    if code not in (MEASURE_JACCARD, MEASURE_MAX_CONTAINMENT, MEASURE_SMH_JACCARD):
        raise ValueError("measure of a hierarchy: 'jaccard', 'max_containment' or 'smh_jaccard' (the symmetric similarities)")
    linkage_code(method)
    m_smh = _matrix_buckets(measure, aux_bytes)
    ds = load_dataset(list_file, m_smh, 0, fp_mode)
    n = len(ds.names)
    with Selector(device, fp_mode) as sel:
        sel.upload(ds.hll, ds.aux if m_smh else np.zeros((n, 1), dtype=np.uint64), ds.cards)
        res = sel.linkage(measure, method, max_height)
    names = list(ds.names)
    whole = res["n_merges"] == max(n - 1, 0) or fill is not None
    res.update(names=names, order=np.asarray(ds.order), table=linkage_table(names, res),
               newick=linkage_newick(res["merges"], res["sizes"], names, fill) if whole else None)
    return res


def cluster_table(names: Sequence[str], order: np.ndarray, res: dict) -> str:
    """the text of `selection -L`: one line per genome in FILE-LIST order, 'path<TAB>cluster<TAB>cluster_size<TAB>degree<TAB>
    representative_path'.  names in rank order, order[rank] = the genome's line in the list, res = Selector.cluster(...) on the host"""
    out = []
    for r in np.argsort(np.asarray(order), kind="stable"):
        c = int(res["clusters"][r])
        out.append(f"{names[r]}\t{c}\t{int(res['sizes'][c])}\t{int(res['degrees'][r])}\t{names[int(res['representatives'][c])]}\n")
    return "".join(out)


def min_matches(m: int, j: float) -> int:
    """the smallest integer c in [1, m] with c / m >= j in float64: the count threshold of criterion smh_c (Selector.set_min_matches)
    that keeps exactly the pairs whose SuperMinHash estimate c / m reaches j.  ValueError for j > 1 (no count reaches it), for a NaN
    and for m < 1"""
    m, j = int(m), float(j)
    if m < 1:
        raise ValueError("min_matches: m must be >= 1")
    if not j <= 1.0:
        raise ValueError("min_matches: no count c <= m has c / m >= j for j > 1 (or NaN)")
    c = min(m, max(1, int(np.ceil(j * m))))
    while c > 1 and (c - 1) / m >= j:             # (j * m is rounded: settle on the exact boundary of the float64 quotient)
        c -= 1
    while c / m < j:
        c += 1
    return c


def containment_matches(m, gamma, e_lo, e_hi):
    """the count of equal SuperMinHash buckets, in [0, m + 1], from which a pair of truncated cardinalities e_lo <= e_hi has a
    SuperMinHash containment estimate c (e_lo + e_hi) / ((m + c) e_lo) >= gamma (m + 1: no count reaches it): the per-pair threshold of
    Selector.set_min_containment, computed by the library's own function (selhip_smhc_threshold; no device is touched).  Scalars give
    an int, arrays broadcast against each other and give an int32 array"""
    fn = hip_lib().selhip_smhc_threshold
    args = np.broadcast_arrays(np.asarray(m, dtype=np.int64), np.asarray(gamma, dtype=np.float64), np.asarray(e_lo, dtype=np.uint64), np.asarray(e_hi, dtype=np.uint64))
    out = np.empty(args[0].shape, dtype=np.int32)
    flat = out.reshape(-1)
    for j, (mm, g, a, b) in enumerate(zip(*(x.reshape(-1).tolist() for x in args))):
        flat[j] = fn(mm, g, a, b)
    return int(out) if out.ndim == 0 else out


ESTIMATORS = {"hll": ESTIMATOR_HLL, "smh": ESTIMATOR_SMH}


def estimator_code(estimator) -> int:
    """the SELHIP_ESTIMATOR_* code of an estimator given by name or by code; ValueError for anything else"""
    code = ESTIMATORS.get(estimator) if isinstance(estimator, str) else estimator
    if isinstance(code, bool) or not isinstance(code, (int, np.integer)) or code not in ESTIMATORS.values():
        raise ValueError("estimator: 'hll' or 'smh'")
    return int(code)


def _pass_estimator(estimator, criterion: str) -> int:
    """the code of a pass's estimator for the file-list helpers; ValueError for what the SuperMinHash estimator refuses"""
    code = estimator_code(estimator)
    if code == ESTIMATOR_SMH and criterion != "smh_c":
        raise ValueError(f"estimator 'smh' records a value computed from the count of criterion smh_c and takes no criterion {criterion}")
    return code


def smh_value(measure, m, c, e1, e2):
    """the value a pass records under Selector.set_estimator("smh") for a pair with c of m equal SuperMinHash buckets and truncated
    cardinalities e1, e2, computed by the library's own function (selhip_smh_value; no device is touched): c / m under "jaccard",
    c (a + b) / ((m + c) a) with a = min(e1, e2), b = max(e1, e2) under "max_containment" (NaN when a = 0; not clamped).  Scalars give a
    float, arrays broadcast against each other and give a float64 array"""
    code = measure_code(measure)
    if code not in (MEASURE_JACCARD, MEASURE_MAX_CONTAINMENT):
        raise ValueError("measure of a pass: 'jaccard' or 'max_containment' (the other measures are matrix measures)")
    fn = hip_lib().selhip_smh_value
    args = np.broadcast_arrays(np.asarray(m, dtype=np.int64), np.asarray(c, dtype=np.int64), np.asarray(e1, dtype=np.uint64), np.asarray(e2, dtype=np.uint64))
    out = np.empty(args[0].shape, dtype=np.float64)
    flat = out.reshape(-1)
    for j, (mm, cc, a, b) in enumerate(zip(*(x.reshape(-1).tolist() for x in args))):
        flat[j] = fn(code, mm, cc, a, b)
    return float(out) if out.ndim == 0 else out


def _criterion_files(criterion: str, aux_bytes: int, min_matches: Optional[int] = None, min_containment: Optional[float] = None) -> Tuple[int, int, int]:
    """(m, p_aux, CRIT_*) of a criterion name and `-a aux_bytes`, for the file-list front ends: m buckets of the .smh<m> files to read
    (0 = none), precision of the auxiliary .hll_<p> files (0 = none).  min_matches and min_containment go with "smh_c" and with nothing
    else; it needs one of them"""
    if min_matches is not None and criterion != "smh_c":
        raise ValueError("min_matches is the count threshold of criterion smh_c")
    if min_containment is not None and criterion != "smh_c":
        raise ValueError("min_containment is the per-pair count threshold of criterion smh_c")
    if criterion == "smh_a":
        return aux_bytes // 8, 0, CRIT_SMH_A                                   # selection.cpp:231
    if criterion == "smh_c":
        if min_matches is None and min_containment is None:
            raise ValueError("criterion smh_c needs min_matches (the count threshold c_min)")
        if aux_bytes // 8 < 1:
            raise ValueError("criterion smh_c reads the .smh<m> files: aux_bytes (8 m) must be given")
        return aux_bytes // 8, 0, CRIT_SMH_C
    if criterion in ("hll_a", "hll_an"):
        return 0, (aux_bytes & -aux_bytes).bit_length() - 1, CRIT_HLL_A if criterion == "hll_a" else CRIT_HLL_AN   # __builtin_ctz(aux_bytes), selection.cpp:125
    if criterion == "none":
        return 0, 0, CRIT_NONE                                                 # only the .hll files are read; aux_bytes is ignored
    raise ValueError("Option -c invalid. The accepted criteria are hll_a, hll_an and smh_a.")


def _aux_files(fold_aux: bool, p_aux: int, criterion: str) -> int:
    """precision of the .hll_<p> files a front end opens: p_aux, or 0 (none) when the context folds them itself (fold_aux)"""
    if not fold_aux:
        return p_aux
    if not p_aux:
        raise ValueError(f"fold_aux folds the auxiliary HLL sketches of the criteria hll_a / hll_an; criterion '{criterion}' reads none")
    return 0


def _filelist_pass(then, list_file: str, tau: float, aux_bytes: int, mode: int = MODE_CB_SMH, device: int = 0,
                   fp_mode: int = FP_FMA, algo: int = ALGO_AUTO, criterion: str = "smh_a", top_k: int = 0,
                   min_matches: Optional[int] = None, measure="jaccard", min_containment: Optional[float] = None, estimator="hll",
                   top_k_rounds=0, fold_aux: bool = False):
    """the all-pairs pass of select_from_filelist (its arguments); returns then(dataset, selector, fetched records) with the pass's
    result list still on the device"""
    meas = _pass_measure(measure, mode, criterion)
    est = _pass_estimator(estimator, criterion)
    rounds = topk_rounds_code(top_k_rounds)
    if rounds and not (top_k and criterion == "smh_c" and est == ESTIMATOR_SMH):
        raise ValueError("top_k_rounds takes top_k > 0, criterion 'smh_c' and estimator 'smh'")
    m, p_aux, crit = _criterion_files(criterion, aux_bytes, min_matches, min_containment)
    ds = load_dataset(list_file, m, _aux_files(fold_aux, p_aux, criterion), fp_mode)
    n_rows, n_bands = banding(m, tau) if m else (1, 1)
    with Selector(device, fp_mode) as sel:
        aux = ds.aux if m else np.zeros((len(ds.names), 1), dtype=np.uint64)
        sel.upload(ds.hll, aux, ds.cards)
        if fold_aux:
            sel.fold_aux_hll(p_aux)
        elif p_aux:
            sel.upload_aux_hll(ds.aux_hll, p_aux)
        sel.set_criterion(crit)
        if crit == CRIT_SMH_C:
            if min_matches is not None:
                sel.set_min_matches(min_matches)
            sel.set_min_containment(min_containment)
        sel.set_measure(meas)
        sel.set_estimator(est)
        pairs = sel.run(tau, mode, n_rows, n_bands, algo=algo, top_k=top_k if top_k else None, rounds=rounds if rounds else None)
        return then(ds, sel, pairs)


def select_from_filelist(list_file: str, tau: float, aux_bytes: int, mode: int = MODE_CB_SMH, device: int = 0,
                         fp_mode: int = FP_FMA, algo: int = ALGO_AUTO, criterion: str = "smh_a", top_k: int = 0,
                         min_matches: Optional[int] = None, measure="jaccard", min_containment: Optional[float] = None, estimator="hll",
                         top_k_rounds=0, fold_aux: bool = False) -> str:
    """The whole of selection_cuda.cpp main() (criterion smh_a) -- and of selection.cpp's hll_a / hll_an
    branches (:122-227): returns the text the CPU reference prints for `-c criterion -a aux_bytes -h tau`.
    criterion "none": no criterion in front of the Jaccard test (CRIT_NONE; mode MODE_CB_SMH = the CB bound alone, MODE_SMH = every pair).
    criterion "smh_c" with min_matches = c: at least c of the m = aux_bytes / 8 SuperMinHash buckets equal (CRIT_SMH_C; `-c smh_c -C c`);
    with min_containment = gamma (`-G gamma`), with or without min_matches: at least containment_matches(m, gamma, e_small, e_large) of them,
    the count at which the SuperMinHash estimate of the smaller genome's containment is gamma (Selector.set_min_containment).
    top_k > 0: only every genome's top_k best partners, one line 'owner_path partner_path J' each, in ranked order (owner rank, then J
    descending, ties by partner rank): a selected pair can be printed twice (once per member), once or not at all.
    measure "max_containment": the pairs with I / min(e_i, e_k) >= tau, that value printed in J's place (Selector.set_measure;
    ValueError with mode=MODE_CB_SMH or an hll_* criterion).
    estimator "smh" (`-V smh`, criterion "smh_c" alone): the value tested and printed is the SuperMinHash estimate of the count,
    smh_value(measure, m, c, e_i, e_k) (Selector.set_estimator), and no HLL stage runs.
    top_k_rounds (`-R rows`, with top_k > 0, criterion "smh_c" and estimator "smh" alone): the pass runs in rounds of that many rows, or
    "auto" (Selector.set_topk_rounds): the same text.
    fold_aux (`-D`, criteria "hll_a" / "hll_an" alone): no .hll_<p> file is opened; the context folds the auxiliary sketches from the
    .hll registers on the device (Selector.fold_aux_hll): the same text."""
    return _filelist_pass(lambda ds, sel, pairs: format_lines(ds.names, pairs), list_file, tau, aux_bytes, mode, device, fp_mode, algo, criterion,
                          top_k, min_matches, measure, min_containment, estimator, top_k_rounds, fold_aux)


def cluster_from_filelist(list_file: str, tau: float, aux_bytes: int, mode: int = MODE_CB_SMH, device: int = 0,
                          fp_mode: int = FP_FMA, algo: int = ALGO_AUTO, criterion: str = "smh_a", top_k: int = 0,
                          min_matches: Optional[int] = None, measure="jaccard", min_containment: Optional[float] = None, estimator="hll",
                          top_k_rounds=0, fold_aux: bool = False, cluster_min: Optional[float] = None, rep="max_degree") -> str:
    """The pass of select_from_filelist (same arguments), clustered on the device instead of printed: the text `selection ... -L file
    [-T cluster_min] [-Y rep]` writes -- one line per genome in file-list order, 'path<TAB>cluster<TAB>cluster_size<TAB>degree<TAB>
    representative_path' (Selector.cluster: single-linkage clusters of the selected pairs with value >= cluster_min, None = all of them;
    rep "max_degree", "min_rank" or "max_rank")"""
    code = rep_code(rep)
    if cluster_min is not None and np.isnan(cluster_min):
        raise ValueError("cluster_min: a number (None takes every selected pair), not NaN")
    return _filelist_pass(lambda ds, sel, pairs: cluster_table(ds.names, ds.order, sel.cluster(cluster_min, code)), list_file, tau, aux_bytes, mode,
                          device, fp_mode, algo, criterion, top_k, min_matches, measure, min_containment, estimator, top_k_rounds, fold_aux)


def greedy_from_filelist(list_file: str, tau: float, aux_bytes: int, mode: int = MODE_CB_SMH, device: int = 0,
                         fp_mode: int = FP_FMA, algo: int = ALGO_AUTO, criterion: str = "smh_a", top_k: int = 0,
                         min_matches: Optional[int] = None, measure="jaccard", min_containment: Optional[float] = None, estimator="hll",
                         top_k_rounds=0, fold_aux: bool = False, cluster_min: Optional[float] = None, order="max_degree", priority=None) -> str:
    """The pass of select_from_filelist (same arguments), clustered greedily on the device instead of printed: the text `selection ...
    -L file -Z greedy [-T cluster_min] [-Y order] [-W scores]` writes -- one line per genome in file-list order, 'path<TAB>cluster<TAB>
    cluster_size<TAB>degree<TAB>representative_path<TAB>value_to_representative' (Selector.cluster_greedy).  priority: one unsigned
    32-bit score per genome in FILE-LIST order (what -W reads); it selects the order "priority" and goes with no other"""
    if priority is not None and order == "max_degree":
        order = "priority"
    code = order_code(order)
    if (code == REP_PRIORITY) != (priority is not None):
        raise ValueError("priority: the scores of order 'priority', and of no other order")
    if cluster_min is not None and np.isnan(cluster_min):
        raise ValueError("cluster_min: a number (None takes every selected pair), not NaN")

    def then(ds, sel, pairs):
        prio = None if priority is None else np.asarray(priority)[np.asarray(ds.order)]          # file-list order -> rank order
        return greedy_table(ds.names, ds.order, sel.cluster_greedy(cluster_min, code, prio))
    return _filelist_pass(then, list_file, tau, aux_bytes, mode, device, fp_mode, algo, criterion, top_k, min_matches, measure, min_containment,
                          estimator, top_k_rounds, fold_aux)


def forest_from_filelist(list_file: str, tau: float, aux_bytes: int, mode: int = MODE_CB_SMH, device: int = 0,
                         fp_mode: int = FP_FMA, algo: int = ALGO_AUTO, criterion: str = "smh_a", top_k: int = 0,
                         min_matches: Optional[int] = None, measure="jaccard", min_containment: Optional[float] = None, estimator="hll",
                         top_k_rounds=0, fold_aux: bool = False, cluster_min: Optional[float] = None) -> str:
    """The pass of select_from_filelist (same arguments), its maximum spanning forest instead of its pairs: the text `selection ...
    -H file [-T cluster_min]` writes -- one line per forest edge, best first, 'path_a<TAB>path_b<TAB>value' (Selector.spanning_forest
    over the selected pairs with value >= cluster_min, None = all of them)"""
    if cluster_min is not None and np.isnan(cluster_min):
        raise ValueError("cluster_min: a number (None takes every selected pair), not NaN")
    return _filelist_pass(lambda ds, sel, pairs: forest_table(ds.names, sel.spanning_forest(cluster_min)["edges"]), list_file, tau, aux_bytes, mode,
                          device, fp_mode, algo, criterion, top_k, min_matches, measure, min_containment, estimator, top_k_rounds, fold_aux)


def topk_rounds_code(rows) -> int:
    """what selhip_ctx_set_topk_rounds takes for Selector.set_topk_rounds' argument: rows per round >= 0, or "auto" / TOPK_ROUNDS_AUTO"""
    if rows == "auto":
        return TOPK_ROUNDS_AUTO
    if isinstance(rows, bool) or not isinstance(rows, (int, np.integer)) or (rows < 0 and rows != TOPK_ROUNDS_AUTO):
        raise ValueError("top-k rounds: rows per round (0 = off) or 'auto'")
    return int(rows)


MEASURES = {"jaccard": MEASURE_JACCARD, "union": MEASURE_UNION, "smh_matches": MEASURE_SMH_MATCHES, "smh_jaccard": MEASURE_SMH_JACCARD,
            "intersection": MEASURE_INTERSECTION, "containment": MEASURE_CONTAINMENT, "max_containment": MEASURE_MAX_CONTAINMENT}
SMH_MEASURES = (MEASURE_SMH_MATCHES, MEASURE_SMH_JACCARD)
PASS_MEASURES = ("jaccard", "max_containment")          # what Selector.set_measure and the `measure=` of the file-list helpers take


def measure_code(measure) -> int:
    """the SELHIP_MEASURE_* code of a measure given by name or by code; ValueError for anything else"""
    code = MEASURES.get(measure) if isinstance(measure, str) else measure
    if isinstance(code, bool) or not isinstance(code, (int, np.integer)) or code not in MEASURES.values():
        raise ValueError("measure: 'jaccard', 'union', 'intersection', 'containment', 'max_containment', 'smh_matches' or 'smh_jaccard'")
    return int(code)


def _pass_measure(measure, mode: int, criterion: str) -> int:
    """the code of a pass's measure for the file-list helpers; ValueError for a matrix-only measure and for what max containment
    refuses -- MODE_CB_SMH and the hll_* criteria are bounds on J -- before any file is read"""
    code = measure_code(measure)
    if code not in (MEASURE_JACCARD, MEASURE_MAX_CONTAINMENT):
        raise ValueError("measure of a pass: 'jaccard' or 'max_containment' (the other measures are matrix measures)")
    if code == MEASURE_MAX_CONTAINMENT:
        if mode == MODE_CB_SMH:
            raise ValueError("measure 'max_containment' takes no MODE_CB_SMH: the CB bound is a bound on J and cuts pairs of unequal size; pass mode=MODE_SMH")
        if criterion in ("hll_a", "hll_an"):
            raise ValueError(f"measure 'max_containment' takes no criterion {criterion}: its bound is derived for J; use smh_a, smh_c or none")
    return code


def _matrix_buckets(measure, aux_bytes: int) -> int:
    """m of the .smh<m> files a matrix of this measure reads: aux_bytes / 8 for the SuperMinHash measures, 0 (none) for the HLL ones"""
    if measure_code(measure) not in SMH_MEASURES:
        return 0
    m = int(aux_bytes) // 8                                                    # 8 bytes per bucket, as `-a` of the selection passes
    if m <= 0:
        raise ValueError("measure 'smh_matches' / 'smh_jaccard' reads the .smh<m> files: aux_bytes (8 m) must be given")
    return m


def _inverse(order: np.ndarray) -> np.ndarray:
    inv = np.empty(len(order), dtype=np.int32)
    inv[order] = np.arange(len(order), dtype=np.int32)
    return inv


def matrix_from_filelist(list_file: str, aux_bytes: int = 0, measure="jaccard", dtype=None, fp_mode: int = FP_FMA, device: int = 0):
    """(names, tensor): the n x n matrix of the genomes of list_file with rows and columns in FILE-LIST order.  The sketches are loaded
    and sorted as for a selection, and the ranks' lines in the list go to the library as both position arrays: the matrix is written in
    place, nothing is gathered afterwards.  The HLL measures read only the .hll files (aux_bytes is accepted for symmetry with the other
    front ends); "smh_matches" / "smh_jaccard" also read the .smh<m> files, m = aux_bytes // 8 (aux_bytes == 0: ValueError)"""
    m_smh = _matrix_buckets(measure, aux_bytes)
    ds = load_dataset(list_file, m_smh, 0, fp_mode)
    n = len(ds.names)
    with Selector(device, fp_mode) as sel:
        sel.upload(ds.hll, ds.aux if m_smh else np.zeros((n, 1), dtype=np.uint64), ds.cards)
        m = sel.matrix(measure, dtype, row_pos=ds.order, col_pos=ds.order)
    names = [ds.names[r] for r in _inverse(ds.order)]
    return names, m


def query_matrix_from_filelists(query_list: str, db_list: str, aux_bytes: int = 0, measure="jaccard", dtype=None, fp_mode: int = FP_FMA,
                                device: int = 0):
    """(query names, database names, tensor): the n_Q x n_D matrix of the two lists, rows and columns in the order of their files
    (aux_bytes as for matrix_from_filelist)"""
    m_smh = _matrix_buckets(measure, aux_bytes)
    qs = load_dataset(query_list, m_smh, 0, fp_mode)
    db = load_dataset(db_list, m_smh, 0, fp_mode)
    with Selector(device, fp_mode) as sel:
        sel.upload(db.hll, db.aux if m_smh else np.zeros((len(db.names), 1), dtype=np.uint64), db.cards)
        sel.upload_queries(qs.hll, qs.aux if m_smh else np.zeros((len(qs.names), 1), dtype=np.uint64), qs.cards)
        m = sel.query_matrix(measure, dtype, row_pos=qs.order, col_pos=db.order)
    return [qs.names[r] for r in _inverse(qs.order)], [db.names[r] for r in _inverse(db.order)], m


def read_pair_list(pair_file: str, names: Sequence[str]) -> np.ndarray:
    """the lines 'name1 name2[ anything]' of a text file as an int32 (P, 2) array of ranks in `names` (rank order), in the file's
    order and orientation (selhost_read_pair_list: unknown names, equal names and short lines raise with the line number)"""
    h = host_lib()
    enc = [n.encode() for n in names]
    arr = (C.c_char_p * len(enc))(*enc)
    cnt = C.c_int64()
    out = np.zeros((0, 2), dtype=np.int32)
    for _ in range(2):
        rc = h.selhost_read_pair_list(str(pair_file).encode(), arr if enc else None, len(enc), out.ctypes.data if len(out) else None, len(out), C.byref(cnt))
        if rc:
            raise RuntimeError(f"selhost error {rc}: {h.selhost_last_error().decode()}")
        if cnt.value <= len(out):
            break
        out = np.zeros((cnt.value, 2), dtype=np.int32)
    return out[:cnt.value]


def select_pairs_from_filelist(list_file: str, pair_file: str, tau: float, aux_bytes: int, mode: int = MODE_CB_SMH, device: int = 0,
                               fp_mode: int = FP_FMA, algo: int = ALGO_AUTO, criterion: str = "smh_a",
                               min_matches: Optional[int] = None, measure="jaccard", min_containment: Optional[float] = None, estimator="hll",
                               fold_aux: bool = False) -> str:
    """select_from_filelist restricted to the pairs listed in pair_file (lines 'path1 path2[ anything]' with paths of list_file, in
    either order): the text `selection -l list_file -p pair_file -c criterion -a aux_bytes -h tau` prints (measure as there: `-S`;
    fold_aux as there: `-D`)"""
    meas = _pass_measure(measure, mode, criterion)
    est = _pass_estimator(estimator, criterion)
    m, p_aux, crit = _criterion_files(criterion, aux_bytes, min_matches, min_containment)
    ds = load_dataset(list_file, m, _aux_files(fold_aux, p_aux, criterion), fp_mode)
    listed = read_pair_list(pair_file, ds.names)
    n_rows, n_bands = banding(m, tau) if m else (1, 1)
    with Selector(device, fp_mode) as sel:
        sel.upload(ds.hll, ds.aux if m else np.zeros((len(ds.names), 1), dtype=np.uint64), ds.cards)
        if fold_aux:
            sel.fold_aux_hll(p_aux)
        elif p_aux:
            sel.upload_aux_hll(ds.aux_hll, p_aux)
        sel.set_criterion(crit)
        if crit == CRIT_SMH_C:
            if min_matches is not None:
                sel.set_min_matches(min_matches)
            sel.set_min_containment(min_containment)
        sel.set_measure(meas)
        sel.set_estimator(est)
        pairs = sel.run_pairs(listed, tau, mode, n_rows, n_bands, algo=algo)
    return format_lines(ds.names, pairs)


def multi_select(devices: Sequence[int], hll: np.ndarray, aux: np.ndarray, cards: np.ndarray, tau: float,
                 mode: int = MODE_CB_SMH, n_rows: Optional[int] = None, n_bands: Optional[int] = None, algo: int = ALGO_AUTO,
                 fp_mode: int = FP_FMA, gather: int = 2, criterion: int = 0, aux_hll: Optional[np.ndarray] = None, p_aux: int = 0,
                 p_hll: int = 14):
    """selhip_multi_select: one process, one context per listed device, interleaved row blocks, RCCL (or host) gather.
    gather: 0 host merge, 1 RCCL required, 2 RCCL if available; criterion / aux_hll / p_aux as for Selector (hll_a, hll_an,
    the two-stage criterion of BASELINE configs[4]; CRIT_NONE takes no auxiliary sketches); p_hll: precision of the main sketches
    (hll is [n, 1 << p_hll]).  Returns (pairs sorted by (i,k), stats dict)."""
    lib = hip_lib()
    hll = np.ascontiguousarray(hll, dtype=np.uint8)
    aux = np.ascontiguousarray(aux, dtype=np.uint64)
    cards = np.ascontiguousarray(cards, dtype=np.float64)
    n, m = aux.shape
    assert hll.shape == (n, 1 << p_hll), (hll.shape, n, p_hll)
    if n_rows is None or n_bands is None:
        n_rows, n_bands = banding(m, tau)
    devs = (C.c_int * len(devices))(*devices)
    ah = np.ascontiguousarray(aux_hll, dtype=np.uint8) if aux_hll is not None and criterion not in (CRIT_SMH_A, CRIT_NONE) else None
    cap = 1 << 16
    while True:
        out = np.zeros(cap, dtype=PAIR_DTYPE)
        cnt = C.c_int64()
        st = (C.c_int64 * 4)()
        rc = lib.selhip_multi_select(devs, len(devices), hll.ctypes.data, aux.ctypes.data, cards.ctypes.data,
                                     ah.ctypes.data if ah is not None else None, p_aux, criterion, n, m, p_hll, mode, algo,
                                     fp_mode, np.float32(tau), n_rows, n_bands, gather, out.ctypes.data, cap, C.byref(cnt), st)
        if rc == -3:
            cap = int(cnt.value)
            continue
        check(rc)
        return out[:cnt.value], {"evaluated": st[0], "survivors": st[1], "selected": st[2], "candidates": st[3]}


def ooc_select(hll: np.ndarray, aux: np.ndarray, cards: np.ndarray, tau: float, block_genomes: int,
               mode: int = MODE_CB_SMH, n_rows: Optional[int] = None, n_bands: Optional[int] = None, algo: int = ALGO_AUTO,
               fp_mode: int = FP_FMA, n_streams: int = 2, device: int = 0, criterion: int = 0,
               aux_hll: Optional[np.ndarray] = None, p_aux: int = 0, p_hll: int = 14):
    """selhip_ooc_select: the sketches stay in host memory, at most n_streams * 2 * block_genomes of them are on the device
    at a time; same result as one in-core pass.  p_hll: precision of the main sketches (hll is [n, 1 << p_hll]).  Returns (pairs with
    global ranks sorted by (i,k), stats dict)."""
    lib = hip_lib()
    hll = np.ascontiguousarray(hll, dtype=np.uint8)
    aux = np.ascontiguousarray(aux, dtype=np.uint64)
    cards = np.ascontiguousarray(cards, dtype=np.float64)
    n, m = aux.shape
    assert hll.shape == (n, 1 << p_hll), (hll.shape, n, p_hll)
    if n_rows is None or n_bands is None:
        n_rows, n_bands = banding(m, tau)
    ah = np.ascontiguousarray(aux_hll, dtype=np.uint8) if aux_hll is not None and criterion not in (CRIT_SMH_A, CRIT_NONE) else None
    cap = 1 << 16
    while True:
        out = np.zeros(cap, dtype=PAIR_DTYPE)
        cnt = C.c_int64()
        st = (C.c_int64 * 4)()
        rc = lib.selhip_ooc_select(device, hll.ctypes.data, aux.ctypes.data, cards.ctypes.data,
                                   ah.ctypes.data if ah is not None else None, p_aux, criterion, n, m, p_hll, mode, algo, fp_mode,
                                   np.float32(tau), n_rows, n_bands, block_genomes, n_streams, out.ctypes.data, cap, C.byref(cnt), st)
        if rc == -3:
            cap = int(cnt.value)
            continue
        check(rc)
        return out[:cnt.value], {"evaluated": st[0], "survivors": st[1], "selected": st[2], "candidates": st[3]}


def query_from_filelists(query_list: str, db_list: str, tau: float, aux_bytes: int, mode: int = MODE_CB_SMH, fp_mode: int = FP_FMA,
                         device: int = 0, algo: int = ALGO_AUTO, criterion: str = "smh_a", top_k: int = 0,
                         min_matches: Optional[int] = None, measure="jaccard", min_containment: Optional[float] = None, estimator="hll",
                         fold_aux: bool = False) -> str:
    """Query-vs-database selection: both lists are loaded and sorted by cardinality (load_dataset); returns one line
    'query_path db_path J' per selected pair, in (query rank, database rank) order, J formatted as selection.cpp prints it.
    top_k > 0: only every query's top_k best pairs, in ranked order (query rank, then J descending, ties by database rank).
    criterion "smh_a" (m = aux_bytes / 8 buckets), "hll_a" / "hll_an" (auxiliary HLL p = ctz(aux_bytes), as select_from_filelist) or
    "none" (every pair of the CB windows -- MODE_SMH: every cross pair -- to the Jaccard test) or "smh_c" with min_matches = c (at least
    c of the m = aux_bytes / 8 buckets equal).  measure "max_containment": the value tested and printed is I / min(e_q, e_d)
    (Selector.set_measure; ValueError with mode=MODE_CB_SMH or an hll_* criterion).  fold_aux (`-D`): the auxiliary sketches of both
    sets are folded from their .hll registers on the device, no .hll_<p> file is opened (as select_from_filelist)."""
    meas = _pass_measure(measure, mode, criterion)
    est = _pass_estimator(estimator, criterion)
    m, p_aux, crit = _criterion_files(criterion, aux_bytes, min_matches, min_containment)
    p_files = _aux_files(fold_aux, p_aux, criterion)
    qs = load_dataset(query_list, m, p_files, fp_mode)
    db = load_dataset(db_list, m, p_files, fp_mode)
    n_rows, n_bands = banding(m, tau) if m else (1, 1)
    with Selector(device, fp_mode) as sel:
        # (hll_a / hll_an read no SuperMinHash buckets: a one-bucket placeholder, as select_from_filelist uploads)
        sel.upload(db.hll, db.aux if m else np.zeros((len(db.names), 1), dtype=np.uint64), db.cards)
        sel.upload_queries(qs.hll, qs.aux if m else np.zeros((len(qs.names), 1), dtype=np.uint64), qs.cards)
        if fold_aux:
            sel.fold_aux_hll(p_aux)
            sel.fold_queries_aux_hll(p_aux)
        elif p_aux:
            sel.upload_aux_hll(db.aux_hll, p_aux)
            sel.upload_queries_aux_hll(qs.aux_hll, p_aux)
        sel.set_criterion(crit)
        if crit == CRIT_SMH_C:
            if min_matches is not None:
                sel.set_min_matches(min_matches)
            sel.set_min_containment(min_containment)
        sel.set_measure(meas)
        sel.set_estimator(est)
        pairs = sel.run_queries(tau, mode, n_rows, n_bands, algo, top_k=top_k if top_k else None)
    h = host_lib()
    buf = C.create_string_buffer(16384)
    out = []
    for rec in pairs:
        w = h.selhost_format_line(qs.names[rec["i"]].encode(), db.names[rec["k"]].encode(), float(rec["jaccard"]), buf, len(buf))
        if w < 0:
            raise RuntimeError("line too long")
        out.append(buf.raw[:w].decode())
    return "".join(out)
