"""The all-pairs top-k in row rounds (selhip_ctx_set_topk_rounds), replayed in numpy on the records of the one-shot
pass: thresholds per round, the admitted set per round, the carried list C per round.  Nothing here comes from the library.

A record is a row of a structured array with the fields i, k (int32) and jaccard (float64) -- the layout of selhip_pair_t.  Records of
a pass have i < k; records of C are directed: i = owner, k = partner.
"""
import numpy as np

REC = np.dtype([("i", "<i4"), ("k", "<i4"), ("jaccard", "<f8")])


def key(values):
    """the u64 whose unsigned order is the IEEE total order of the doubles (kernel_topk.cuh)"""
    bits = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    return np.where(bits >> np.uint64(63) != 0, ~bits, bits ^ np.uint64(1 << 63))


def ranked_cut(directed, K):
    """every owner's first min(L, K) records by (key descending, partner ascending), owners ascending"""
    d = np.ascontiguousarray(directed, dtype=REC)
    d = d[np.lexsort((d["k"], ~key(d["jaccard"]), d["i"]))]
    if len(d) == 0:
        return d
    start = np.r_[0, np.flatnonzero(d["i"][1:] != d["i"][:-1]) + 1]
    pos = np.arange(len(d)) - np.repeat(start, np.diff(np.r_[start, len(d)]))
    return d[pos < K]


def both_members(records):
    """the two directed records of every record: {owner i, partner k}, {owner k, partner i}"""
    r = np.ascontiguousarray(records, dtype=REC)
    s = r.copy()
    s["i"], s["k"] = r["k"], r["i"]
    return np.concatenate([r, s])


def thresholds(C, n, K):
    """thr[g]: -inf while C holds fewer than K records of owner g, else the value of its K-th record (C in ranked order)"""
    thr = np.full(n, -np.inf)
    if len(C):
        owners, first, count = np.unique(C["i"], return_index=True, return_counts=True)
        full = count >= K
        thr[owners[full]] = C["jaccard"][first[full] + K - 1]
    return thr


def round_rows(row_begin, row_end, R):
    """the row ranges of the rounds"""
    return [(b, min(b + R, row_end)) for b in range(row_begin, row_end, R)]


def replay(records, n, K, R, rows=None):
    """(final list C in ranked order, records admitted over all rounds, [admitted per round], [C per round]) of the pass whose one-shot
    result is `records` (i < k, any order), over the rows [rows[0], rows[1]) (default all n) in rounds of R rows"""
    rec = np.ascontiguousarray(records, dtype=REC)
    rb, re = rows if rows is not None else (0, n)
    C = np.zeros(0, dtype=REC)
    per_round, lists = [], []
    for b, e in round_rows(rb, re, R):
        thr = thresholds(C, n, K)                                     # as they stand when the round begins
        mine = rec[(rec["i"] >= b) & (rec["i"] < e)]
        adm = mine[(mine["jaccard"] >= thr[mine["i"]]) | (mine["jaccard"] >= thr[mine["k"]])]
        C = ranked_cut(np.concatenate([C, both_members(adm)]), K)
        per_round.append(len(adm))
        lists.append(C)
    return C, int(sum(per_round)), per_round, lists
