"""The model of the greedy representative clusters (selhip_greedy_representatives, selhip_ctx_cluster_greedy; include/selection_hip.h
sections 2h and 3): plain numpy and Python, nothing from the library.

An edge list is an integer array [P, 2] of vertices in 0 .. n - 1; self-loops and repeated rows are legal and change nothing.  A record
list is a structured array with the fields i, k and jaccard (the layout of selhip_pair_t); its edges are the records with
jaccard >= min_value and i != k, and the value of an edge is the greatest of its records'.  A key is an unsigned 64-bit integer per
vertex; a vertex goes before another when its key is greater, or the keys are equal and it is the smaller vertex.
"""
import numpy as np

REP_MAX_DEGREE, REP_MIN_RANK, REP_MAX_RANK, REP_PRIORITY = 0, 1, 2, 3
ORDER_NAMES = {"max_degree": REP_MAX_DEGREE, "min_rank": REP_MIN_RANK, "max_rank": REP_MAX_RANK, "priority": REP_PRIORITY}


def _edges(edges):
    return np.asarray(edges, dtype=np.int64).reshape(-1, 2)


def visiting_order(n, key=None):
    """the vertices as the greedy visits them: descending key, equal keys by ascending vertex; key None = the vertex itself"""
    key = [int(k) for k in (range(n) if key is None else key)]
    return sorted(range(n), key=lambda g: (-key[g], g))


def representatives(edges, n, key=None):
    """bool [n]: the sequential greedy by sorted key -- a vertex is a representative unless a neighbour visited before it is one"""
    adj = [set() for _ in range(n)]
    for u, v in _edges(edges).tolist():
        if u != v:
            adj[u].add(v)
            adj[v].add(u)
    rep = np.zeros(n, dtype=bool)
    for g in visiting_order(n, key):
        rep[g] = not any(rep[h] for h in adj[g])
    return rep


def representatives_by_lists(edges, n, key=None):
    """the same from adjacency LISTS, marking the neighbours of every new representative as taken: the independent check"""
    nbr = [[] for _ in range(n)]
    for u, v in _edges(edges).tolist():
        nbr[u].append(v)
        nbr[v].append(u)
    taken, rep = [False] * n, [False] * n
    for g in visiting_order(n, key):
        if not taken[g]:
            rep[g] = True
            for h in nbr[g]:
                if h != g:
                    taken[h] = True
    return np.array(rep, dtype=bool).reshape(n)


def rounds_synchronous(edges, n, key=None):
    """the rounds of the device's scheme when every read of a round sees the state the round began with (all reads stale): an edge
    whose earlier end is a representative makes its later end a member, one whose earlier end is undecided blocks its later end, and
    the undecided vertices nothing blocked become representatives.  Returns (rounds, bool [n] representatives): the first round after
    which no vertex was undecided -- the upper bound of the device's count; 0 for n == 0"""
    e = _edges(edges)
    e = e[e[:, 0] != e[:, 1]]
    pos = np.empty(n, dtype=np.int64)
    pos[visiting_order(n, key)] = np.arange(n)
    first = pos[e[:, 0]] < pos[e[:, 1]]
    h, l = np.where(first, e[:, 0], e[:, 1]), np.where(first, e[:, 1], e[:, 0])
    UNDECIDED, REP, MEMBER = 0, 1, 2
    state = np.zeros(n, dtype=np.int8)
    rounds = 0
    while n and (rounds == 0 or np.any(state == UNDECIDED)):
        rounds += 1
        live = state[l] == UNDECIDED
        member = l[live & (state[h] == REP)]
        blocked = np.zeros(n, dtype=bool)
        blocked[l[live & (state[h] == UNDECIDED)]] = True
        state[member] = MEMBER
        state[(state == UNDECIDED) & ~blocked] = REP
    return rounds, state == REP


def degrees(records_or_edges, n):
    """int32 [n]: the ROWS a vertex appears in, once per column -- a repeated row counts again, a self-loop twice (as cluster_model)"""
    e = _edges(records_or_edges)
    return (np.bincount(e[:, 0], minlength=n) + np.bincount(e[:, 1], minlength=n)).astype(np.int32)


def keep(records, min_value=-np.inf):
    """the records whose value is >= min_value in float64 (NaN never is), self-records included: what the degrees count"""
    rec = np.asarray(records)
    with np.errstate(invalid="ignore"):
        return rec[rec["jaccard"].astype(np.float64) >= np.float64(min_value)]


def order_keys(rule, n, degree=None, priority=None):
    """the 64-bit keys of an order rule, as Python integers: (degree, reversed rank), reversed rank, rank, (priority, reversed rank)"""
    rule = ORDER_NAMES.get(rule, rule)
    rev = [0xFFFFFFFF - g for g in range(n)]
    if rule == REP_MAX_DEGREE:
        return [(int(degree[g]) << 32) | rev[g] for g in range(n)]
    if rule == REP_MIN_RANK:
        return rev
    if rule == REP_MAX_RANK:
        return list(range(n))
    if rule == REP_PRIORITY:
        return [(int(priority[g]) << 32) | rev[g] for g in range(n)]
    raise ValueError(rule)


def clusters(records, n, min_value=-np.inf, rule="max_degree", priority=None):
    """everything selhip_ctx_cluster_greedy returns, as a dict of arrays, n_clusters, and the synchronous scheme's rounds as
    "rounds_bound" (1 for a list without records)"""
    rec = keep(records, min_value)
    deg = degrees(np.stack([rec["i"], rec["k"]], axis=1), n)
    edge = rec[rec["i"] != rec["k"]]
    pairs = np.stack([edge["i"], edge["k"]], axis=1).astype(np.int64).reshape(-1, 2)
    key = order_keys(rule, n, deg, priority)
    rep = representatives(pairs, n, key)
    rep_of = np.where(rep, np.arange(n), -1).astype(np.int64)
    value = np.where(rep, 1.0, np.nan)
    # a member's candidates: its edges to representatives; the greatest value (as f64: -0.0 == +0.0), then the smaller rank
    best = {}
    for i, k, v in zip(edge["i"].tolist(), edge["k"].tolist(), edge["jaccard"].astype(np.float64).tolist()):
        for g, r in ((i, k), (k, i)):
            if not rep[g] and rep[r]:
                cur = best.get(g)
                if cur is None or v > cur[0] or (v == cur[0] and r < cur[1]):
                    best[g] = (v + 0.0, r)                                         # (-0.0 + 0.0 = +0.0: a zero is written +0.0)
    for g, (v, r) in best.items():
        rep_of[g], value[g] = r, v
    assert np.all(rep_of >= 0)                                                     # maximality: every member has a representative
    reps = np.flatnonzero(rep)
    ids = np.full(n, -1, dtype=np.int64)
    ids[reps] = np.arange(len(reps))
    cl = ids[rep_of]
    return {"rep_of": rep_of.astype(np.int32), "values": value.astype(np.float64), "clusters": cl.astype(np.int32), "degrees": deg,
            "sizes": np.bincount(cl, minlength=len(reps)).astype(np.int32), "representatives": reps.astype(np.int32),
            "n_clusters": len(reps), "rounds_bound": rounds_synchronous(pairs, n, key)[0] if len(rec) else min(n, 1)}


def table(names, order, res):
    """the text of `selection -L file -Z greedy`: one line per genome in file-list order (names in rank order, order[rank] = its line
    in the list); the value with six decimals, as std::to_string prints a double"""
    out = []
    for r in np.argsort(np.asarray(order), kind="stable").tolist():
        c = int(res["clusters"][r])
        out.append("%s\t%d\t%d\t%d\t%s\t%f\n" % (names[r], c, int(res["sizes"][c]), int(res["degrees"][r]), names[int(res["rep_of"][r])],
                                                float(res["values"][r])))
    return "".join(out)
