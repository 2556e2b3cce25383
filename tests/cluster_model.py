"""The model of the single-linkage clusters (selhip_components, selhip_ctx_cluster; include/selection_hip.h sections 2g and 3): plain
numpy and Python, nothing from the library.

An edge list is an integer array [P, 2] of vertices in 0 .. n - 1; self-loops and repeated rows are legal.  A record list is a structured
array with the fields i, k and jaccard (the layout of selhip_pair_t); its edges are the records with jaccard >= min_value.
"""
import numpy as np

REP_MAX_DEGREE, REP_MIN_RANK, REP_MAX_RANK = 0, 1, 2
REP_NAMES = {"max_degree": REP_MAX_DEGREE, "min_rank": REP_MIN_RANK, "max_rank": REP_MAX_RANK}


def labels(edges, n):
    """int32 [n]: the smallest vertex of every vertex's connected component -- a sequential union-find that hooks the larger root under
    the smaller one, so a root is the minimum of its tree"""
    parent = list(range(n))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for u, v in np.asarray(edges, dtype=np.int64).reshape(-1, 2).tolist():
        a, b = find(u), find(v)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(g) for g in range(n)], dtype=np.int32)


def bfs_labels(edges, n):
    """the same by a breadth-first search from every vertex not reached yet, in ascending order: the independent check of labels()"""
    adj = [[] for _ in range(n)]
    for u, v in np.asarray(edges, dtype=np.int64).reshape(-1, 2).tolist():
        adj[u].append(v)
        adj[v].append(u)
    lab = [-1] * n
    for s in range(n):
        if lab[s] >= 0:
            continue
        lab[s] = s
        frontier = [s]
        while frontier:
            nxt = []
            for x in frontier:
                for y in adj[x]:
                    if lab[y] < 0:
                        lab[y] = s
                        nxt.append(y)
            frontier = nxt
    return np.array(lab, dtype=np.int32)


def dense_ids(lab):
    """(int32 [n] cluster of every vertex, C): the components numbered 0 .. C - 1 by ascending label"""
    lab = np.asarray(lab, dtype=np.int64)
    roots = np.flatnonzero(lab == np.arange(len(lab)))
    ids = np.full(len(lab), -1, dtype=np.int64)
    ids[roots] = np.arange(len(roots))
    return ids[lab].astype(np.int32), len(roots)


def degrees(edges, n):
    """int32 [n]: the ROWS of the edge list a vertex appears in, once per column -- a repeated row counts again, a self-loop twice"""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    return (np.bincount(e[:, 0], minlength=n) + np.bincount(e[:, 1], minlength=n)).astype(np.int32)


def sizes(cluster, n_clusters):
    return np.bincount(np.asarray(cluster, dtype=np.int64), minlength=n_clusters).astype(np.int32)


def representatives(cluster, n_clusters, degree, rule):
    """int32 [C]: max_degree -- the member with the largest degree, ties to the smaller vertex; min_rank -- the smallest member;
    max_rank -- the largest"""
    rule = REP_NAMES.get(rule, rule)
    rep = [None] * n_clusters
    for g, c in enumerate(np.asarray(cluster).tolist()):
        cur = rep[c]
        if cur is None:
            rep[c] = g
        elif rule == REP_MAX_DEGREE:
            if degree[g] > degree[cur]:
                rep[c] = g
        elif rule == REP_MAX_RANK:
            rep[c] = g
        elif rule != REP_MIN_RANK:
            raise ValueError(rule)
    return np.array(rep, dtype=np.int32).reshape(n_clusters)


def record_edges(records, min_value=-np.inf):
    """the edges [P, 2] of a record list: the records whose value is >= min_value in float64 (NaN never is)"""
    rec = np.asarray(records)
    with np.errstate(invalid="ignore"):
        keep = rec["jaccard"].astype(np.float64) >= np.float64(min_value)
    return np.stack([rec["i"][keep], rec["k"][keep]], axis=1).astype(np.int64).reshape(-1, 2)


def clusters(edges, n, rule="max_degree"):
    """everything selhip_ctx_cluster returns, as a dict of int32 arrays and n_clusters"""
    lab = labels(edges, n)
    cl, c = dense_ids(lab)
    deg = degrees(edges, n)
    return {"labels": lab, "clusters": cl, "degrees": deg, "sizes": sizes(cl, c), "representatives": representatives(cl, c, deg, rule),
            "n_clusters": c}


def table(names, order, res):
    """the text of `selection -L`: one line per genome in file-list order (names in rank order, order[rank] = its line in the list)"""
    out = []
    for r in np.argsort(np.asarray(order), kind="stable").tolist():
        c = int(res["clusters"][r])
        out.append("%s\t%d\t%d\t%d\t%s\n" % (names[r], c, int(res["sizes"][c]), int(res["degrees"][r]), names[int(res["representatives"][c])]))
    return "".join(out)
