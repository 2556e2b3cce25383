"""The Markov clustering of include/selection_hip.h section 2o, restated in numpy and plain Python: every column is worked out in a dense
float64 vector, with Python loops for every sum whose order the definition fixes; between the iterations a column is kept as its
(rows, values), so that a graph of a few thousand vertices stays light.  Python's float is the IEEE double, so `a * b` and `a + b`
round as the definition says."""
import numpy as np


def settle(x, K, margins):
    """a column's candidates x (dense, 0 = none) cut to the K best -- greater value first, equal values by the smaller row -- and
    normalised, the sum in ascending row order: (rows ascending, values)"""
    order = sorted(np.flatnonzero(x), key=lambda i: (-x[i], i))
    if len(order) > K:
        margins.append((x[order[K - 1]] - x[order[K]]) / x[order[K - 1]])
    keep = sorted(order[:K])
    s = 0.0
    for i in keep:
        s = s + float(x[i])
    return np.array(keep, dtype=np.int64), np.array([float(x[i]) / s for i in keep])


def chaos_of(vals):
    s = 0.0
    for v in vals:
        s = s + float(v) * float(v)
    return float(vals.max()) - s


def dense(columns, n):
    """the flow matrix of a list of (rows, values) columns"""
    M = np.zeros((n, n))
    for j, (rows, vals) in enumerate(columns):
        M[rows, j] = vals
    return M


def mcl(row_ptr, col, val, n, inflation=2.0, max_entries=32, prune=1e-4, max_iters=64, chaos_tol=1e-3):
    """{"label", "cluster", "n_clusters", "iters", "chaos", "columns" (the final matrix: (rows, values) per column), "margin" (the smallest
    relative distance of an iteration's prune or cut decision from its threshold)}"""
    K, margins, M = max_entries, [], []
    for j in range(n):
        x = np.zeros(n)
        for e in range(row_ptr[j], row_ptr[j + 1]):
            if col[e] != j and val[e] > 0:
                x[col[e]] = val[e]
        x[j] = x.max() if x.max() > 0 else 1.0
        M.append(settle(x, K, []))                                              # (no pow in the start: its decisions are exact, the self loop's tie included)
    iters, chaos = 0, 0.0
    while iters < max_iters:
        N, chaos = [], -np.inf
        for j in range(n):
            x, seen = np.zeros(n), np.zeros(n, dtype=bool)
            for k, w in zip(*M[j]):                                             # ascending k = ascending s
                for i, m in zip(*M[k]):
                    p = float(m) * float(w)
                    x[i] = x[i] + p if seen[i] else p
                    seen[i] = True
            x = x * x if inflation == 2.0 else np.power(x, inflation)
            cut = prune * float(x.max())
            margins.extend(abs(v - cut) / cut for v in x[x > 0])
            x[x < cut] = 0.0
            N.append(settle(x, K, margins))
            chaos = max(chaos, chaos_of(N[j][1]))
        M, iters = N, iters + 1
        if chaos <= chaos_tol:
            break
    label = np.arange(n)

    def find(v):
        while label[v] != v:
            v = label[v]
        return v
    for j, (rows, _) in enumerate(M):
        for i in rows:
            a, b = find(i), find(j)
            label[max(a, b)] = min(a, b)
    label = np.array([find(v) for v in range(n)], dtype=np.int32)
    cluster = np.searchsorted(np.unique(label), label).astype(np.int32)
    return {"label": label, "cluster": cluster, "n_clusters": len(np.unique(label)), "iters": iters, "chaos": chaos, "columns": M,
            "margin": min(margins, default=np.inf)}


def planted(seed=1, hub=True):
    """(row_ptr, col, val, n) of a symmetric graph: six clusters of 5 .. 40 vertices with weights in (0.5, 1), a few weak bridges, two
    isolated vertices at the end and, with hub, one vertex of the largest cluster with 45 weak edges into the others: a row above 64"""
    rng = np.random.default_rng(seed)
    sizes = [5, 12, 19, 26, 33, 40]
    n = sum(sizes) + 2
    A = np.zeros((n, n))
    starts = np.concatenate([[0], np.cumsum(sizes)])
    for a, b in zip(starts[:-1], starts[1:]):
        A[a:b, a:b] = np.triu(rng.uniform(0.5, 1.0, (b - a, b - a)) * (rng.random((b - a, b - a)) < 0.8), 1)
    for c in range(5):                                                          # a weak bridge from each cluster into the next
        A[starts[c], starts[c + 1] + 1] = rng.uniform(0.02, 0.08)
    if hub:
        A[rng.permutation(starts[5])[:45], starts[5] + 3] = rng.uniform(0.02, 0.08, 45)
    A = A + A.T
    row_ptr = np.concatenate([[0], np.cumsum((A > 0).sum(axis=1))]).astype(np.int64)
    rows, cols = np.nonzero(A)
    return row_ptr, cols.astype(np.int32), A[rows, cols], n
