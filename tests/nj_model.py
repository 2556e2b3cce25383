"""The neighbour-joining definition of include/selection_hip.h section 2l in numpy: sequential over the joins, vectorised inside one,
f64 and plain.  It follows the header's row-sum shape (1 024 lanes, wave butterflies, the wave sums from wave 0 upwards), so its
records are the device's bit for bit.  Also the additive dyadic trees the tests take their truth from."""
import numpy as np

NJ_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("len_a", "<f8"), ("len_b", "<f8")], align=True)
LANES, WAVE = 1024, 64


def row_sums(cells):
    """the sums of the rows of cells [m, n] in the contract's shape; a cell that adds nothing is given as +0.0"""
    m, n = cells.shape
    x = np.zeros((m, -(-max(n, 1) // LANES) * LANES))
    x[:, :n] = cells
    acc = np.zeros((m, LANES))
    for j in range(x.shape[1] // LANES):
        acc = acc + x[:, j * LANES:(j + 1) * LANES]
    w = acc.reshape(m, LANES // WAVE, WAVE)
    lane = np.arange(WAVE)
    for s in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, lane ^ s]
    total = w[:, 0, 0]
    for i in range(1, LANES // WAVE):
        total = total + w[:, i, 0]
    return total


def neighbor_joining(dist):
    """the n - 1 records of the strict upper triangle of dist [n, n]"""
    n = dist.shape[0]
    joins = np.zeros(max(n - 1, 0), dtype=NJ_DTYPE)
    if n < 2:
        return joins
    D = np.triu(np.asarray(dist, dtype=np.float64), 1)
    D = D + D.T
    R = row_sums(D)
    act = np.arange(n)
    lower = np.tri(n, dtype=bool)                                            # the diagonal and below: no pair
    with np.errstate(all="ignore"):
        for s in range(n - 1):
            r = len(act)
            rm2 = float(r - 2)
            q = (rm2 * D[np.ix_(act, act)] - R[act][:, None]) - R[act][None, :]
            q[np.isnan(q)] = np.inf
            best = int(np.argmin(np.where(lower[:r, :r], np.inf, q)))                   # row-major, the first: the smallest (a, b) among the equal
            if best // r >= best % r:                                                   # every q is +inf
                best = 1
            a, b = int(act[best // r]), int(act[best % r])
            d = D[a, b]
            if r == 2:
                joins[s] = (a, b, 0.5 * d, 0.5 * d)
                break
            len_a = 0.5 * d + (R[a] - R[b]) / (2.0 * rm2)
            joins[s] = (a, b, len_a, d - len_a)
            k = act[(act != a) & (act != b)]
            v = 0.5 * ((D[a, k] + D[b, k]) - d)
            R[k] = ((R[k] - D[a, k]) - D[b, k]) + v
            D[a, k] = v
            D[k, a] = v
            act = act[act != b]
            new_row = np.zeros((1, n))
            new_row[0, k] = v
            R[a] = row_sums(new_row)[0]
    return joins


def dyadic_tree(n, seed):
    """a random unrooted binary tree over the leaves 0 .. n - 1 (n >= 3) whose edge lengths are multiples of 2^-6 in (0, 4):
    (dist [n, n] the leaves' path lengths -- every operation of the definition is exact on it --, the total edge length, the set of
    its non-trivial splits, each as the frozenset of leaves on the side without leaf 0)"""
    rng = np.random.default_rng(seed)
    length = lambda: float(rng.integers(1, 256)) / 64.0
    edges = {(0, n): length(), (1, n): length(), (2, n): length()}           # a star on three leaves around node n
    nxt = n + 1
    for leaf in range(3, n):                                                  # each further leaf hangs from the middle of a random edge
        keys = sorted(edges)
        u, w = keys[int(rng.integers(len(keys)))]
        del edges[(u, w)]
        edges.update({(u, nxt): length(), (w, nxt): length(), (leaf, nxt): length()})
        nxt += 1
    nodes = nxt
    adj = [[] for _ in range(nodes)]
    for (u, w), x in edges.items():
        adj[u].append((w, x))
        adj[w].append((u, x))
    dist = np.zeros((n, n))
    splits = set()
    for src in range(n):
        depth = np.full(nodes, -1.0)
        depth[src] = 0.0
        order, parent = [src], {src: -1}
        for u in order:
            for w, x in adj[u]:
                if w not in parent:
                    parent[w] = u
                    depth[w] = depth[u] + x
                    order.append(w)
        dist[src] = depth[:n]
        if src == 0:                                                          # the leaves below every internal edge, seen from leaf 0
            below = {u: {u} if u < n else set() for u in order}
            for u in reversed(order[1:]):
                below[parent[u]] |= below[u]
                if 1 < len(below[u]) < n - 1:
                    splits.add(frozenset(below[u]))
    return dist, sum(edges.values()), splits


def join_splits(joins, n):
    """the non-trivial splits of the tree the records describe, in dyadic_tree's form"""
    members = {g: {g} for g in range(n)}
    splits = set()
    for e in joins:
        a, b = int(e["a"]), int(e["b"])
        members[a] = members[a] | members.pop(b)
        side = members[a] if 0 not in members[a] else set(range(n)) - members[a]
        if 1 < len(side) < n - 1:
            splits.add(frozenset(side))
    return splits
