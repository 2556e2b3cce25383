"""The neighbour-joining definition of include/selection_hip.h section 2l in numpy: sequential over the joins, vectorised inside one,
f64 and plain.  It follows the header's row-sum shape (1 024 lanes, wave butterflies, the wave sums from wave 0 upwards), so its
records are the device's bit for bit.  The working matrix is the upper triangle mirrored by COPY, so signed zeros survive as on the
device; neighbor_joining(dist, first=k) stops behind k records.  Also the additive dyadic trees the tests take their truth from, and
the value sets tests/test_nj_host.py and tests/test_nj_gpu.py share: the file's seeded matrices (value_sets), the forged pair that
the pick kernel's later trips decide (forged), tied values at those sizes (tie_sets), signed zeros (zero_sets) and cells whose
sums overflow (overflow_sets)."""
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


def mirrored(dist):
    """the working matrix: the strict upper triangle of dist COPIED into the lower one, cell by cell (a -0.0 stays -0.0, as section 2l's
    "is mirrored" says and nj_mirror_kernel does; a sum of two triangles would turn it into +0.0), the diagonal +0.0"""
    D = np.array(dist, dtype=np.float64)
    np.fill_diagonal(D, 0.0)
    lo = np.tril_indices(D.shape[0], -1)
    D[lo] = D.T[lo]
    return D


def neighbor_joining(dist, first=None):
    """the n - 1 records of the strict upper triangle of dist [n, n]; first=k: the first min(k, n - 1) of them, and no join behind them
    is computed (a prefix of a large matrix costs what its joins cost)"""
    n = dist.shape[0]
    joins = np.zeros(max(n - 1, 0) if first is None else min(max(n - 1, 0), max(int(first), 0)), dtype=NJ_DTYPE)
    if len(joins) == 0:
        return joins
    D = mirrored(dist)
    act = np.arange(n)
    lower = np.tri(n, dtype=bool)                                            # the diagonal and below: no pair
    with np.errstate(all="ignore"):
        R = row_sums(D)
        for s in range(len(joins)):
            r = len(act)
            rm2 = float(r - 2)
            q = D[np.ix_(act, act)]                                                     # (a copy; the three steps in place, each rounded on its own)
            q *= rm2
            q -= R[act][:, None]
            q -= R[act][None, :]
            q[np.isnan(q)] = np.inf
            q[lower[:r, :r]] = np.inf
            best = int(np.argmin(q))                                                    # row-major, the first: the smallest (a, b) among the equal
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


# ---- the value sets of tests/test_nj_host.py and tests/test_nj_gpu.py: n x n float64, of which the strict upper triangle counts -----------
TRIP_SIZES = (LANES + 7, 2 * LANES + 7)      # two and three trips of the 1 024-lane loops (the pick's walk over the rows' bests, the row sums)
ZERO_SIZES = (2, 3, 5, 65, 257)
OVERFLOW_SIZES = (5, 65, 130)
PREFIX = 16                                  # records of the model computed at TRIP_SIZES
TWIN = (100, 102)                            # the pair that ties with forged_pair(n) in tie_sets(n)["twins"]


def first_q(dist):
    """q of every pair a < b at the first join (+inf elsewhere), as the definition forms it"""
    n = dist.shape[0]
    D = mirrored(dist)
    R = row_sums(D)
    q = (float(n - 2) * D - R[:, None]) - R[None, :]
    q[np.tri(n, dtype=bool)] = np.inf
    return q


def value_sets(n):
    """{value set: matrix} of test_against_the_model, from one seeded generator in this order"""
    rng = np.random.default_rng(2000 + n)
    sets = {"distinct": (rng.permutation(n * n).reshape(n, n) + rng.random((n, n)) / 2) / float(max(n * n, 1))}
    if n <= 513:
        sets["negative"] = 10.0 * rng.random((n, n)) ** 4                     # far from a metric: negative branch lengths
        if n >= 3:
            sets["dyadic"] = dyadic_tree(n, n)[0]
    if n <= 257:                                                              # ties: the smallest (a, b)
        sets["levels"] = rng.choice([0.25, 0.5, 0.75], size=(n, n))
        sets["equal"] = np.full((n, n), 0.5)
    return sets


def forged_pair(n):
    return n - 4, n - 2


def forged(n):
    """the "distinct" matrix of n with +50 on the rows and columns of forged_pair(n) and 0.001 between the two: both row sums are far
    above every other, so the first join is that pair -- the row at list position n - 4, which for n = 1 024 j + 7 lies in the pick's
    last trip, with two columns behind it"""
    p, q = forged_pair(n)
    D = value_sets(n)["distinct"].copy()
    D[[p, q], :] += 50.0
    D[:, [p, q]] += 50.0
    D[p, q] = 0.001
    return D


def tie_sets(n):
    """"equal": every q ties in every join, the answer is (0, 1), (0, 2), ...; "levels": three values, ties by the thousand; "twins":
    "equal" with 0.25 in the cells TWIN and forged_pair(n) -- every operation is exact, the two cells share the smallest q of the first
    join, and for n = 1 024 j + 7 the pick kernel meets them in different waves: the row n - 4 in a later trip of a lane of wave 0, the
    row 100 in wave 1, so only the cross-wave step's comparison of a gives the smaller pair"""
    twins = np.full((n, n), 0.5)
    twins[TWIN] = twins[forged_pair(n)] = 0.25
    return {"equal": np.full((n, n), 0.5), "levels": np.random.default_rng(3000 + n).choice([0.25, 0.5, 0.75], size=(n, n)), "twins": twins}


def zero_sets(n):
    """-0.0 in every cell; in a random half of the cells of an all-zero matrix; in half the zero cells of a "levels" matrix with a fourth
    level 0.0"""
    rng = np.random.default_rng(4000 + n)
    half = np.where(rng.random((n, n)) < 0.5, -0.0, 0.0)
    levels = rng.choice([0.0, 0.25, 0.5, 0.75], size=(n, n))
    levels[(levels == 0.0) & (rng.random((n, n)) < 0.5)] = -0.0
    return {"all": np.full((n, n), -0.0), "half": half, "levels0": levels}


def overflow_sets(n):
    """finite cells whose sums are not: "huge" -- every cell (0.5 + u) * 0.9e308, every sum overflows and every length is NaN --; at
    n = 65 also "mixed" -- uniform cells, those in the rows or columns 0 .. 7 times 1e307: the sums of those rows overflow, the others
    do not, and the lengths are +-inf, NaN and finite"""
    rng = np.random.default_rng(5000 + n)
    sets = {"huge": (0.5 + rng.random((n, n))) * 0.9e308}
    if n == 65:
        mixed = rng.random((n, n))
        i, j = np.indices((n, n))
        mixed[(i < 8) | (j < 8)] *= 1e307
        sets["mixed"] = mixed
    return sets
