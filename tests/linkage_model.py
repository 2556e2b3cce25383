"""The sequential model of the dense-matrix hierarchy (include/selection_hip.h section 2k): plain numpy, no device, no SciPy.  Every
output of selhip_linkage / selhip_ctx_linkage is DEFINED by it, bit for bit.  Shared by test_linkage_host.py and test_linkage_gpu.py.

numpy evaluates `sa * x`, `+` and `/` on float64 arrays one operation at a time, each rounded on its own: the arithmetic the header
prescribes (no fused multiply-add)."""
import numpy as np

SINGLE, COMPLETE, AVERAGE, WEIGHTED = 0, 1, 2, 3
METHODS = {"single": SINGLE, "complete": COMPLETE, "average": AVERAGE, "weighted": WEIGHTED}
PAIR_DTYPE = np.dtype([("i", "<i4"), ("k", "<i4"), ("jaccard", "<f8")], align=True)


def lw(method, x, y, sa, sb):
    """Lance-Williams: d(i u j, k) from x = d(i, k), y = d(j, k) and the sizes (as doubles)"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    sa, sb = np.asarray(sa, dtype=np.float64), np.asarray(sb, dtype=np.float64)
    with np.errstate(all="ignore"):
        if method == SINGLE:
            return np.where(y < x, y, x)
        if method == COMPLETE:
            return np.where(y > x, y, x)
        if method == AVERAGE:
            px, py, s = sa * x, sb * y, sa + sb
            num = px + py
            return num / s
        hx, hy = np.float64(0.5) * x, np.float64(0.5) * y
        return hx + hy


class BadCells(ValueError):
    def __init__(self, count, a, b):
        super().__init__(f"{count} cells of the upper triangle are NaN or -inf; cell ({a}, {b}) is one")
        self.count, self.cell = count, (a, b)


def linkage_model(dist, method, max_height=np.inf):
    """dict: merges (PAIR_DTYPE, emitted order), sizes (int32), n_merges, rounds (rescan rounds and the empty last one included),
    rescans, rowscans, pairs_per_round"""
    method = METHODS.get(method, method)
    D = np.array(dist, dtype=np.float64, copy=True)
    n = D.shape[0]
    assert D.shape == (n, n) and method in (SINGLE, COMPLETE, AVERAGE, WEIGHTED) and not np.isnan(max_height)
    iu = np.triu_indices(n, 1)
    up = D[iu]
    bad = ~(up > -np.inf)                                          # NaN or -inf
    if bad.any():
        j = int(np.flatnonzero(bad)[0])                            # (row-major: the smallest a * n + b)
        raise BadCells(int(bad.sum()), int(iu[0][j]), int(iu[1][j]))
    D[(iu[1], iu[0])] = up                                         # the mirror; the diagonal is never read
    active = np.ones(n, dtype=bool)
    size = np.ones(n, dtype=np.int64)
    nn = np.full(n, -1, dtype=np.int64)
    nd = np.zeros(n, dtype=np.float64)
    dirty = np.ones(n, dtype=bool)
    merges, sizes, per_round = [], [], []
    rounds = rescans = rowscans = 0
    while n > 0:
        rounds += 1
        rows = np.flatnonzero(active & dirty)
        full = len(rows) == int(active.sum())
        for r in rows:                                             # 1. scan
            mask = active.copy()
            mask[r] = False
            cols = np.flatnonzero(mask)
            if len(cols) == 0:
                nn[r], nd[r] = -1, 0.0
                continue
            v = D[r, cols]
            j = int(np.argmin(v))                                  # the first of the equal minima: the smallest slot; -0.0 == +0.0
            nn[r], nd[r] = cols[j], v[j]
        rowscans += len(rows)
        dirty[:] = False
        pairs = [(int(a), int(nn[a])) for a in np.flatnonzero(active)                                       # 2. pair
                 if nn[a] > a and active[nn[a]] and nn[nn[a]] == a and nd[a] <= max_height]
        per_round.append(len(pairs))
        if not pairs:
            if full:
                break
            rescans += 1
            dirty[active] = True
            continue
        paired = np.zeros(n, dtype=bool)
        for a, b in pairs:
            paired[a] = paired[b] = True
        free = np.flatnonzero(active & ~paired)
        pa, pb = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
        writes = []                                                # 3. update: every read is of the matrix before the round
        for j, (a, b) in enumerate(pairs):
            sa, sb = size[a], size[b]
            if len(free):
                writes.append((a, free, lw(method, D[a, free], D[b, free], sa, sb)))
            if j + 1 < len(pairs):                                 # the pairs (c, d) behind it (ascending a: c > a), all at once
                cs, ds = pa[j + 1:], pb[j + 1:]
                sc, sd = size[cs], size[ds]
                writes.append((a, cs, lw(method, lw(method, D[a, cs], D[a, ds], sc, sd), lw(method, D[b, cs], D[b, ds], sc, sd), sa, sb)))
        for a, ks, v in writes:
            D[a, ks] = v
            D[ks, a] = v
        gone = set()
        for a, b in pairs:                                         # 4. record
            merges.append((a, b, nd[a]))
            sizes.append(size[a] + size[b])
            size[a] += size[b]
            active[b] = False
            dirty[a] = True
            gone.update((a, b))
        for s in np.flatnonzero(active):
            if int(nn[s]) in gone:
                dirty[s] = True
    out = np.zeros(len(merges), dtype=PAIR_DTYPE)
    for j, (a, b, h) in enumerate(merges):
        out[j] = (a, b, h)
    return {"merges": out, "sizes": np.array(sizes, dtype=np.int32), "n_merges": len(merges), "rounds": rounds, "rescans": rescans,
            "rowscans": rowscans, "pairs_per_round": per_round}


def members_of(merges, n):
    """the member set (a frozenset of leaves) every merge creates, in emitted order"""
    held = {g: frozenset([g]) for g in range(n)}
    out = []
    for e in merges:
        a, b = int(e["i"]), int(e["k"])
        held[a] = held[a] | held.pop(b)
        out.append(held[a])
    return out


def labels_of(merges, n):
    """labels [n] (the smallest member) of the partition the merges leave"""
    lab = np.arange(n, dtype=np.int32)
    for s in members_of(merges, n):
        lab[list(s)] = min(s)
    return lab
