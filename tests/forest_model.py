"""Plain-Python models of the maximum spanning forest of a record list (include/selection_hip.h section 2j).

image            the order-preserving 64-bit integer image of a float64 that is no NaN (-0.0 and +0.0 share one)
kruskal          THE DEFINITION: one edge per unordered pair with the greatest of its records' values; the edges visited best first
                 (greater image, then the smaller (a, b)); an edge is kept iff its ends are not yet connected
boruvka_rounds   the device's scheme run synchronously: per round two passes over the RECORDS (every component's greatest outgoing image,
                 then the smallest pair among the records of that image), the mutual-pick rule, hooks, flatten; the rounds counted with
                 the empty last one

Both return edges as (a, b, image) tuples in BEFORE order and the labels (smallest vertex of the component)."""
import math
import struct

import numpy as np

PAIR_DTYPE = np.dtype([("i", "<i4"), ("k", "<i4"), ("jaccard", "<f8")])


def image(v):
    v = float(v)
    if v == 0.0:
        v = 0.0                                                   # -0.0 -> +0.0
    b = struct.unpack("<Q", struct.pack("<d", v))[0]
    return (~b) & (2 ** 64 - 1) if b >> 63 else b | (1 << 63)


def value_of(im):
    """the float64 whose image is im"""
    b = im & (2 ** 63 - 1) if im >> 63 else (~im) & (2 ** 64 - 1)
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def graph(records, min_value=-math.inf):
    """records (u, v, value) -> {(a, b): greatest image}: one edge per unordered pair; NaN values, values below the cut and loops are none"""
    g = {}
    for u, v, x in records:
        if not (x >= min_value) or u == v:
            continue
        key = (u, v) if u < v else (v, u)
        im = image(x)
        if g.get(key, 0) < im:
            g[key] = im
    return g


def kruskal(records, n, min_value=-math.inf):
    order = sorted(graph(records, min_value).items(), key=lambda kv: (-kv[1], kv[0]))
    par = list(range(n))

    def find(x):
        while par[x] != x:
            par[x] = par[par[x]]
            x = par[x]
        return x

    out = []
    for (a, b), im in order:
        ra, rb = find(a), find(b)
        if ra != rb:
            par[max(ra, rb)] = min(ra, rb)
            out.append((a, b, im))
    return out, [find(x) for x in range(n)]


def boruvka_rounds(records, n, min_value=-math.inf):
    recs = [(min(u, v), max(u, v), image(x)) for u, v, x in records if x >= min_value and u != v]
    comp = list(range(n))
    out = []
    rounds = 0
    while True:
        rounds += 1
        live = [(a, b, im, comp[a], comp[b]) for a, b, im in recs if comp[a] != comp[b]]
        best = {}
        for a, b, im, ca, cb in live:                             # pass 1: the greatest image per component
            for c in (ca, cb):
                if best.get(c, 0) < im:
                    best[c] = im
        pick = {}
        for a, b, im, ca, cb in live:                             # pass 2: the smallest pair among the records of that image
            for c in (ca, cb):
                if best[c] == im and pick.get(c, (n, n)) > (a, b):
                    pick[c] = (a, b)
        if not pick:
            break
        par = list(range(n))

        def find(x):
            while par[x] != x:
                par[x] = par[par[x]]                              # (halving: a hook chain of n stays cheap)
                x = par[x]
            return x

        other ={c: (comp[b] if comp[a] == c else comp[a]) for c, (a, b) in pick.items()}
        for c, (a, b) in pick.items():
            if pick.get(other[c]) == (a, b) and other[c] < c:     # a mutual pick: the smaller root emits
                continue
            out.append((a, b, best[c]))
        for c in pick:
            rc, ro = find(c), find(other[c])
            assert rc != ro or pick.get(other[c]) == pick[c], "the picks of a round close a cycle"
            if rc != ro:
                par[max(rc, ro)] = min(rc, ro)
        comp = [find(c) for c in comp]
        recs = [(a, b, im) for a, b, im, _, _ in live]            # (a record inside one component never leaves it again)
    out.sort(key=lambda e: (-e[2], e[0], e[1]))
    return out, comp, rounds


def records_of(pairs, values=None):
    """(u, v, value) tuples of an edge array and its values (None: 1.0 each)"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    vals = np.ones(len(pairs)) if values is None else np.asarray(values, dtype=np.float64)
    return list(zip(pairs[:, 0].tolist(), pairs[:, 1].tolist(), vals.tolist()))


def records_of_pass(rec):
    return list(zip(rec["i"].tolist(), rec["k"].tolist(), rec["jaccard"].tolist()))


def as_records(edges):
    """(a, b, image) tuples -> the PAIR_DTYPE array the device writes"""
    out = np.zeros(len(edges), dtype=PAIR_DTYPE)
    for j, (a, b, im) in enumerate(edges):
        out[j] = (a, b, value_of(im))
    return out


def linkage(edges, n, distance=lambda v: 1.0 - v):
    """SciPy's linkage matrix of a spanning TREE given as (a, b, image) tuples in BEFORE order"""
    par, cid, size, z = list(range(n)), list(range(n)), [1] * n, []

    def find(x):
        while par[x] != x:
            x = par[x]
        return x

    for s, (a, b, im) in enumerate(edges):
        ra, rb = find(a), find(b)
        ia, ib = cid[ra], cid[rb]
        lo, hi = min(ra, rb), max(ra, rb)
        par[hi] = lo
        size[lo] += size[hi]
        cid[lo] = n + s
        z.append([min(ia, ib), max(ia, ib), distance(value_of(im)), size[lo]])
    return np.array(z, dtype=float).reshape(-1, 4)
