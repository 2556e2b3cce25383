"""A plain model of stage 1's band signatures, and sketch sets with FORGED signature collisions (no GPU, numpy / Python integers).

The signature of a band of r buckets v_0 .. v_{r-1} (csrc/kernel_sigjoin.cuh) is

    x_j = mix64(v_j + 0x9E3779B97F4A7C15 * (j + 1))        (64-bit wrapping)
    sig = (sum_j low32(x_j) mod 2^32)  xor  (sum_j high32(x_j) mod 2^32)

mix64 (two xor-shifts, two odd multiplications, a last xor-shift) is a bijection of the 64-bit words, so for any r - 1 buckets and any
32-bit target the last bucket can be solved for: choose the two half sums with the wanted xor, subtract the prefix's partial sums,
invert mix64, subtract the salt (forge_last).  planted_set hands the kernels bands whose signatures are equal while their contents are
not -- the case every verification behind a signature join exists for, and which random 64-bit buckets produce about once in 2^32.
"""
from dataclasses import dataclass, field

import numpy as np

MASK64 = (1 << 64) - 1
MASK32 = (1 << 32) - 1
GOLD = 0x9E3779B97F4A7C15
MUL1 = 0xBF58476D1CE4E5B9
MUL2 = 0x94D049BB133111EB
MUL1_INV = pow(MUL1, -1, 1 << 64)
MUL2_INV = pow(MUL2, -1, 1 << 64)


# ---- the hash --------------------------------------------------------------------------------------------------------------------
def _mix64_array(x):
    x = x.astype(np.uint64, copy=True)
    x ^= x >> np.uint64(30); x *= np.uint64(MUL1)
    x ^= x >> np.uint64(27); x *= np.uint64(MUL2)
    x ^= x >> np.uint64(31)
    return x


def mix64(x):
    """a Python integer -> a Python integer; a numpy array -> a uint64 array"""
    if isinstance(x, np.ndarray):
        return _mix64_array(x)
    x = int(x) & MASK64
    x ^= x >> 30; x = (x * MUL1) & MASK64
    x ^= x >> 27; x = (x * MUL2) & MASK64
    x ^= x >> 31
    return x


def _unxorshift(y, s):
    """x with x ^ (x >> s) == y"""
    x, t = y, y >> s
    while t:
        x ^= t
        t >>= s
    return x


def unmix64(y):
    """the inverse of mix64 (Python integers; arrays element by element)"""
    if isinstance(y, np.ndarray):
        return np.array([unmix64(int(v)) for v in y.ravel()], dtype=np.uint64).reshape(y.shape)
    y = int(y) & MASK64
    y = _unxorshift(y, 31); y = (y * MUL2_INV) & MASK64
    y = _unxorshift(y, 27); y = (y * MUL1_INV) & MASK64
    return _unxorshift(y, 30)


def band_sigs(aux, r, nb):
    """uint32[n, nb]: the 32-bit signature of every band of every genome (aux uint64[n, r * nb])"""
    aux = np.ascontiguousarray(aux, dtype=np.uint64)
    n = aux.shape[0]
    assert aux.shape == (n, r * nb)
    salt = np.arange(1, r + 1, dtype=np.uint64) * np.uint64(GOLD)              # wraps
    x = _mix64_array(aux.reshape(n, nb, r) + salt)
    lo = (x & np.uint64(MASK32)).sum(axis=2, dtype=np.uint64) & np.uint64(MASK32)
    hi = (x >> np.uint64(32)).sum(axis=2, dtype=np.uint64) & np.uint64(MASK32)
    return (lo ^ hi).astype(np.uint32)


def _half_sums(values):
    lo = hi = 0
    for j, v in enumerate(values):
        x = mix64((int(v) + GOLD * (j + 1)) & MASK64)
        lo += x & MASK32
        hi += x >> 32
    return lo & MASK32, hi & MASK32


def band_sig(values):
    """signature of ONE band (its r buckets), Python integers"""
    lo, hi = _half_sums(values)
    return lo ^ hi


def forge_last(prefix, target, rng):
    """uint64[r]: `prefix` (r - 1 buckets, possibly none) and a last bucket that gives the band the 32-bit signature `target`.  The low
    half sum is drawn from rng, so two calls with the same arguments give different last buckets"""
    prefix = [int(v) for v in prefix]
    r = len(prefix) + 1
    lo_p, hi_p = _half_sums(prefix)
    lo_t = int(rng.integers(0, 1 << 32))
    hi_t = lo_t ^ (int(target) & MASK32)
    x = (((hi_t - hi_p) & MASK32) << 32) | ((lo_t - lo_p) & MASK32)
    last = (unmix64(x) - GOLD * r) & MASK64
    return np.array(prefix + [last], dtype=np.uint64)


# ---- the literal predicate -------------------------------------------------------------------------------------------------------
def literal_smh_a(aux_i, aux_k, r, nb):
    """some band of r buckets entirely equal"""
    a = np.asarray(aux_i, dtype=np.uint64).reshape(nb, r)
    b = np.asarray(aux_k, dtype=np.uint64).reshape(nb, r)
    return bool((a == b).all(axis=1).any())


def literal_matrix(aux_x, aux_y, r, nb):
    """bool[n_x, n_y]: literal_smh_a of every (x, y)"""
    ax = np.ascontiguousarray(aux_x, dtype=np.uint64).reshape(-1, nb, r)
    ay = np.ascontiguousarray(aux_y, dtype=np.uint64).reshape(-1, nb, r)
    out = np.zeros((ax.shape[0], ay.shape[0]), dtype=bool)
    for i in range(ax.shape[0]):
        out[i] = (ax[i][None] == ay).all(axis=2).any(axis=1)
    return out


def sig_match_matrix(sig_x, sig_y):
    """bool[n_x, n_y]: at least one band signature equal"""
    out = np.zeros((sig_x.shape[0], sig_y.shape[0]), dtype=bool)
    for i in range(sig_x.shape[0]):
        out[i] = (sig_x[i][None] == sig_y).any(axis=1)
    return out


# ---- the windows of a pass -------------------------------------------------------------------------------------------------------
def trunc_cards(cards):
    return np.asarray(cards, dtype=np.float64).astype(np.int64).astype(np.uint64)


def _cb(e_lo, e_hi, tau):
    with np.errstate(divide="ignore", invalid="ignore"):
        return (e_lo.astype(np.float64) / e_hi.astype(np.float64)) >= np.float64(np.float32(tau))


def allpairs_windows(cards, tau, use_cb):
    """(lo, hi): row i of an all-pairs pass over genomes in ascending cardinality meets k in [lo[i], hi[i]] = [max(i + 1, z0), hi_i]; z0 =
    the first genome with a non-zero truncated cardinality, hi_i = the last k with (double)e_i / (double)e_k >= tau (n - 1 without CB)"""
    e = trunc_cards(cards)
    n = e.shape[0]
    nz = np.nonzero(e != 0)[0]
    z0 = int(nz[0]) if nz.size else n
    lo = np.maximum(np.arange(n) + 1, z0)
    hi = np.full(n, n - 1, dtype=np.int64)
    if use_cb:
        for i in range(n):
            ok = np.nonzero(_cb(e[i], e[lo[i]:], tau))[0] if lo[i] < n else np.zeros(0, dtype=np.int64)
            hi[i] = lo[i] + int(ok[-1]) if ok.size else lo[i] - 1
            assert ok.size == 0 or ok.size == ok[-1] + 1                       # e_k ascends: the predicate holds on a prefix
    return lo, hi


def query_windows(cards_q, cards_d, tau, use_cb):
    """(lo, hi): query q meets the database genomes d in [lo[q], hi[q]] -- those with e_hi != 0 and, under CB, e_lo / e_hi >= tau"""
    e_q, e_d = trunc_cards(cards_q), trunc_cards(cards_d)
    lo = np.zeros(e_q.shape[0], dtype=np.int64)
    hi = np.full(e_q.shape[0], -1, dtype=np.int64)
    for q in range(e_q.shape[0]):
        e_lo, e_hi = np.minimum(e_q[q], e_d), np.maximum(e_q[q], e_d)
        ok = e_hi != 0
        if use_cb:
            ok &= _cb(e_lo, e_hi, tau)
        idx = np.nonzero(ok)[0]
        if idx.size:
            lo[q], hi[q] = idx[0], idx[-1]
            assert idx.size == idx[-1] - idx[0] + 1                            # contiguous
    return lo, hi


def window_mask(lo, hi, n_cols, rows=None):
    """bool[len(lo), n_cols]: column k inside row i's window; rows = (begin, end) keeps those rows only"""
    k = np.arange(n_cols)[None, :]
    mask = (k >= np.asarray(lo)[:, None]) & (k <= np.asarray(hi)[:, None])
    if rows is not None:
        i = np.arange(len(lo))[:, None]
        mask &= (i >= rows[0]) & (i < rows[1])
    return mask


def expected_candidates(sigs, lo, hi, rows=None):
    """all-pairs pass: the pairs (i, k), k inside row i's window, with at least one band signature equal -- each pair once, however
    many of its bands match"""
    return int((sig_match_matrix(sigs, sigs) & window_mask(lo, hi, sigs.shape[0], rows)).sum())


def expected_candidates_qd(sig_q, sig_d, lo, hi):
    """query pass: the same count over the (q, d) windows"""
    return int((sig_match_matrix(sig_q, sig_d) & window_mask(lo, hi, sig_d.shape[0])).sum())


def index_dir_bits(n_d):
    """bits of the bucket directory the sorted signature index of n_d database genomes gets (2 .. 4 entries per bucket on average)"""
    bits = 0
    while (4 << bits) < n_d:
        bits += 1
    return bits


# ---- the planted set -------------------------------------------------------------------------------------------------------------
CANDIDATE_CLASSES = ("C1", "C2", "C3", "C6", "C7", "C8", "C8=")       # at least one band signature equal: one candidate each
SURVIVOR_CLASSES = ("C2", "C3", "C8=")                                  # some band entirely equal
EDGE_SIGS = (0x00000000, 0xFFFFFFFF, 0x0000FFFF, 0xFFFF0000)
CROWD = 70
# (m, rows, bands) of the collision tests: one-bucket bands; 2 .. 32 rows (the tiled build, the one-launch pass); 128 bands (two
# 16-byte signature groups per lane of the verifications); bands longer than the 16 lanes that compare them; the serial r > 64 build
SHAPES = ((64, 1, 64), (64, 2, 32), (128, 8, 16), (128, 16, 8), (512, 4, 128), (512, 32, 16), (512, 64, 8), (1024, 128, 8))


@dataclass
class Planted:
    aux: np.ndarray                     # uint64[n, m], row = rank
    r: int
    nb: int
    pairs: dict = field(default_factory=dict)      # (i, k), i < k  ->  class name
    detail: dict = field(default_factory=dict)     # (i, k) -> (band, differing position or None) of the C1 pairs
    triples: list = field(default_factory=list)    # C7: (signature, band, (g0, g1, g2))
    crowd: tuple = ()                              # C8: the ranks that share band 0's signature
    crowd_equal: tuple = ()                        # ... and the one pair among them with equal contents

    def of(self, *classes):
        return sorted(p for p, c in self.pairs.items() if c in classes)


def c1_positions(r):
    """the differing positions of the C1 pairs: None = the last bucket alone, j = bucket j and the compensating last bucket.  Up to
    r = 32 every j in 0 .. r - 2.  A pair of genomes shows one position only (its first flagged band is the one compared bucket by
    bucket), so beyond that the set would not hold the pairs: there the positions are every lane of the 16-lane compares (16 t + s with
    t = s mod r / 16, so every `+= 16` step too), the first and the last lane of every step, and r - 2"""
    if r <= 32:
        return [None] + list(range(r - 1))
    steps = r // 16
    pos = {16 * (s % steps) + s for s in range(16)} | {16 * t for t in range(steps)} | {16 * t + 15 for t in range(steps)} | {r - 2}
    pos.discard(r - 1)
    return [None] + sorted(pos)


def planted_bands(nb):
    """where the planted bands sit: the first and the last band; for 128 bands also the edges of the verifications' 16-byte signature
    groups (3 | 4) and of their two halves of 16 groups (63 | 64)"""
    return [0, nb - 1] + ([3, 4, 63, 64] if nb == 128 else [])


def planted_set(n, m, r, nb, seed, dir_bits=6, q_stride=3, good=None, stale_cut=130):
    """Random 64-bit buckets with the collision classes planted on disjoint genomes (rows are ranks):
      C1  one band with an equal signature and unequal contents, one pair per position of c1_positions(r)      candidate, no survivor
      C2  band b0 collides, band b1 > b0 is entirely equal                                                       survivor, once
      C3  band b0 is entirely equal, band b1 > b0 collides                                                       survivor, once
      C4  one band whose signatures agree in the top 16 bits only                                                neither
      C5  one band whose signatures agree in the low 16 bits only                                                neither
      C6  every band collides, none is equal                                                                     ONE candidate, no survivor
      C7  triples sharing a band signature 0, 0xFFFFFFFF, 0x0000FFFF, 0xFFFF0000, and -- for a sorted index with 2^dir_bits directory
          buckets -- v << (32 - dir_bits) and that minus 1 for v = 5 and the last v; contents unequal           3 candidates a triple
      C8  70 genomes sharing band 0's signature, contents pairwise different but for ONE equal pair              2 415 candidates, 1 survivor
    Placement: a C1 pair sits on ranks (0, n - 1), a C6 pair on (15, 16), a C1 pair on (63, 64); ranks that are multiples of q_stride
    are the query side of the query tests: every class has a pair across the two sides and (but C8) one inside the database side, the
    crowd has three members on the query side, its equal pair lies across.  The zero-signature triple has two members below rank
    stale_cut and one at or above it.  good (bool[n, n], optional): the C2 / C3 pairs are put on rank pairs (i < k) marked there."""
    assert m == r * nb and n >= 190 and dir_bits >= 3
    rng = np.random.default_rng(seed)
    aux = rng.integers(0, 1 << 64, size=(n, m), dtype=np.uint64)
    P = Planted(aux, r, nb)
    free = set(range(n))
    is_q = lambda g: g % q_stride == 0                                        # noqa: E731

    def take(pred=lambda g: True):
        pool = sorted(g for g in free if pred(g))
        g = int(pool[int(rng.integers(len(pool)))])
        free.discard(g)
        return g

    def take_pair(kind):
        if kind == "cross":
            a, b = take(is_q), take(lambda g: not is_q(g))
        else:
            a, b = take(lambda g: not is_q(g)), take(lambda g: not is_q(g))
        return (a, b) if a < b else (b, a)

    def take_good(kind):
        if good is None:
            return take_pair(kind)
        side = (lambda i, k: is_q(i) != is_q(k)) if kind == "cross" else (lambda i, k: not is_q(i) and not is_q(k))
        pool = [(i, k) for i in sorted(free) for k in sorted(free) if i < k and good[i, k] and side(i, k)]
        i, k = pool[int(rng.integers(len(pool)))]
        free.discard(i); free.discard(k)
        return int(i), int(k)

    def band(g, b):
        return aux[g, b * r:(b + 1) * r]

    def collide(a, g, b, pos):
        """g's band b: a's, different in bucket `pos` (if any) and in the last bucket, with a's signature"""
        src = band(a, b).copy()
        if pos is not None:
            src[pos] ^= np.uint64(int(rng.integers(1, 1 << 63)))
        while True:
            new = forge_last(src[:-1], band_sig(band(a, b)), rng)
            if new[-1] != band(a, b)[-1]:
                break
        band(g, b)[:] = new

    def set_sig(g, b, target):
        band(g, b)[:] = forge_last(band(g, b)[:-1], target, rng)

    bands = planted_bands(nb)
    kinds = lambda cnt: ["cross", "db"] + ["cross" if t % 2 == 0 else "db" for t in range(cnt - 2)]      # noqa: E731

    # pinned placements first
    pinned = {"C1": [(0, n - 1), (63, 64)], "C6": [(15, 16)]}
    for prs in pinned.values():
        for i, k in prs:
            free.discard(i); free.discard(k)

    # C8: the crowd
    crowd_q = [take(is_q) for _ in range(3)]
    crowd_d = [take(lambda g: not is_q(g)) for _ in range(CROWD - 3)]
    crowd_sig = int(rng.integers(1, 1 << 32))
    for g in crowd_q + crowd_d:
        set_sig(g, 0, crowd_sig)
    band(crowd_d[0], 0)[:] = band(crowd_q[0], 0)
    P.crowd = tuple(sorted(crowd_q + crowd_d))
    P.crowd_equal = tuple(sorted((crowd_q[0], crowd_d[0])))
    for x in range(CROWD):
        for y in range(x + 1, CROWD):
            P.pairs[(P.crowd[x], P.crowd[y])] = "C8"
    P.pairs[P.crowd_equal] = "C8="

    # C2 / C3: a collided band and an equal band, in both orders
    band_pairs = [(0, nb - 1)] + ([(3, 4), (63, 64), (4, 63)] if nb == 128 else [(0, nb - 1)])
    for cls in ("C2", "C3"):
        for (b0, b1), kind in zip(band_pairs, kinds(len(band_pairs))):
            i, k = take_good(kind)
            coll, equal = (b0, b1) if cls == "C2" else (b1, b0)
            collide(i, k, coll, int(rng.integers(r - 1)) if r > 1 else None)
            band(k, equal)[:] = band(i, equal)
            P.pairs[(i, k)] = cls

    # C7: triples on edge signatures
    vals = list(EDGE_SIGS)
    for v in (5, (1 << dir_bits) - 1):
        vals += [v << (32 - dir_bits), (v << (32 - dir_bits)) - 1]
    for t, sig in enumerate(vals):
        b = bands[t % len(bands)]
        if sig == 0:
            gs = [take(lambda g: is_q(g) and g < stale_cut), take(lambda g: not is_q(g) and g < stale_cut),
                  take(lambda g: not is_q(g) and g >= stale_cut)]
        else:
            gs = [take(is_q), take(lambda g: not is_q(g)), take(lambda g: not is_q(g))]
        for g in gs:
            set_sig(g, b, sig)
        gs = tuple(sorted(gs))
        P.triples.append((sig, b, gs))
        for x in range(3):
            for y in range(x + 1, 3):
                P.pairs[(gs[x], gs[y])] = "C7"

    # C4 / C5: half a signature
    for cls in ("C4", "C5"):
        for t, kind in enumerate(kinds(len(bands))):
            i, k = take_pair(kind)
            b = bands[t % len(bands)]
            half = int(rng.integers(1, 1 << 16))
            set_sig(k, b, band_sig(band(i, b)) ^ (half if cls == "C4" else half << 16))
            P.pairs[(i, k)] = cls

    # C6: every band collides
    for i, k in pinned["C6"] + [take_pair("db")]:
        for b in range(nb):
            set_sig(k, b, band_sig(band(i, b)))
        P.pairs[(i, k)] = "C6"

    # C1: one collided band, every position
    positions = c1_positions(r)
    places = list(pinned["C1"])
    while len(places) < max(len(positions), 3):
        places.append(take_pair("db" if len(places) == 2 else "cross"))
    for t, (i, k) in enumerate(places):
        b, pos = bands[t % len(bands)], positions[t % len(positions)]
        collide(i, k, b, pos)
        P.pairs[(i, k)] = "C1"
        P.detail[(i, k)] = (b, pos)
    return P
