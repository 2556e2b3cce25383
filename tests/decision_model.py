"""An exact model of the threshold decisions, and sketch sets whose CARDINALITIES are forged onto those thresholds (no GPU).

Everything a pass promises ends in a few IEEE-double comparisons with tau (a float widened to a double):
    CB       (double)e_lo / (double)e_hi >= tau                         criteria_sketch.hpp:45-49
    J        ((double)e1 + (double)e2 - t) / t >= tau                   selection.cpp:287-288
    hll_a    K+ = ((1 + gamma) * e_hi - t+) / t+ >= tau                 criteria_sketch.hpp:36-43,60-64
    hll_an   J^ + C >= tau                                              criteria_sketch.hpp:22-34,52-58
on TRUNCATED cardinalities e = (size_t)card.  With estimator outputs as cardinalities no pair lies within an ulp of tau; but the
cardinalities are a caller input of their own, so the boundary can be forged exactly -- as band-signature collisions are in sig_model.py.

What is exact here (fractions.Fraction, never the oracle): trunc_card, u64_to_f64 (round to nearest even), round_to_double, cb_ref
(ONE correctly rounded division), and every case's label: the exact real distance of e_lo / e_hi from tau in ulps of tau.  For J, hll_a and
hll_an the VALUE reference is the oracle's C restatement (oracle_py.Oracle: union_size, kota_mas, cota_n, hll_a, hll_an, jaccard); the
model only searches the forged integers around a given union estimate.

What a caller can reach.  A cardinality is a double, so a truncated cardinality of 2^53 or more IS a double: its conversion back never
rounds, and (double)e1 + (double)e2 equals (double)(e1 + e2) (one rounding of the same exact sum either way).  Integers that are no doubles
exist in this model only (`reachable` False): they show that the wrong variants of test_decision_model_host.py differ from the reference,
and no set carries them.  The conversion that does round on the device is hll_an's (double)(e_lo + e_hi), and the sets reach it.
"""
import math
from dataclasses import dataclass
from fractions import Fraction

import numpy as np

import sig_model as S

TAUS = (0.5, 0.8, 0.9, 0.95, 0.01)
TWO52, TWO53, TWO63 = 1 << 52, 1 << 53, 1 << 63


# ---- exact arithmetic ------------------------------------------------------------------------------------------------------------
def tau_double(tau):
    """the threshold every kernel compares with: the float widened to a double"""
    return float(np.float32(tau))


def tau_parts(tau):
    """(num, k): (double)(float)tau == num / 2^k in lowest terms"""
    f = Fraction(tau_double(tau))
    k = f.denominator.bit_length() - 1
    assert f.denominator == 1 << k
    return f.numerator, k


def trunc_card(card):
    """(size_t)card of a double in [0, 2^63): toward zero"""
    f = Fraction(card)
    assert 0 <= f < TWO63
    return f.numerator // f.denominator


def round_to_double(q, toward_zero=False):
    """the double nearest to the rational q >= 0, ties to even (normal range); toward_zero: the one at or below it"""
    q = Fraction(q)
    if q == 0:
        return 0.0
    n, d = q.numerator, q.denominator
    s = 52 - (n.bit_length() - d.bit_length())
    while True:
        a, b = (n << s, d) if s >= 0 else (n, d << -s)
        m, r = divmod(a, b)
        if m >= TWO53:
            s -= 1
        elif m < TWO52:
            s += 1
        else:
            break
    if not toward_zero and (2 * r > b or (2 * r == b and m & 1)):
        m += 1
    return math.ldexp(float(m), -s)


def u64_to_f64(e, toward_zero=False):
    return round_to_double(Fraction(int(e)), toward_zero)


def is_double(e):
    return int(float(e)) == int(e)


def cb_quotient(e_lo, e_hi):
    """gamma of criteria_sketch.hpp:47: both conversions, then ONE correctly rounded division"""
    return round_to_double(Fraction(u64_to_f64(e_lo)) / Fraction(u64_to_f64(e_hi)))


def cb_ref(tau, e_lo, e_hi):
    return cb_quotient(e_lo, e_hi) >= tau_double(tau)


def cb_distance(tau, e_lo, e_hi):
    """(e_lo / e_hi - tau) / ulp(tau), exact"""
    t = tau_double(tau)
    return (Fraction(int(e_lo), int(e_hi)) - Fraction(t)) / Fraction(math.ulp(t))


# ---- the wrong variants (test_decision_model_host.py shows that the cases tell each from the reference) ---------------------------
def cb_mul_compare(tau, e_lo, e_hi):
    """e_lo >= tau * e_hi: no divide in the search"""
    return u64_to_f64(e_lo) >= tau_double(tau) * u64_to_f64(e_hi)


def cb_trunc_divide(tau, e_lo, e_hi):
    """a division rounded toward zero"""
    return round_to_double(Fraction(u64_to_f64(e_lo)) / Fraction(u64_to_f64(e_hi)), toward_zero=True) >= tau_double(tau)


def cb_float_gamma(tau, e_lo, e_hi):
    """gamma held in a float"""
    return float(np.float32(cb_quotient(e_lo, e_hi))) >= tau_double(tau)


def cb_strict_greater(tau, e_lo, e_hi):
    return cb_quotient(e_lo, e_hi) > tau_double(tau)


def cb_trunc_convert(tau, e_lo, e_hi):
    """u64 -> f64 by dropping the low bits"""
    return round_to_double(Fraction(u64_to_f64(e_lo, True)) / Fraction(u64_to_f64(e_hi, True))) >= tau_double(tau)


def j_value(e1, e2, t):
    """selection.cpp:287 in Python doubles (the search; the oracle's jaccard() is the value reference of what the search finds)"""
    with np.errstate(all="ignore"):
        return float((np.float64(u64_to_f64(e1)) + np.float64(u64_to_f64(e2)) - np.float64(t)) / np.float64(t))


def j_value_sum_first(e1, e2, t):
    """(double)(e1 + e2) written for (double)e1 + (double)e2"""
    return (u64_to_f64(int(e1) + int(e2)) - t) / t


def j_value_trunc_convert(e1, e2, t):
    return (u64_to_f64(e1, True) + u64_to_f64(e2, True) - t) / t


# ---- CB cases --------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class CBCase:
    tau: float
    e_lo: int
    e_hi: int
    dist: Fraction                # exact (e_lo / e_hi - tau) / ulp(tau)
    accept: bool                  # the reference's side
    big: bool                     # e_hi in (2^53, 2^63)
    reachable: bool               # both integers are doubles: a card can carry them

    @property
    def kind(self):
        if self.dist == 0:
            return "on"
        if self.dist < 0:
            return "below-accepted" if self.accept else ("below-rejected" if self.dist > -1 else "far-rejected")
        return "above" if self.accept else "above-rejected"

    @property
    def convert_decides(self):
        """the roundings of the two conversions, not the value of e_lo / e_hi, decide: the correctly rounded EXACT quotient lies on the
        other side, or a truncating conversion does"""
        exact = round_to_double(Fraction(self.e_lo, self.e_hi)) >= tau_double(self.tau)
        return exact != self.accept or cb_trunc_convert(self.tau, self.e_lo, self.e_hi) != self.accept


def cb_case(tau, e_lo, e_hi):
    return CBCase(tau, int(e_lo), int(e_hi), cb_distance(tau, e_lo, e_hi), cb_ref(tau, e_lo, e_hi), e_hi > TWO53,
                  is_double(e_lo) and is_double(e_hi))


def cb_solve(tau, d, near):
    """(e_lo, e_hi), e_hi the first integer >= near with e_lo * 2^k - num * e_hi == d (tau = num / 2^k): e_lo / e_hi lies d / (2^k e_hi)
    from tau.  num is odd (or tau = 1/2), so e_hi comes from a modular inverse"""
    num, k = tau_parts(tau)
    M = 1 << k
    r = (-d * pow(num, -1, M)) % M
    e_hi = near + ((r - near) % M)
    assert (num * e_hi + d) % M == 0
    return (num * e_hi + d) >> k, e_hi


_CB_CACHE = {}


def cb_cases(tau):
    """every kind of pair around tau, e_hi from 2^32 to 2^63.
      d = 0                     exactly on the threshold (e_hi = 2 e_lo at tau = 0.5)
      d = -1 .. -3              below tau by less than half an ulp once e_hi > |d| 2^31: the quotient rounds to tau, accepted
      d = -c ulp(tau) e_hi 2^k  c = 0.3 .. 0.49 accepted, 0.51 .. 0.95 rejected within one ulp.  A multiply-and-compare differs from the
                                division for e_hi just above a power of two and c between 1 / (2 (1 + f)) and 1 / 2 (f = the fraction
                                of e_hi above that power): tau * e_hi then rounds UP from e_lo
      d = +1                    the first integer pair above
    2^53 and beyond: every small case scaled by a power of two (the same quotient, both integers still doubles: reachable), and
    integers that are no doubles around the scaled ones, where the conversions round (model only).
    tau = 0.5: e_lo / e_hi = 1/2 + d / (2 e_hi) is at least an ulp from 1/2 for every d != 0 and e_hi < 2^53, so only "on" exists below
    2^53; the kinds within an ulp come from the integers beyond 2^53 that are no doubles."""
    if tau in _CB_CACHE:
        return _CB_CACHE[tau]
    _, k = tau_parts(tau)
    u = Fraction(math.ulp(tau_double(tau)))
    seen, out = set(), []

    def add(e_lo, e_hi):
        if 0 < e_lo <= e_hi < TWO63 and (e_lo, e_hi) not in seen:
            seen.add((e_lo, e_hi))
            c = cb_case(tau, e_lo, e_hi)
            if abs(c.dist) < 2:
                out.append(c)

    small = []
    for a in range(32, 52, 1):
        for f in (1.0, 1.04, 1.5, 1.96):
            near = int(f * (1 << a))
            ds = [0, 1, -1, -2, -3]
            for c in (0.3, 0.45, 0.49, 0.51, 0.55, 0.75, 0.95):
                d = -int(c * u * near * (1 << k))
                if d < -3:
                    ds.append(d)
            for d in ds:
                e_lo, e_hi = cb_solve(tau, d, near)
                if e_hi < TWO52:
                    add(e_lo, e_hi)
                    small.append((e_lo, e_hi))
    for t, (e_lo, e_hi) in enumerate(small):
        # scaled into (2^53, 2^63): the shift walks through the ten binades
        sh = 54 + t % 9 - e_hi.bit_length()
        if sh > 0:
            add(e_lo << sh, e_hi << sh)
    rng = np.random.default_rng(0xDEC1 + int(tau * 1000))
    for a in range(54, 63):
        for f in (1.0, 1.5):
            for d in (0, 1, -1, -int(Fraction(3, 4) * u * int(f * (1 << a)) * (1 << k))):
                e_lo, e_hi = cb_solve(tau, d, int(f * (1 << a)))
                h_hi, h_lo = 1 << (e_hi.bit_length() - 54), 1 << max(e_lo.bit_length() - 54, 0)      # half an ulp of either integer
                for _ in range(12):
                    pick = lambda h: int(rng.choice([0, 1, -1, h - 1, h, h + 1, -h + 1, -h, -h - 1]))      # noqa: E731
                    add(e_lo + pick(h_lo), e_hi + pick(h_hi))
    _CB_CACHE[tau] = out
    return out


def cb_counts(tau, reachable=None):
    """{(kind, big): cases} of cb_cases(tau); reachable None = all, True / False = only those"""
    cnt = {}
    for c in cb_cases(tau):
        if reachable is None or c.reachable == reachable:
            cnt[(c.kind, c.big)] = cnt.get((c.kind, c.big), 0) + 1
    return cnt


# ---- sketches --------------------------------------------------------------------------------------------------------------------
def small_main_rows(n, rng, p=14):
    """main sketches with a few non-zero registers: every union estimate is in the hundreds, so J of cards beyond 2^31 is far above
    any tau and every pair that reaches the Jaccard test yields a record -- a wrong pair is NAMED"""
    hll = np.zeros((n, 1 << p), dtype=np.uint8)
    for g in range(n):
        idx = rng.choice(1 << p, size=int(rng.integers(100, 300)), replace=False)
        hll[g, idx] = rng.integers(1, 4, size=idx.size)
    return hll


def high_rows(n, base, rng, p=14):
    """registers drawn from [base - 2, base + 2]: the union estimate of two of them is about 2^p 2^base"""
    return rng.integers(base - 2, base + 3, size=(n, 1 << p)).astype(np.uint8)


def shared_band_aux(n, m, r, rng):
    """random buckets with band 0 equal in every row: every pair clears smh_a, and only the cardinalities vary"""
    aux = rng.integers(0, 1 << 64, size=(n, m), dtype=np.uint64)
    aux[:, :r] = aux[0, :r]
    assert all(S.literal_smh_a(aux[0], aux[g], r, m // r) for g in range(n))
    return aux


# ---- CB sets ---------------------------------------------------------------------------------------------------------------------
def just_below_next(e):
    """the largest double below e + 1: a card that truncates to e and ROUNDS to e + 1 (e < 2^52)"""
    return float(np.nextafter(np.float64(e + 1), 0.0))


@dataclass
class CardSet:
    """cards (ascending, as forged) with the ranks of the forged pairs"""
    tau: float
    cards: np.ndarray               # float64[n]
    forged: list                    # (rank of e_lo's last copy, rank of e_hi's first copy, CBCase)
    inside: bool


def _spaced(cases, tau, limit):
    """up to `limit` cases in ascending order whose clusters do not meet (each e_lo more than 2 / tau above the last e_hi), the kinds
    taken in turn"""
    gap = Fraction(2) / Fraction(tau_double(tau))
    out, top, count = [], 0, {}
    while len(out) < limit:
        ok = [c for c in cases if c.e_lo > top * gap]
        if not ok:
            break
        floor = min(c.e_hi for c in ok)
        c = min((c for c in ok if c.e_hi <= 8 * floor), key=lambda c: (count.get((c.kind, c.big), 0), c.e_hi))
        count[(c.kind, c.big)] = count.get((c.kind, c.big), 0) + 1
        out.append(c)
        top = c.e_hi
    return out


def pick_cb_cases(tau, accept):
    """the reachable cases of one side within an ulp of tau"""
    return [c for c in cb_cases(tau) if c.reachable and c.accept == accept and c.kind != "far-rejected"]


def _run_of(e, copies):
    """`copies` ascending cards that all truncate to e: e, e + 0.5 and just_below_next(e) where doubles have room for a fraction"""
    if e < TWO52:
        return [float(e), e + 0.5, just_below_next(e)][:copies]
    return [float(e)] * copies


def cb_sets(tau, accept, n_sets=4, per_set=14):
    """CardSets of one side (accept: every forged pair inside CB; else every forged pair outside), fewer than 200 cards each:
      * zeros first: cards in (0, 1) truncate to 0 and are no candidates;
      * fillers 2.5 * 1.3^j (few of them within 1 / tau of each other), so that the first forged pair lies across ranks 63 | 64 (two waves);
      * per forged pair a cluster [e_lo ... e_lo | (cards between, inside sets) | e_hi ... e_hi]: runs of equal e on either side of the
        boundary, written as e, e + 0.5 and just_below_next(e) below 2^52 (truncation, not rounding, keeps them equal);
      * clusters alternate between the partner at rank i + 1 and some ranks away; the last cluster ends the set: its partner is the
        LAST rank."""
    remaining = pick_cb_cases(tau, accept)
    kinds = {(c.kind, c.big) for c in remaining}
    sets = []
    while remaining and len(sets) < 2 * n_sets:
        shown = {(c.kind, c.big) for cs in sets for _, _, c in cs.forged}
        if len(sets) >= n_sets:                                              # further sets only for the kinds none has shown yet
            if shown == kinds:
                break
            remaining = [c for c in remaining if (c.kind, c.big) not in shown]
        chosen = _spaced(remaining, tau, per_set)
        remaining = [c for c in remaining if c not in chosen]
        cards, forged = [5e-324, 0.25, just_below_next(0)], []
        for t, c in enumerate(chosen):
            lo_run, hi_run = _run_of(c.e_lo, 1 + t % 3), _run_of(c.e_hi, 1 + (t + 1) % 3)
            between = []
            if t == 0:
                cards += [2.5 * 1.3 ** j for j in range(63 - (len(cards) + len(lo_run) - 1))]
            elif accept and t % 2 == 1 and c.e_hi - c.e_lo > 8:
                step = (c.e_hi - c.e_lo) // 4
                between = [b for b in (float(c.e_lo + step), float(c.e_lo + 2 * step)) if c.e_lo < trunc_card(b) < c.e_hi]
            lo_rank = len(cards) + len(lo_run) - 1
            cards += lo_run + between
            forged.append((lo_rank, len(cards), c))
            cards += hi_run
        arr = np.array(cards, dtype=np.float64)
        assert len(arr) < 200 and np.all(np.diff(arr) >= 0)
        assert forged[0][:2] == (63, 64) and forged[-1][1] + len(hi_run) == len(arr)
        sets.append(CardSet(tau, arr, forged, accept))
    return sets


def split_for_queries(cs):
    """(query ranks, database ranks) of a CardSet: per cluster one side goes to the queries and the other to the database, alternating,
    so the partner lies above P (= the first database genome beyond the query) and below it in turn; the FIRST cluster's e_lo and the
    LAST cluster's e_hi are database genomes -- the partner at the first and at the last database rank; a copy of a run stays on the
    other side where the run has several (a query equal to the database's boundary genome); the zeros and the fillers are queries"""
    n = len(cs.cards)
    e = [trunc_card(c) for c in cs.cards]
    is_q = np.ones(n, dtype=bool)
    last = len(cs.forged) - 1
    for t, (lo_rank, hi_rank, c) in enumerate(cs.forged):
        lo_ranks = [g for g in range(n) if e[g] == c.e_lo]
        hi_ranks = [g for g in range(n) if e[g] == c.e_hi]
        lo_in_db = t == 0 or (t != last and t % 2 == 0)
        db, qq = (lo_ranks, hi_ranks) if lo_in_db else (hi_ranks, lo_ranks)
        is_q[db] = False
        if len(qq) > 1:
            is_q[qq[0] if lo_in_db is False else qq[-1]] = False             # the database holds a copy of the query's own e too
        for g in range(lo_rank + 1, hi_rank):                                # the cards between: database
            is_q[g] = False
    q = np.nonzero(is_q)[0]
    d = np.nonzero(~is_q)[0]
    return q, d


# ---- J cases ---------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class JCase:
    tau: float
    e1: int
    e2: int
    t: float
    j: float                      # selection.cpp:287 in doubles
    side: int                     # -1: the nearest J below tau reached, 0: J == tau, +1: the nearest above

    @property
    def accept(self):
        return self.j >= tau_double(self.tau)


def _doubles_near(x, span):
    x = np.float64(x)
    lo = x
    for _ in range(span):
        lo = np.nextafter(lo, -np.inf)
    out = []
    for _ in range(2 * span + 1):
        out.append(float(lo))
        lo = np.nextafter(lo, np.inf)
    return out


def forge_j(tau, t, span=48):
    """{-1, 0, +1} -> JCase for a pair of main rows with union estimate t (finite, > 0): integers e1 <= e2, both doubles, nearly equal
    (so the pair clears CB at any tau), with J == tau exactly (0, where some x = fl(e1 + e2) - t with fl(x / t) == tau can be formed
    from two doubles) and the nearest J on either side that such pairs reach"""
    td = tau_double(tau)
    best = {}
    for x in _doubles_near(td * t, span):
        total = Fraction(x) + Fraction(t)
        base = total.numerator // total.denominator
        for s in (base - 1, base, base + 1, base + 2):
            e1 = int(float(s // 2))
            for e1 in (e1, int(np.nextafter(np.float64(e1), 0.0))):
                e2 = s - e1
                if not (0 < e1 < TWO63 and 0 < e2 < TWO63 and is_double(e2)):
                    continue
                lo, hi = min(e1, e2), max(e1, e2)
                j = j_value(lo, hi, t)
                side = 0 if j == td else (-1 if j < td else 1)
                cur = best.get(side)
                if cur is None or (side and abs(j - td) < abs(cur.j - td)):
                    best[side] = JCase(tau, lo, hi, t, j, side)
    return best


def sum_order_case(tau, t, span=4096):
    """model only: integers e1, e2 > 2^53 that are NO doubles, for which (double)e1 + (double)e2 and (double)(e1 + e2) put J on opposite
    sides of tau -- the two forms differ only on integers a card cannot carry.  None if t is too small for them"""
    td = tau_double(tau)
    total = int(Fraction(td * t) + Fraction(t))
    if total // 2 <= TWO53:
        return None
    a = total // 2
    for delta in range(1, span):
        for s in (total - 2048 + delta, total + delta):
            e1, e2 = a - delta, s - (a - delta)
            j_ref, j_mut = j_value(e1, e2, t), j_value_sum_first(e1, e2, t)
            if (j_ref >= td) != (j_mut >= td):
                return e1, e2, j_ref, j_mut
    return None


# ---- hll_a / hll_an cases --------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class AuxCase:
    crit: str                     # "hll_a" | "hll_an"
    tau: float
    p_aux: int
    pair: int                     # which pair of auxiliary rows
    e_lo: int
    e_hi: int
    union: tuple                  # (U strict, U fma)
    value: tuple                  # (K+ or J^ + C: strict, fma)
    accept: tuple                 # (strict, fma)


def aux_value(oracle, crit, e_lo, e_hi, U, p_aux):
    if crit == "hll_a":
        return oracle.kota_mas(e_lo, e_hi, U, p_aux)
    j_hat = (u64_to_f64(int(e_lo) + int(e_hi)) - U) / U                       # criteria_sketch.hpp:55
    return j_hat + oracle.cota_n(e_lo, e_hi, U, p_aux)


def aux_decide(oracle, crit, tau, e_lo, e_hi, U, p_aux):
    return (oracle.hll_a if crit == "hll_a" else oracle.hll_an)(tau, e_lo, e_hi, U, p_aux)


def forge_aux(oracle, crit, tau, row_a, row_b, p_aux, pair, window=40):
    """AuxCases for one pair of auxiliary rows: e_hi fixed (a double near 0.55 of the sum the criterion needs), e_lo scanned over the
    consecutive DOUBLES around the place where the oracle's decision flips (found by bisection, per flavour): the cases whose value
    equals tau, the nearest value on either side, and every e_lo on which the two flavours decide differently"""
    td = tau_double(tau)
    U = []
    for fma in (0, 1):
        oracle.set_fma(fma)
        U.append(oracle.union_size(row_a, row_b, p_aux))
    oracle.set_fma(1)
    assert all(math.isfinite(u) and 0 < u < TWO63 for u in U), U
    zs = 1.96 * oracle.lib.orc_sigma(p_aux)
    # about the e_lo + e_hi at which the decision flips
    need = (1 + td) * U[1] / (1 + zs) if crit == "hll_a" else (1 + td - min(1.0, (1 + zs) * 0.9) * 1.9 * zs) * U[1]
    def ends(e_hi, step, fma):
        """the decision at the two ends of the scan: it must be False at the smallest e_lo and True at e_lo = e_hi"""
        top = (e_hi // step) * step
        return aux_decide(oracle, crit, tau, step, e_hi, U[fma], p_aux), aux_decide(oracle, crit, tau, top, e_hi, U[fma], p_aux)

    for share in (0.55, 0.65, 0.8, 1.0, 1.3):                                 # e_hi's share of that sum: the first that brackets the flip
        e_hi = int(float(int(share * need)))
        step = max(1, int(math.ulp(float(e_hi // 2 + 1))))                   # e_lo stays below e_hi, at most one binade down
        ok = True
        for fma in (0, 1):
            oracle.set_fma(fma)
            ok = ok and ends(e_hi, step, fma) == (False, True)
        if ok and e_hi < TWO63:
            break
    else:
        oracle.set_fma(1)
        return []

    def grid(j):
        return j * step

    flips = []
    for fma in (0, 1):
        oracle.set_fma(fma)
        lo, hi = 1, e_hi // step
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if aux_decide(oracle, crit, tau, grid(mid), e_hi, U[fma], p_aux):
                hi = mid
            else:
                lo = mid
        flips.append(hi)
    rows = []
    for j in range(min(flips) - window, max(flips) + window + 1):
        e_lo = grid(j)
        if not (0 < e_lo <= e_hi and is_double(e_lo)):
            continue
        val, acc = [], []
        for fma in (0, 1):
            oracle.set_fma(fma)
            val.append(aux_value(oracle, crit, e_lo, e_hi, U[fma], p_aux))
            acc.append(aux_decide(oracle, crit, tau, e_lo, e_hi, U[fma], p_aux))
        rows.append(AuxCase(crit, tau, p_aux, pair, e_lo, e_hi, tuple(U), tuple(val), tuple(acc)))
    oracle.set_fma(1)
    keep = {}
    for fma in (0, 1):
        below = [c for c in rows if c.value[fma] < td]
        above = [c for c in rows if c.value[fma] > td]
        on = [c for c in rows if c.value[fma] == td]
        if below:
            keep[max(below, key=lambda c: (c.value[fma], c.e_lo)).e_lo] = None
        if above:
            keep[min(above, key=lambda c: (c.value[fma], c.e_lo)).e_lo] = None
        for c in on[:2] + on[-1:]:
            keep[c.e_lo] = None
    for c in [c for c in rows if c.accept[0] != c.accept[1]][:3]:
        keep[c.e_lo] = None
    return [c for c in rows if c.e_lo in keep]


def aux_rows(n_pairs, p_aux, bases, rng):
    """pairs of auxiliary rows with registers in [base - 2, base + 2]: union estimates of about 2^p_aux 2^base"""
    out = []
    for t in range(n_pairs):
        base = bases[t % len(bases)]
        out.append(rng.integers(base - 2, base + 3, size=(2, 1 << p_aux)).astype(np.uint8))
    return out


def aux_bases(p_aux):
    """register levels whose union estimates run from about 2^50 to 2^61: finite and below 2^63 (beyond, the reference's size_t
    conversion is undefined: DESIGN.md)"""
    return [b - p_aux for b in (50, 52, 53, 54, 55, 57, 59, 61)]


# ---- sets of genomes -------------------------------------------------------------------------------------------------------------
@dataclass
class GenomeSet:
    """sketches in the order of their forged cards (the rows follow the cards)"""
    cards: np.ndarray               # float64[n] ascending
    hll: np.ndarray                 # uint8[n, 2^14]
    aux: np.ndarray                 # uint64[n, m], band 0 shared
    aux_hll: np.ndarray             # uint8[n, 2^p_aux] or None
    forged: list                    # (rank, rank, case): the forged pairs
    r: int
    nb: int


def assemble(genomes, pairs, m, r, rng):
    """genomes: (card, main row, auxiliary row or None) each; pairs: (index, index, case) into them.  Stable sort by card"""
    cards = np.array([g[0] for g in genomes], dtype=np.float64)
    order = np.argsort(cards, kind="stable")
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    hll = np.stack([genomes[g][1] for g in order])
    aux_hll = np.stack([genomes[g][2] for g in order]) if genomes[0][2] is not None else None
    forged = [(int(min(rank[a], rank[b])), int(max(rank[a], rank[b])), c) for a, b, c in pairs]
    return GenomeSet(cards[order], hll, shared_band_aux(len(order), m, r, rng), aux_hll, forged, r, m // r)


def cb_genome_set(cs, seed, m=64, r=8):
    rng = np.random.default_rng(seed)
    hll = small_main_rows(len(cs.cards), rng)
    return GenomeSet(cs.cards, hll, shared_band_aux(len(cs.cards), m, r, rng), None, cs.forged, r, m // r)


J_BASES = (38, 40, 42, 44, 46, 47, 48)


def j_genome_sets(oracle, tau, seed, m=64, r=8):
    """(inside set, outside set, cases): per base of J_BASES a pair of high main rows and its forged (e1, e2) -- J == tau and the nearest
    J above go inside, the nearest J below outside; each case on rows of its own (copies of the pair's two rows).  Two more pairs at
    the extremes: both rows saturated (t = +inf, J is a NaN: rejected, outside) and both rows empty (t = 0, J = +inf: accepted with
    +inf in the record, inside)"""
    rng = np.random.default_rng(seed)
    inside, outside, in_pairs, out_pairs, cases = [], [], [], [], []
    for base in J_BASES:
        a, b = high_rows(2, base, rng)
        t = oracle.union_size(a, b)
        for side, c in sorted(forge_j(tau, t).items()):
            dest, prs = (inside, in_pairs) if c.accept else (outside, out_pairs)
            prs.append((len(dest), len(dest) + 1, c))
            dest += [(float(c.e1), a, None), (float(c.e2), b, None)]
            cases.append(c)
    full = np.full(1 << 14, 64 - 14 + 1, dtype=np.uint8)
    empty = np.zeros(1 << 14, dtype=np.uint8)
    e = float(3 << 40)
    out_pairs.append((len(outside), len(outside) + 1, JCase(tau, int(e), int(e) + 1, math.inf, math.nan, -1)))
    outside += [(e, full, None), (e + 1, full, None)]
    in_pairs.append((len(inside), len(inside) + 1, JCase(tau, int(e), int(e) + 1, 0.0, math.inf, 1)))
    inside += [(e, empty, None), (e + 1, empty, None)]
    return assemble(inside, in_pairs, m, r, rng), assemble(outside, out_pairs, m, r, rng), cases


def j_low_genome_sets(oracle, tau, seed, base=29, pool=96, want=3, m=64, r=8):
    """(inside set, outside set, cases) for the one-launch pass of small sets, which takes main registers below 32 only: t is then below
    2^46, e1 + e2 is an integer below 2^53 and converts exactly, so J moves in steps of 1 / t (about 2^-44) and x = e1 + e2 - t cannot be
    chosen freely.  J == tau needs a pair of rows whose (1 + tau) t lies within t ulp(tau) / 2 of an integer -- about one pair in 2^10 at
    t = 2^43: the pairs of a pool of rows are searched for them.  Per hit: J == tau and one step above (inside), one step below (outside);
    and the pair of empty rows (t = 0, J = +inf, inside)"""
    rng = np.random.default_rng(seed)
    rows = high_rows(pool, base, rng)
    assert rows.max() < 32
    td = tau_double(tau)
    inside, outside, in_pairs, out_pairs, cases = [], [], [], [], []
    hits = 0
    for a in range(pool):
        for b in range(a + 1, pool):
            if hits == want:
                break
            t = oracle.union_size(rows[a], rows[b])
            s = round((1 + Fraction(td)) * Fraction(t))
            e1 = s // 2
            if j_value(e1, s - e1, t) != td:
                continue
            hits += 1
            for side, e2 in ((-1, s - e1 - 1), (0, s - e1), (1, s - e1 + 1)):
                c = JCase(tau, e1, e2, t, j_value(e1, e2, t), side)
                assert c.accept == (side >= 0) and (c.j == td) == (side == 0)
                dest, prs = (inside, in_pairs) if c.accept else (outside, out_pairs)
                prs.append((len(dest), len(dest) + 1, c))
                dest += [(float(e1), rows[a], None), (float(e2), rows[b], None)]
                cases.append(c)
    empty = np.zeros(1 << 14, dtype=np.uint8)
    e = float(3 << 40)
    in_pairs.append((len(inside), len(inside) + 1, JCase(tau, int(e), int(e) + 1, 0.0, math.inf, 1)))
    inside += [(e, empty, None), (e + 1, empty, None)]
    if not outside:
        return assemble(inside, in_pairs, m, r, rng), None, cases
    return assemble(inside, in_pairs, m, r, rng), assemble(outside, out_pairs, m, r, rng), cases


def aux_seed(crit, tau, p_aux):
    """one seed per configuration: the host tests count the coverage of the very sets the device tests upload"""
    return 0xA0 + p_aux + int(tau * 10) + (100 if crit == "hll_an" else 0)


def aux_genome_sets(oracle, crit, tau, p_aux, seed=None, n_pairs=8, m=64, r=8):
    """{(flavour, accept): GenomeSet} and the cases: per pair of auxiliary rows its forged (e_lo, e_hi), each case on rows of its own;
    the main rows are small, so whatever clears the criterion yields a record"""
    rng = np.random.default_rng(aux_seed(crit, tau, p_aux) if seed is None else seed)
    rows = aux_rows(n_pairs, p_aux, aux_bases(p_aux), rng)
    cases = [c for t, (a, b) in enumerate(rows) for c in forge_aux(oracle, crit, tau, a, b, p_aux, t)]
    main = small_main_rows(2, rng)
    sets = {}
    for fma in (0, 1):
        for accept in (False, True):
            genomes, pairs = [], []
            for c in cases:
                if c.accept[fma] == accept:
                    pairs.append((len(genomes), len(genomes) + 1, c))
                    genomes += [(float(c.e_lo), main[0], rows[c.pair][0]), (float(c.e_hi), main[1], rows[c.pair][1])]
            if genomes:
                sets[(fma, accept)] = assemble(genomes, pairs, m, r, rng)
    return sets, cases
