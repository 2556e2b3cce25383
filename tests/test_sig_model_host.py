"""tests/sig_model.py checked on its own (no GPU): the inverse of the hash, the forged last bucket, the window model, and -- for every
band shape the collision tests run -- that every class of planted_set has the property it is listed with."""
import numpy as np
import pytest

import sig_model as S

TARGETS = (0x00000000, 0xFFFFFFFF, 0x80000000, 0x0000FFFF, 0xFFFF0000)
N = 200


def test_mix64_known_value_and_inverse():
    # mix64 is the output function of SplitMix64: its first output for state 0 is the mix of the increment
    assert S.mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    rng = np.random.default_rng(1)
    xs = [0, S.MASK64, 1, 1 << 63] + [int(v) for v in rng.integers(0, 1 << 64, size=2000, dtype=np.uint64)]
    for x in xs:
        assert S.unmix64(S.mix64(x)) == x and S.mix64(S.unmix64(x)) == x
    arr = np.array(xs, dtype=np.uint64)
    assert np.array_equal(S.mix64(arr), np.array([S.mix64(x) for x in xs], dtype=np.uint64))      # array form == integer form
    assert np.array_equal(S.unmix64(S.mix64(arr)), arr)


@pytest.mark.parametrize("r", [1, 2, 4, 8, 16, 32, 64, 128])
def test_forge_last_hits_target(r):
    rng = np.random.default_rng(100 + r)
    for target in TARGETS + tuple(int(v) for v in rng.integers(0, 1 << 32, size=3)):
        prefix = rng.integers(0, 1 << 64, size=r - 1, dtype=np.uint64)
        a, b = S.forge_last(prefix, target, rng), S.forge_last(prefix, target, rng)
        assert a.shape == (r,) and np.array_equal(a[:-1], prefix) and np.array_equal(b[:-1], prefix)
        assert S.band_sig(a) == target and S.band_sig(b) == target
        assert a[-1] != b[-1]                                                  # same signature, different contents
        # the array form of the signature, with the forged band in every band position of a genome
        for nb in (1, 8):
            row = rng.integers(0, 1 << 64, size=(2, r * nb), dtype=np.uint64)
            row[0, (nb - 1) * r:] = a
            row[1, :r] = b
            sg = S.band_sigs(row, r, nb)
            assert sg.dtype == np.uint32 and sg[0, nb - 1] == target and sg[1, 0] == target


def test_band_sigs_two_ways():
    rng = np.random.default_rng(7)
    for r, nb in ((1, 8), (2, 32), (16, 8), (128, 2)):
        aux = rng.integers(0, 1 << 64, size=(5, r * nb), dtype=np.uint64)
        sg = S.band_sigs(aux, r, nb)
        for g in range(5):
            for b in range(nb):
                assert int(sg[g, b]) == S.band_sig(aux[g, b * r:(b + 1) * r])


def test_window_model():
    rng = np.random.default_rng(3)
    cards = np.sort(np.concatenate([np.zeros(3), rng.uniform(0.2, 50.0, 5), rng.uniform(1e3, 1e5, 80)]))
    e = S.trunc_cards(cards)
    n = len(cards)
    for tau, use_cb in ((0.0, False), (0.5, True), (0.9, True), (0.0, True)):
        lo, hi = S.allpairs_windows(cards, tau, use_cb)
        want = np.zeros((n, n), dtype=bool)
        for i in range(n):
            for k in range(i + 1, n):
                want[i, k] = e[k] != 0 and (not use_cb or float(e[i]) / float(e[k]) >= float(np.float32(tau)))
        assert np.array_equal(S.window_mask(lo, hi, n), want)
        assert S.window_mask(lo, hi, n, rows=(10, 20)).sum() == want[10:20].sum()
        cq, cd = cards[::3], np.delete(cards, np.arange(0, n, 3))
        lo, hi = S.query_windows(cq, cd, tau, use_cb)
        eq, ed = S.trunc_cards(cq), S.trunc_cards(cd)
        want = np.zeros((len(cq), len(cd)), dtype=bool)
        for q in range(len(cq)):
            for d in range(len(cd)):
                e_lo, e_hi = min(eq[q], ed[d]), max(eq[q], ed[d])
                want[q, d] = e_hi != 0 and (not use_cb or float(e_lo) / float(e_hi) >= float(np.float32(tau)))
        assert np.array_equal(S.window_mask(lo, hi, len(cd)), want)


def test_shapes_of_the_collision_tests():
    """one-bucket bands, the tiled build's 2 .. 32 rows, 128 bands, bands longer than 16 rows, the serial build above 64 rows"""
    assert [(r, nb) for _, r, nb in S.SHAPES] == [(1, 64), (2, 32), (8, 16), (16, 8), (4, 128), (32, 16), (64, 8), (128, 8)]
    assert all(m == r * nb for m, r, nb in S.SHAPES)


def test_c1_positions_cover_lanes_and_steps():
    for r in (1, 2, 4, 8, 16, 32, 64, 128):
        pos = S.c1_positions(r)
        assert pos[0] is None and len(set(pos)) == len(pos) and all(0 <= j < r - 1 for j in pos[1:])
        if r <= 32:
            assert pos[1:] == list(range(r - 1))
        else:
            # (position r - 1, the compensating bucket, differs in every pair: lane 15 of the last step)
            assert {j % 16 for j in pos[1:]} | {15} == set(range(16)) and {j // 16 for j in pos[1:]} == set(range(r // 16))
            assert len(pos) <= 32


@pytest.mark.parametrize("m,r,nb", S.SHAPES)
def test_planted_classes_cover(m, r, nb):
    """every class has the property it claims under band_sigs and literal_smh_a; the model's count over the whole set = the classes'
    candidates + whatever the random background matches by accident"""
    rng = np.random.default_rng(m + r)
    good = rng.random((N, N)) < 0.6
    for dir_bits, use_good in ((6, None), (5, good)):
        P = S.planted_set(N, m, r, nb, seed=0xC011 + r, dir_bits=dir_bits, good=use_good)
        aux, sg = P.aux, S.band_sigs(P.aux, r, nb)
        band = lambda g, b: aux[g, b * r:(b + 1) * r]                          # noqa: E731
        eq_sig = lambda i, k: np.nonzero(sg[i] == sg[k])[0].tolist()            # noqa: E731
        eq_band = lambda i, k: [b for b in range(nb) if np.array_equal(band(i, b), band(k, b))]      # noqa: E731
        assert all(i < k for i, k in P.pairs)
        # the classes sit on disjoint genomes
        groups = [set(P.crowd)] + [set(t[2]) for t in P.triples] + [set(p) for p, c in P.pairs.items() if c not in ("C7", "C8", "C8=")]
        assert sum(len(g) for g in groups) == len(set().union(*groups)) <= N

        # C1: one band collides, the contents differ in exactly the listed position and the last bucket
        c1 = P.of("C1")
        assert [P.detail[p][1] for p in c1 if P.detail[p][1] is None] and {P.detail[p][1] for p in c1} == set(S.c1_positions(r))
        assert {P.detail[p][0] for p in c1} == set(S.planted_bands(nb)[:len(c1)])
        for i, k in c1:
            b, pos = P.detail[(i, k)]
            assert eq_sig(i, k) == [b] and eq_band(i, k) == []
            diff = np.nonzero(band(i, b) != band(k, b))[0].tolist()
            assert diff == ([r - 1] if pos is None else [pos, r - 1])
            assert not S.literal_smh_a(aux[i], aux[k], r, nb)
        # C2 / C3: a collided band before / after an equal one
        for cls in ("C2", "C3"):
            prs = P.of(cls)
            assert len(prs) >= 2
            for i, k in prs:
                s, e = eq_sig(i, k), eq_band(i, k)
                assert len(s) == 2 and len(e) == 1
                assert e[0] == (s[1] if cls == "C2" else s[0])
                assert S.literal_smh_a(aux[i], aux[k], r, nb)
        if nb == 128:
            for cls in ("C2", "C3"):
                assert {(eq_sig(i, k)[0], eq_sig(i, k)[1]) for i, k in P.of(cls)} == {(0, 127), (3, 4), (63, 64), (4, 63)}
        # C4 / C5: half a signature, neither candidate nor survivor
        for cls in ("C4", "C5"):
            prs = P.of(cls)
            assert len(prs) == len(S.planted_bands(nb))
            for i, k in prs:
                x = sg[i] ^ sg[k]
                half = (x >> 16 == 0) if cls == "C4" else (x & 0xFFFF == 0)
                assert half.sum() == 1 and eq_sig(i, k) == [] and not S.literal_smh_a(aux[i], aux[k], r, nb)
            assert {int(np.nonzero((sg[i] ^ sg[k]) >> 16 == 0 if cls == "C4" else (sg[i] ^ sg[k]) & 0xFFFF == 0)[0][0]) for i, k in prs} \
                == set(S.planted_bands(nb))
        # C6: every band collides, none is equal
        assert len(P.of("C6")) == 2
        for i, k in P.of("C6"):
            assert eq_sig(i, k) == list(range(nb)) and eq_band(i, k) == [] and not S.literal_smh_a(aux[i], aux[k], r, nb)
        # C7: triples on the edge signatures and the index directory's bucket boundaries
        last = (1 << dir_bits) - 1
        assert [t[0] for t in P.triples] == list(S.EDGE_SIGS) + [5 << (32 - dir_bits), (5 << (32 - dir_bits)) - 1,
                                                                  last << (32 - dir_bits), (last << (32 - dir_bits)) - 1]
        for sig, b, gs in P.triples:
            assert all(int(sg[g, b]) == sig for g in gs)
            for x in range(3):
                for y in range(x + 1, 3):
                    assert P.pairs[(gs[x], gs[y])] == "C7" and eq_band(gs[x], gs[y]) == [] and b in eq_sig(gs[x], gs[y])
        zero = P.triples[0][2]
        assert sum(g < 130 for g in zero) == 2
        # C8: the crowd
        assert len(P.crowd) == S.CROWD and len(set(int(sg[g, 0]) for g in P.crowd)) == 1
        crowd_pairs = [(P.crowd[x], P.crowd[y]) for x in range(S.CROWD) for y in range(x + 1, S.CROWD)]
        assert len(crowd_pairs) == 2415 and all(P.pairs[p] in ("C8", "C8=") for p in crowd_pairs)
        assert [p for p in crowd_pairs if S.literal_smh_a(aux[p[0]], aux[p[1]], r, nb)] == [P.crowd_equal] == P.of("C8=")
        assert sum(g % 3 == 0 for g in P.crowd) == 3 and (P.crowd_equal[0] % 3 == 0) != (P.crowd_equal[1] % 3 == 0)

        # the whole set: candidates = the classes' + the accidental matches of the background; survivors likewise
        match = np.triu(S.sig_match_matrix(sg, sg), 1)
        lit = np.triu(S.literal_matrix(aux, aux, r, nb), 1)
        planted = set(P.of(*S.CANDIDATE_CLASSES))
        assert all(match[p] for p in planted) and not any(match[p] for p in P.of("C4", "C5"))
        accidental = {(int(i), int(k)) for i, k in zip(*np.nonzero(match))} - planted
        lo, hi = S.allpairs_windows(np.arange(1.0, N + 1), 0.0, False)
        assert S.expected_candidates(sg, lo, hi) == len(planted) + len(accidental)
        assert len(planted) == 2415 + 3 * 8 + len(P.of("C1", "C2", "C3", "C6"))
        survivors = {(int(i), int(k)) for i, k in zip(*np.nonzero(lit))}
        assert set(P.of(*S.SURVIVOR_CLASSES)) <= survivors and not (survivors - set(P.of(*S.SURVIVOR_CLASSES))) & set(P.pairs)
        assert survivors <= planted | accidental                               # an equal band has an equal signature

        # placement: lane groups, the 15 | 16 batch boundary, the first and the last rank, the two sides of the query split
        cand = P.of("C1", "C2", "C3", "C6", "C7")
        assert any(i // 64 == k // 64 for i, k in cand) and any(i // 64 != k // 64 for i, k in cand)
        assert P.pairs[(0, N - 1)] == "C1" and P.pairs[(63, 64)] == "C1" and P.pairs[(15, 16)] == "C6"
        for cls in ("C1", "C2", "C3", "C4", "C5", "C6", "C7"):
            sides = {(i % 3 == 0) != (k % 3 == 0) for i, k in P.of(cls)}
            assert sides == {True, False}, cls
        if use_good is not None:
            assert all(use_good[p] for p in P.of("C2", "C3"))
