"""The dense-matrix hierarchy on the GPU (selhip_linkage, selhip_ctx_linkage; include/selection_hip.h section 2k).
Every output is compared bit for bit with tests/linkage_model.py, the sequential model in numpy, run on the same matrix; outputs go
into guarded buffers; every case runs twice and the two runs must be byte-equal.  Section 1b runs the slot kernels (lk_init_kernel,
lk_all_kernel, lk_book_kernel) under the process-wide grid hook "vertex_blocks", 1c the update kernel's stride over the pairs of a round
(n = 8 200) and 3b the distance transform's second trip (1 500 genomes): DESIGN.md section 32."""
import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import linkage_model as LM
from test_exhaustive_gpu import ranked
from test_matrix_gpu import synth

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import FP_FMA, PAIR_DTYPE, SelhipError, Selector

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
GUARD = 64                     # 16-byte records / int32 words of sentinel on both sides of every output array
SENTINEL = -77
METHODS = ("single", "complete", "average", "weighted")
SCAN_COLS = 512                # kLkScanCols of csrc/kernel_linkage.cuh: the columns one sweep of a row-scan workgroup covers
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2 * SCAN_COLS + 7]
RESCAN_SEEDS = (4, 36, 48)     # three-level matrices under single linkage whose model takes the rescan branch (asserted below)
VERTEX_BLOCKS = (1, 3)         # the slot kernels' grid under the hook: strides of 256 and of 768 slots
PAIR_CAPS = {"average": 200.0, "complete": 300.0, "single": 110.0, "weighted": 200.0}      # max_height for the "pairs" matrices: a few rounds and one rescan
UPDATE_ROWS = 4096             # the rows of lk_update_kernel's grid at most (host_linkage.hpp): a round of more pairs strides over them
DISTANCE_CELLS = 8192 * 256    # the cells one trip of lk_distance_kernel's grid covers at most


@pytest.fixture
def vertex_hook():
    """sets the process-wide grid of the kernels that take a lane per slot (0 = automatic) and puts the default back"""
    with Selector(0) as sel:
        def set_hook(vertex_blocks):
            sel.set_param("vertex_blocks", vertex_blocks)
            assert sel.get_param("vertex_blocks") == vertex_blocks
        yield set_hook
        set_hook(0)
        sel.set_param("cluster_blocks", 0)


def three_levels(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(8, 48))
    return rng.choice([0.25, 0.5, 0.75], size=(n, n))


def pairs_matrix(n, rng):
    """points on a line in n / 2 close pairs far apart: the first round pairs them all"""
    gaps = np.repeat(np.cumsum(100.0 + 50.0 * rng.random(n // 2 + 1)), 2)[:n]
    p = gaps + np.tile([0.0, 1.0], n // 2 + 1)[:n] * (0.5 + 0.4 * rng.random(n))
    return np.abs(p[:, None] - p[None, :])


def matrices(n):
    """{value set: n x n float64}; only the strict upper triangle counts"""
    rng = np.random.default_rng(1000 + n)
    sets = {"distinct": (rng.permutation(n * n).reshape(n, n) + rng.random((n, n)) / 2) / float(max(n * n, 1)),
            "levels": rng.choice([0.25, 0.5, 0.75], size=(n, n)),
            "specials": rng.choice([np.inf, -0.0, 0.0, 5e-324, -1.5, -0.25, 0.25, 1.0, 3.0], size=(n, n))}
    sets["pairs"] = pairs_matrix(n, rng)
    if n <= 257:                                                   # (the model rescans every row in each of their n - 1 rounds)
        sets["equal"] = np.full((n, n), 0.5)
        c = np.cumsum(1.5 ** np.arange(n))
        sets["chain"] = np.abs(c[:, None] - c[None, :])
    return sets


def linkage_raw(dist, method, max_height=np.inf, ld_extra=0, offset=0):
    """selhip_linkage on a copy of `dist` laid out with ld = n + ld_extra at `offset` doubles behind a 16-byte boundary, into guarded
    buffers: (merges PAIR_DTYPE [F], sizes [F], F, rounds)"""
    lib = pkg.hip_lib()
    n = dist.shape[0]
    ld = n + ld_extra
    cap = max(n - 1, 0)
    buf = torch.full((n * ld + 2 + offset,), float("nan"), dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[offset:offset + n * ld].view(n, ld) if n else buf[:0].view(0, max(ld, 1))
    if n:
        view[:, :n] = torch.from_numpy(np.ascontiguousarray(dist)).cuda()
    mbuf = torch.full(((cap + 2 * GUARD) * 4,), SENTINEL, dtype=torch.int32, device="cuda")
    sbuf = torch.full((cap + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    f, rounds = C.c_int64(-5), C.c_int64(-5)
    rc = lib.selhip_linkage(buf.data_ptr() + 8 * offset if n else None, n, ld, LM.METHODS[method], float(max_height), mbuf.data_ptr() + 16 * GUARD,
                            sbuf.data_ptr() + 4 * GUARD, C.byref(f), C.byref(rounds), None)
    msg = lib.selhip_last_error(None).decode()
    m, s = mbuf.cpu().numpy(), sbuf.cpu().numpy()
    if rc != 0:
        assert np.all(m == SENTINEL) and np.all(s == SENTINEL) and (f.value, rounds.value) == (-5, -5)      # nothing is written
        raise SelhipError(rc, msg)
    assert 0 <= f.value <= cap
    assert np.all(m[:4 * GUARD] == SENTINEL) and np.all(m[4 * (GUARD + f.value):] == SENTINEL)               # entries from F on are not written
    assert np.all(s[:GUARD] == SENTINEL) and np.all(s[GUARD + f.value:] == SENTINEL)
    return m[4 * GUARD:4 * (GUARD + f.value)].copy().view(PAIR_DTYPE), s[GUARD:GUARD + f.value].copy(), f.value, rounds.value


def same(got, want, what):
    merges, sizes, f, rounds = got
    assert f == want["n_merges"] and rounds == want["rounds"], (what, f, want["n_merges"], rounds, want["rounds"])
    assert merges.tobytes() == want["merges"].tobytes(), (what, np.flatnonzero(merges != want["merges"])[:3])
    assert np.array_equal(sizes, want["sizes"]), what


_WANT = {}


def model(n, vname, method, dist):
    """the model's answer for matrices(n)[vname], computed once for the tests that share it"""
    if (n, vname, method) not in _WANT:
        _WANT[n, vname, method] = LM.linkage_model(dist, method)
    return _WANT[n, vname, method]


# ---- 1. selhip_linkage: every size, layout, method and value set against the model, twice -----------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_linkage_against_the_model(n):
    for vname, dist in matrices(n).items():
        for method in METHODS:
            if n >= 511 and method == "single" and vname in ("levels", "specials"):
                continue                                           # (n - 1 rounds of full rescans: seconds of model time; n <= 257 covers them)
            want = model(n, vname, method, dist)
            assert want["n_merges"] == max(n - 1, 0)
            if vname == "equal" and n > 1:
                assert want["rounds"] == n and want["pairs_per_round"] == [1] * (n - 1) + [0]
            if vname == "pairs":
                assert want["pairs_per_round"][:1] == [n // 2] if n > 1 else want["rounds"] == 1
            first = linkage_raw(dist, method)
            again = linkage_raw(dist, method)
            assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(first, again)), (n, vname, method)
            same(first, want, (n, vname, method))
            for ld_extra, offset in ((3, 0), (0, 1), (3, 1)):      # the 8-byte path: an odd ld, a base 8 bytes off a 16-byte boundary
                same(linkage_raw(dist, method, ld_extra=ld_extra, offset=offset), want, (n, vname, method, ld_extra, offset))


@pytest.mark.parametrize("seed", RESCAN_SEEDS)
def test_rescan_rounds(seed):
    dist = three_levels(seed)
    want = LM.linkage_model(dist, "single")
    assert want["rescans"] > 0
    for ld_extra, offset in ((0, 0), (3, 1)):
        same(linkage_raw(dist, "single", ld_extra=ld_extra, offset=offset), want, seed)
    for method in METHODS[1:]:
        same(linkage_raw(dist, method), LM.linkage_model(dist, method), (seed, method))


# ---- 1b. the slot kernels in 1 and 3 blocks: every trip of lk_init, lk_all and lk_book ends in a ballot and a lane-ordered scatter ----------
@pytest.mark.parametrize("n", [257, 513, 2 * SCAN_COLS + 7])
def test_slot_kernels_under_the_vertex_hook(vertex_hook, n):
    """257, 513 and 1 031 slots in blocks of 256: under one block 2, 3 and 5 trips, the last of 1, 1 and 7 lanes; under three blocks
    the last trip of 1 031 holds 263.  The capped "pairs" hierarchy ends in a rescan round: lk_all_kernel then lists the active slots
    with inactive ones in every trip"""
    sets = matrices(n)
    for vname in ("distinct", "levels", "pairs"):
        for method in METHODS:
            if n >= 511 and method == "single" and vname == "levels":
                continue                                           # (as above)
            want = model(n, vname, method, sets[vname])
            for blocks in VERTEX_BLOCKS:
                vertex_hook(blocks)
                first = linkage_raw(sets[vname], method)
                again = linkage_raw(sets[vname], method)
                assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(first, again)), (n, vname, method, blocks)
                same(first, want, (n, vname, method, blocks))
            same(linkage_raw(sets[vname], method, ld_extra=3, offset=1), want, (n, vname, method, blocks, "8-byte"))
    for method, cap in PAIR_CAPS.items():
        want = LM.linkage_model(sets["pairs"], method, cap)
        assert want["rescans"] == 1 and 0 < want["n_merges"] < n - 1 and want["pairs_per_round"][0] == n // 2
        for blocks in VERTEX_BLOCKS:
            vertex_hook(blocks)
            same(linkage_raw(sets["pairs"], method, cap), want, (n, "pairs, capped", method, blocks))


def test_rescan_rounds_under_the_vertex_hook(vertex_hook):
    """(these matrices have fewer than 48 slots -- one trip of one block; the rescan rounds over several trips are the capped ones above)"""
    dist = three_levels(RESCAN_SEEDS[0])
    want = LM.linkage_model(dist, "single")
    assert want["rescans"] > 0
    for blocks in VERTEX_BLOCKS:
        vertex_hook(blocks)
        same(linkage_raw(dist, "single"), want, (RESCAN_SEEDS[0], blocks))


# ---- 1c. more pairs in a round than lk_update_kernel's grid has rows: the stride p += gridDim.y ------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
def test_update_kernel_pair_stride(method):
    """n = 8 200 points in 4 100 close pairs: round 1 pairs them all, so the update of the distances serves the pairs 4 096 .. 4 099 -- the
    slots 8 192 .. 8 199 -- in a second trip over the grid's rows.  The records of round 1 do not depend on the update; the later merges
    do, and the model has some among the slots from 8 192 on.  Capped (PAIR_CAPS): the whole hierarchy takes the model minutes"""
    n = 2 * UPDATE_ROWS + 8
    dist = pairs_matrix(n, np.random.default_rng(1000 + n))
    want = LM.linkage_model(dist, method, PAIR_CAPS[method])
    assert want["pairs_per_round"][0] == n // 2 == 4100 > UPDATE_ROWS and want["rescans"] == 1
    late = want["merges"][n // 2:]
    served_late = [(int(a), int(b)) for a, b in zip(late["i"], late["k"]) if max(a, b) >= 2 * UPDATE_ROWS]
    assert len(served_late) >= 1 and (method == "single" or len(served_late) == 3), served_late
    print(f"{method}: rounds {want['rounds']}, pairs per round {want['pairs_per_round'][:4]}, merges {want['n_merges']}, late merges of slots >= 8192: {served_late}")
    for ld_extra, offset in ((0, 0), (3, 1)):                      # the 16-byte path and one 8-byte layout
        got = linkage_raw(dist, method, PAIR_CAPS[method], ld_extra=ld_extra, offset=offset)
        torch.cuda.empty_cache()                                   # (538 MB of matrix: gone before the next one)
        same(got, want, (method, ld_extra, offset))


def test_empty_and_wrapper():
    assert linkage_raw(np.zeros((0, 0)), "average")[2:] == (0, 0)
    assert linkage_raw(np.zeros((1, 1)), "average")[2:] == (0, 1)
    dist = matrices(65)["distinct"]
    want = LM.linkage_model(dist, "average")
    res = pkg.linkage(dist, "average")
    assert res["merges"].dtype == PAIR_DTYPE and res["merges"].tobytes() == want["merges"].tobytes() and np.array_equal(res["sizes"], want["sizes"])
    assert res["n_merges"] == 64 and res["rounds"] == want["rounds"]
    t = torch.from_numpy(dist).cuda()
    keep = t.clone()
    on_dev = pkg.linkage(t, pkg.LINKAGE_AVERAGE, to_host=False)
    assert torch.equal(t, keep)                                    # cloned: the caller's tensor is as it was
    assert on_dev["merges"].is_cuda and on_dev["merges"].shape == (64, 16) and on_dev["merges"].cpu().numpy().tobytes() == want["merges"].tobytes()
    assert pkg.linkage(t, "average", overwrite=True)["merges"].tobytes() == want["merges"].tobytes()
    with pytest.raises(ValueError):
        pkg.linkage(dist, "ward")
    with pytest.raises(ValueError):
        pkg.linkage(dist, "average", max_height=float("nan"))


# ---- 2. the input contract --------------------------------------------------------------------------------------------------------------
def test_lower_triangle_and_diagonal_are_ignored():
    n = 257
    dist = matrices(n)["distinct"]
    want = LM.linkage_model(dist, "average")
    junk = dist.copy()
    junk[np.tril_indices(n)] = np.nan
    assert LM.linkage_model(junk, "average")["merges"].tobytes() == want["merges"].tobytes()
    for ld_extra, offset in ((0, 0), (3, 1)):
        same(linkage_raw(junk, "average", ld_extra=ld_extra, offset=offset), want, (ld_extra, offset))


@pytest.mark.parametrize("bad", [np.nan, -np.inf])
def test_bad_cells_are_refused(bad):
    n = 300
    dist = matrices(n)["distinct"]
    dist[[17, 5, 200], [230, 6, 299]] = bad                        # three cells of the upper triangle
    dist[40, 3] = np.nan                                           # (the lower one is not read)
    with pytest.raises(LM.BadCells) as model:
        LM.linkage_model(dist, "complete")
    assert model.value.count == 3 and model.value.cell == (5, 6)
    lib = pkg.hip_lib()
    for ld_extra, offset in ((0, 0), (3, 1)):
        with pytest.raises(SelhipError, match=r"3 cells .* cell \(5, 6\) is one") as err:
            linkage_raw(dist, "complete", ld_extra=ld_extra, offset=offset)
        assert err.value.code == -1
    dist[[17, 5, 200], [230, 6, 299]] = np.inf                     # +inf is data
    same(linkage_raw(dist, "complete"), LM.linkage_model(dist, "complete"), "+inf")
    # arguments
    buf = torch.zeros(4 * 4 + 2, dtype=torch.float64, device="cuda")
    out = torch.zeros(64, dtype=torch.uint8, device="cuda")
    for args, text in (((buf.data_ptr(), 4, 4, 7, 1.0, None, None), "bad method 7"), ((buf.data_ptr(), 4, 4, -1, 1.0, None, None), "bad method -1"),
                       ((buf.data_ptr(), 4, 4, 2, float("nan"), None, None), "max_height is NaN"), ((buf.data_ptr(), 4, 3, 2, 1.0, None, None), "ld >= n"),
                       ((buf.data_ptr(), -1, 4, 2, 1.0, None, None), "0 <= n"), ((None, 4, 4, 2, 1.0, None, None), "non-null"),
                       ((buf.data_ptr() + 4, 4, 4, 2, 1.0, None, None), "8-byte aligned"), ((buf.data_ptr(), 4, 4, 2, 1.0, out.data_ptr() + 8, None), "16-byte aligned")):
        assert lib.selhip_linkage(*args, None, None, None) == -1 and text in lib.selhip_last_error(None).decode(), text
    assert lib.selhip_linkage(buf.data_ptr(), 4, 4, 2, float("inf"), None, None, None, None, None) == 0          # every output may be NULL


@pytest.mark.parametrize("method", METHODS)
def test_max_height(method):
    n = 300
    dist = matrices(n)["distinct"]
    full = LM.linkage_model(dist, method)
    h = np.sort(full["merges"]["jaccard"])
    below = float(np.nextafter(dist[np.triu_indices(n, 1)].min(), -np.inf))
    between = float((h[n // 2] + h[n // 2 + 1]) / 2)
    assert h[n // 2] < between < h[n // 2 + 1]
    whole = linkage_raw(dist, method)
    same(whole, full, method)
    for cap, f in ((below, 0), (between, n // 2 + 1), (float(h[-1]), n - 1), (np.inf, n - 1)):
        want = LM.linkage_model(dist, method, cap)
        assert want["n_merges"] == f, (method, cap)
        got = linkage_raw(dist, method, cap)
        same(got, want, (method, cap))
        # the cut of the whole hierarchy at that height is the partition the capped call leaves
        labels = pkg.linkage_cut(whole[0], n, cap)
        assert labels.dtype == np.int32 and np.array_equal(labels, LM.labels_of(got[0], n)), (method, cap)
    assert pkg.linkage(dist, method, max_height=between)["n_merges"] == n // 2 + 1


def test_single_linkage_equals_the_spanning_forest():
    """two independent device implementations: the sorted heights are, bit for bit, the negated values of the maximum spanning forest
    over all pairs with the values -d"""
    for n, vname in ((257, "distinct"), (300, "levels"), (129, "specials")):
        dist = matrices(n)[vname]
        a, b = np.triu_indices(n, 1)
        d = dist[a, b] + 0.0                                       # (-0.0 and +0.0 are one value to the forest, written +0.0)
        forest = pkg.spanning_forest(np.stack([a, b], axis=1).astype(np.int32), n, -d)
        got = linkage_raw(dist, "single")
        assert forest["n_edges"] == got[2] == n - 1
        assert np.array_equal(np.sort(got[0]["jaccard"] + 0.0).view(np.uint64), np.sort(-forest["edges"]["jaccard"] + 0.0).view(np.uint64)), (n, vname)


# ---- 3. the context entry ---------------------------------------------------------------------------------------------------------------
def raw_ctx_linkage(sel, measure, method, max_height=np.inf, null=()):
    n = sel.n
    cap = max(n - 1, 0)
    mbuf = torch.full(((cap + 2 * GUARD) * 4,), SENTINEL, dtype=torch.int32, device="cuda")
    sbuf = torch.full((cap + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    out = pkg._lib.Linkage(None if "merges" in null else mbuf.data_ptr() + 16 * GUARD, None if "sizes" in null else sbuf.data_ptr() + 4 * GUARD)
    cnt = C.c_int64(-5)
    pkg._lib.check(sel._lib.selhip_ctx_linkage(sel._ctx, pkg.measure_code(measure), LM.METHODS[method], float(max_height), C.byref(out), C.byref(cnt)), sel._ctx)
    f = cnt.value
    m, s = mbuf.cpu().numpy(), sbuf.cpu().numpy()
    fm, fs = (0 if "merges" in null else f), (0 if "sizes" in null else f)
    assert np.all(m[:4 * GUARD] == SENTINEL) and np.all(m[4 * (GUARD + fm):] == SENTINEL)
    assert np.all(s[:GUARD] == SENTINEL) and np.all(s[GUARD + fs:] == SENTINEL)
    assert sel.get_param("linkage_merges_last") == f
    return m[4 * GUARD:4 * (GUARD + fm)].copy().view(PAIR_DTYPE), s[GUARD:GUARD + fs].copy(), f, sel.get_param("linkage_rounds_last")


def distance_of(sel, measure):
    d = 1.0 - sel.matrix(measure).cpu().numpy()
    d[np.isnan(d)] = 1.0
    return d


def check_context(sel, measures):
    n = sel.n
    for measure in measures:
        dist = distance_of(sel, measure)
        for method in METHODS:
            want = LM.linkage_model(dist, method)
            got = raw_ctx_linkage(sel, measure, method)
            same(got, want, (measure, method))
            assert sel.get_param("linkage_rowscans_last") == want["rowscans"] and sel.get_param("linkage_rescans_last") == want["rescans"]
        h = np.sort(want["merges"]["jaccard"])
        cap = float(h[len(h) // 2])
        same(raw_ctx_linkage(sel, measure, "weighted", cap), LM.linkage_model(dist, "weighted", cap), (measure, "capped"))
        res = sel.linkage(measure, "weighted")
        assert res["merges"].tobytes() == want["merges"].tobytes() and np.array_equal(res["sizes"], want["sizes"]) and res["rounds"] == want["rounds"]
        assert res["n_merges"] == n - 1
    only_m, only_s, neither = (raw_ctx_linkage(sel, measures[0], "average", null=x) for x in (("sizes",), ("merges",), ("merges", "sizes")))
    assert only_m[2] == only_s[2] == neither[2] == n - 1 and len(only_m[1]) == 0 and len(only_s[0]) == 0


def test_context_synthetic_set(oracle):
    """~300 synthetic genomes, three of them with empty HLL sketches (J is NaN between them: distance 1.0)"""
    hll, aux = synth("cfg2-spread", 300)
    hll = hll.copy()
    hll[:3] = 0
    hll, aux, cards = ranked(oracle, hll, aux, FP_FMA)
    assert np.all(cards[:3] == 0)
    with Selector(0) as sel:
        assert [sel.get_param(k) for k in ("linkage_rounds_last", "linkage_merges_last", "linkage_rowscans_last")] == [-1, -1, -1]
        sel.upload(hll, aux, cards)
        assert np.isnan(sel.matrix("jaccard").cpu().numpy()[0, 1])
        check_context(sel, ("jaccard", "max_containment", "smh_jaccard"))


# ---- 3b. more cells than one trip of lk_distance_kernel's grid covers ---------------------------------------------------------------------
def test_context_distance_second_trip():
    """1 500 genomes, 2 250 000 cells: the distance transform comes round for the cells from 2 097 152 on -- row 1 398, column 304.  Five
    genomes have empty HLL sketches and J is NaN between them: three in the first rows, two past row 1 398, so NaN cells lie in both
    trips.  The rows stay in generation order and the device computes the cardinalities: a matrix call asks for no ranking, and ranked
    rows would have every empty sketch in front"""
    n = 1500
    empty = (0, 1, 2, 1450, 1499)
    hll, aux = synth("cfg2-spread", n)
    hll = hll.copy()
    hll[list(empty)] = 0
    assert n * n > DISTANCE_CELLS
    with Selector(0) as sel:
        sel.upload(hll, aux, None)
        assert np.flatnonzero(sel.cards() == 0).tolist() == list(empty)
        nan_at = np.flatnonzero(np.isnan(sel.matrix("jaccard").cpu().numpy().reshape(-1)))
        assert nan_at.min() < DISTANCE_CELLS <= 1450 * n + 1499 and 1450 * n + 1499 in nan_at and 1499 * n + 1450 in nan_at, (nan_at.min(), nan_at.max())
        dist = distance_of(sel, "jaccard")
        want = LM.linkage_model(dist, "average")
        same(raw_ctx_linkage(sel, "jaccard", "average"), want, "average")
        assert sel.get_param("linkage_rowscans_last") == want["rowscans"] and sel.get_param("linkage_rescans_last") == want["rescans"]
        h = np.sort(want["merges"]["jaccard"])
        cap = float(h[len(h) // 2])
        capped = LM.linkage_model(dist, "complete", cap)
        assert 0 < capped["n_merges"] < n - 1
        same(raw_ctx_linkage(sel, "jaccard", "complete", cap), capped, "complete, capped")


def test_context_influenza(monkeypatch):
    monkeypatch.chdir(GOLDEN)
    ds = pkg.load_dataset("influenza_filelist.txt", 64)
    with Selector(0) as sel:
        sel.upload(ds.hll, ds.aux, ds.cards)
        check_context(sel, ("jaccard", "max_containment", "smh_jaccard"))
        # the distance= route: the Mash distance in torch, the model on the same tensor copied to the host
        mash = lambda j: -torch.log(2 * j / (1 + j)) / 21
        dist = mash(sel.matrix("jaccard")).cpu().numpy()
        assert not np.isnan(dist[np.triu_indices(sel.n, 1)]).any()
        for method in ("average", "complete"):
            want = LM.linkage_model(dist, method)
            res = sel.linkage("jaccard", method, distance=mash)
            assert res["merges"].tobytes() == want["merges"].tobytes() and np.array_equal(res["sizes"], want["sizes"]) and res["rounds"] == want["rounds"]


def test_context_states_and_refusals(oracle):
    n = 150
    hll, aux, cards = ranked(oracle, *synth("cfg2-spread", n))
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        sel.set_criterion(pkg.CRIT_NONE)
        rec = sel.run(0.05, pkg.MODE_SMH, 1, 1)
        assert len(rec) > 0
        snap = lambda: (sel.fetch().tobytes(), sel.stats(), sel.last_attempts(), sel.result_count(), sel.get_param("forest_edges_last"),
                        sel.get_param("clusters_last"), sel.get_param("allpairs_topk"))
        before = snap()
        sel.timing(1)
        sel.matrix("jaccard")
        sel.matrix("smh_jaccard")
        names = ("prep", "stage1", "total", "topk", "matrix", "matrix_smh", "cluster", "greedy", "merge", "forest", "hist", "select")
        ms, launches = [sel.kernel_ms(k) for k in names], [sel.kernel_launches(k) for k in names]
        assert sel.kernel_ms("linkage") < 0
        raw_ctx_linkage(sel, "jaccard", "average")
        raw_ctx_linkage(sel, "smh_jaccard", "single")
        assert sel.kernel_ms("linkage") > 0
        assert [sel.kernel_ms(k) for k in names] == ms and [sel.kernel_launches(k) for k in names] == launches
        sel.timing(0)
        assert snap() == before                                     # the result list, the statistics and the other calls' reports
        last = [sel.get_param(k) for k in ("linkage_rounds_last", "linkage_merges_last", "linkage_rowscans_last")]
        for measure in ("union", "intersection", "containment", "smh_matches"):
            with pytest.raises(SelhipError, match="no symmetric similarity") as err:
                raw_ctx_linkage(sel, measure, "average")
            assert err.value.code == -1
        lib = sel._lib
        out = pkg._lib.Linkage(None, None)
        assert lib.selhip_ctx_linkage(sel._ctx, 0, 9, 1.0, C.byref(out), None) == -1 and "bad method 9" in lib.selhip_last_error(sel._ctx).decode()
        assert lib.selhip_ctx_linkage(sel._ctx, 0, 2, float("nan"), C.byref(out), None) == -1 and "NaN" in lib.selhip_last_error(sel._ctx).decode()
        assert lib.selhip_ctx_linkage(sel._ctx, 0, 2, 1.0, None, None) == -1 and "null selhip_linkage_t" in lib.selhip_last_error(sel._ctx).decode()
        buf = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
        out = pkg._lib.Linkage(buf.data_ptr() + 8, None)
        assert lib.selhip_ctx_linkage(sel._ctx, 0, 2, 1.0, C.byref(out), None) == -1 and "16-byte aligned" in lib.selhip_last_error(sel._ctx).decode()
        sel.run_async(0.05, pkg.MODE_SMH, 1, 1)
        with pytest.raises(SelhipError, match="pending") as err:
            raw_ctx_linkage(sel, "jaccard", "average")
        assert err.value.code == -5
        sel.finish()
        assert [sel.get_param(k) for k in ("linkage_rounds_last", "linkage_merges_last", "linkage_rowscans_last")] == last
        # an empty set and a single genome
        sel.upload(hll[:1], aux[:1], cards[:1])
        assert raw_ctx_linkage(sel, "jaccard", "average")[2:] == (0, 1)
        sel.upload(hll[:0], aux[:0], cards[:0])
        assert raw_ctx_linkage(sel, "smh_jaccard", "average")[2:] == (0, 0)
    # the HLL measures need p_hll = 14 and the bit planes; smh_jaccard reads the bucket rows alone
    with Selector(0) as sel:
        sel.upload(np.zeros((n, 1 << 12), dtype=np.uint8), aux, None, p_hll=12)
        with pytest.raises(SelhipError, match="p_hll = 14") as err:
            raw_ctx_linkage(sel, "jaccard", "average")
        assert err.value.code == -1
        same(raw_ctx_linkage(sel, "smh_jaccard", "average"), LM.linkage_model(distance_of(sel, "smh_jaccard"), "average"), "p_hll 12")


# ---- 4. the Python helpers on a device result ----------------------------------------------------------------------------------------------
def test_helpers_on_a_device_result():
    from scipy.cluster.hierarchy import fcluster, is_valid_linkage
    n = 300
    dist = matrices(n)["distinct"]
    for method in METHODS:
        res = pkg.linkage(dist, method)
        Z = pkg.linkage_matrix(res["merges"], res["sizes"], n)
        assert is_valid_linkage(Z) and Z.shape == (n - 1, 4)
        h = np.sort(res["merges"]["jaccard"])
        for t in (float(h[10]), float((h[150] + h[151]) / 2), float(h[-1])):
            mine = pkg.linkage_cut(res["merges"], n, t)
            theirs = fcluster(Z, t, criterion="distance")
            assert len(set(zip(mine.tolist(), theirs.tolist()))) == len(set(mine.tolist())) == len(set(theirs.tolist())), (method, t)


# ---- 5. the command line, on the influenza fixtures ---------------------------------------------------------------------------------------
def selection(args, status=0):
    out = subprocess.run([str(BIN / "selection")] + args, cwd=GOLDEN, capture_output=True, text=True)
    assert out.returncode == status, (out.returncode, out.stderr)
    return out


def parse_newick(text):
    """(the member sets of the inner nodes as frozensets of leaf names, {leaf or inner-node member set: branch length}) of a Newick
    line with unquoted names"""
    assert text.endswith(";\n")
    sets, lengths, stack, pos = [], {}, [], 0
    body = text[:-2]
    last = None
    while pos < len(body):
        ch = body[pos]
        if ch == "(":
            stack.append([])
            pos += 1
        elif ch == ",":
            pos += 1
        elif ch == ")":
            last = frozenset().union(*stack.pop())
            sets.append(last)
            if stack:
                stack[-1].append(last)
            pos += 1
        elif ch == ":":
            end = pos + 1
            while end < len(body) and body[end] not in ",()":
                end += 1
            lengths[last] = float(body[pos + 1:end])
            pos = end
        else:
            end = pos
            while body[end] not in ":,()":
                end += 1
            last = frozenset([body[pos:end]])
            stack[-1].append(last)
            pos = end
    return sets, lengths


@pytest.mark.parametrize("args,kw", [([], dict(measure="jaccard", method="average")), (["-X", "complete"], dict(measure="jaccard", method="complete")),
                                     (["-X", "single", "-E", "smh", "-a", "512"], dict(measure="smh_jaccard", method="single", aux_bytes=512)),
                                     (["-X", "weighted", "-S", "max_containment"], dict(measure="max_containment", method="weighted"))],
                         ids=["average", "complete", "single-smh", "weighted-max_containment"])
def test_cli(monkeypatch, tmp_path, args, kw):
    monkeypatch.chdir(GOLDEN)
    want = pkg.linkage_from_filelist("influenza_filelist.txt", **kw)
    names, n = want["names"], len(want["names"])
    assert want["n_merges"] == n - 1 and want["table"].count("\n") == n - 1
    tree, table, matrix = tmp_path / "tree.nwk", tmp_path / "merges.tsv", tmp_path / "matrix.tsv"
    out = selection(["-l", "influenza_filelist.txt", "-N", str(tree), "-J", str(table)] + args)
    assert out.stdout == ""
    assert table.read_text() == want["table"]
    assert tree.read_text() == want["newick"]
    sets, lengths = parse_newick(tree.read_text())
    members = [frozenset(names[g] for g in s) for s in LM.members_of(want["merges"], n)]
    assert sorted(sets, key=sorted) == sorted(members, key=sorted)
    # ultrametric: a node's branch is (parent's height - own height) / 2
    height = {frozenset([nm]): 0.0 for nm in names}
    height.update({s: float(e["jaccard"]) for s, e in zip(members, want["merges"])})
    parent = {}
    for s in sorted(members, key=len):
        for child in list(height):
            if child < s and child not in parent:
                parent[child] = s
    for node, length in lengths.items():
        assert length == max((height[parent[node]] - height[node]) / 2.0, 0.0), node
    # -J alone, and both beside -M
    table.unlink()
    selection(["-l", "influenza_filelist.txt", "-J", str(table)] + args)
    assert table.read_text() == want["table"]
    tree.unlink()
    selection(["-l", "influenza_filelist.txt", "-N", str(tree), "-M", str(matrix)] + args)
    assert tree.read_text() == want["newick"] and len(matrix.read_text().splitlines()) >= n
