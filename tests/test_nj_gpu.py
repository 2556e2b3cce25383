"""The neighbour-joining tree on the device (include/selection_hip.h section 2l) against tests/nj_model.py, bit for bit:
selhip_neighbor_joining into guarded buffers, every case twice and byte-equal, over both scan paths (16-byte and 8-byte loads), the
slot kernels under the "vertex_blocks" hook, the refusals, the context entry and the command line.

Beyond the well-behaved matrices (the sets are tests/nj_model.py's, their premises tests/test_nj_host.py's):
  test_later_trips_decide, test_later_trips_under_the_vertex_hook   n = 1 031 and 2 055: the winning row in the last trip of the pick's
                      walk, three cells per lane of the row sums, ties across trips, waves and sweep steps; the model's first 16 records
  test_signed_zero_literals, test_signed_zeros   -0.0 cells survive the mirror: two truths worked out by hand, and three kinds of set
  test_sums_that_overflow   finite cells near 1e308: NaN q counts as +inf; the one comparison that takes a NaN for a NaN
  test_context_small_sets_and_null_arguments   contexts of 0, 1, 2, 3 and 5 genomes, d_joins NULL, n_joins_out NULL, a pending pass"""
import ctypes as C
import functools
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import nj_model as NM
from test_exhaustive_gpu import ranked
from test_matrix_gpu import synth

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import FP_FMA, NJ_DTYPE, SelhipError, Selector
from cuda_selection_criteria_amd._lib import check as lib_check

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
GUARD = 64                     # records of sentinel on both sides of the output array
SENTINEL = -77
SCAN_COLS = 512                # kNjScanCols of csrc/kernel_nj.cuh; a scan workgroup takes kNjRows = 4 list rows: n = 4 and 5 lie on either side
SIZES = [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2 * SCAN_COLS + 7]
LAYOUTS = [(0, 0), (3, 0), (0, 1), (3, 1)]      # (ld - n, doubles behind a 16-byte boundary): 16-byte loads need an even ld and offset 0


@functools.lru_cache(maxsize=None)
def matrices(n):
    """{value set: (n x n float64 of which the strict upper triangle counts, the model's records)}, computed once"""
    return {k: (v, NM.neighbor_joining(v)) for k, v in NM.value_sets(n).items()}


def nj_raw(dist, ld_extra=0, offset=0):
    """selhip_neighbor_joining on a copy of `dist` laid out with ld = n + ld_extra at `offset` doubles behind a 16-byte boundary,
    into a guarded buffer: the records NJ_DTYPE [n - 1]"""
    lib = pkg.hip_lib()
    n = dist.shape[0]
    ld = n + ld_extra
    cap = max(n - 1, 0)
    buf = torch.full((n * ld + 2 + offset,), float("nan"), dtype=torch.float64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    if n:
        buf[offset:offset + n * ld].view(n, ld)[:, :n] = torch.from_numpy(np.ascontiguousarray(dist)).cuda()
    jbuf = torch.full(((cap + 2 * GUARD) * 6,), SENTINEL, dtype=torch.int32, device="cuda")
    f = C.c_int64(-5)
    rc = lib.selhip_neighbor_joining(buf.data_ptr() + 8 * offset if n else None, n, ld, jbuf.data_ptr() + 24 * GUARD, C.byref(f), None)
    msg = lib.selhip_last_error(None).decode()
    j = jbuf.cpu().numpy()
    if rc != 0:
        assert np.all(j == SENTINEL) and f.value == -5                        # nothing is written
        raise SelhipError(rc, msg)
    assert f.value == cap
    assert np.all(j[:6 * GUARD] == SENTINEL) and np.all(j[6 * (GUARD + cap):] == SENTINEL)
    return j[6 * GUARD:6 * (GUARD + cap)].copy().view(NJ_DTYPE)


@pytest.mark.parametrize("n", SIZES)
def test_against_the_model(n):
    for vname, (dist, want) in matrices(n).items():
        for ld_extra, offset in LAYOUTS:
            got, again = nj_raw(dist, ld_extra, offset), nj_raw(dist, ld_extra, offset)
            assert got.tobytes() == want.tobytes(), (vname, ld_extra, offset, np.flatnonzero(got != want)[:3])
            assert again.tobytes() == got.tobytes(), (vname, ld_extra, offset)
        if vname == "dyadic":                                                 # the truth that does not depend on the model
            _, total, splits = NM.dyadic_tree(n, n)
            assert NM.join_splits(got, n) == splits and float(np.sum(got["len_a"]) + np.sum(got["len_b"])) == total
        if vname == "negative" and n >= 64:
            assert min(want["len_a"].min(), want["len_b"].min()) < 0
        if vname == "equal" and n >= 2:
            assert np.all(want["a"] == 0) and np.array_equal(want["b"], np.arange(1, n))


@pytest.mark.parametrize("blocks", (1, 3))
def test_slot_kernels_under_the_vertex_hook(blocks):
    """nj_init_kernel and nj_update_kernel walk their grid-stride loops: 513 slots over 1 and 3 workgroups of 256 lanes"""
    dist, want = matrices(513)["distinct"]
    with Selector(0) as sel:
        sel.set_param("vertex_blocks", blocks)
        try:
            assert nj_raw(dist).tobytes() == want.tobytes() and nj_raw(dist, 3, 1).tobytes() == want.tobytes()
        finally:
            sel.set_param("vertex_blocks", 0)


BOTH_SCANS = [(0, 0), (3, 1)]                    # nj_scan_kernel<true> and <false>
TRIP_SETS = ("forged", "equal", "levels", "twins")


@functools.lru_cache(maxsize=None)
def trip_case(n, vname):
    """(matrix, the first NM.PREFIX records of the model) of a set whose answer the later trips of the 1 024-lane loops decide"""
    dist = NM.forged(n) if vname == "forged" else NM.tie_sets(n)[vname]
    return dist, NM.neighbor_joining(dist, first=NM.PREFIX)


def twice_in_both_scans(dist, want, compare=None):
    """`dist` through both scan instantiations, each twice and byte-equal: the device's first len(want) records are the model's (by
    bytes, or by compare(got, want)), and whatever lies behind them is the same in all four runs.  Returns the records"""
    first = None
    for layout in BOTH_SCANS:
        got, again = nj_raw(dist, *layout), nj_raw(dist, *layout)
        head = got[:len(want)]
        if compare is None:
            assert head.tobytes() == want.tobytes(), (layout, np.flatnonzero(head != want)[:3], head[:2], want[:2])
        else:
            compare(head, want, layout)
        assert again.tobytes() == got.tobytes(), layout
        first = got if first is None else first
        assert got.tobytes() == first.tobytes(), "the two scan paths give different records"
    return first


def check_trip_case(n, vname):
    dist, want = trip_case(n, vname)
    got = twice_in_both_scans(dist, want)
    assert len(got) == n - 1 and np.all(got["a"] < got["b"])
    if vname == "equal":                                                      # the truth that does not depend on the model: a star
        assert np.all(got["a"] == 0) and np.array_equal(got["b"], np.arange(1, n))
        assert np.all(got["len_b"][:-1] == 0.25) and np.all(got["len_a"][1:-1] == 0.0) and got["len_a"][-1] == got["len_b"][-1] == 0.125
    if vname == "forged":
        assert (int(got["a"][0]), int(got["b"][0])) == NM.forged_pair(n)
    if vname == "twins":
        assert [(int(e["a"]), int(e["b"])) for e in got[:2]] == [NM.TWIN, NM.forged_pair(n)]


@pytest.mark.parametrize("vname", TRIP_SETS)
@pytest.mark.parametrize("n", NM.TRIP_SIZES)
def test_later_trips_decide(n, vname):
    """n = 1 024 + 7 and 2 * 1 024 + 7: nj_pick_kernel walks the rows' bests in two and three trips and the winning row lies in the
    last one ("forged": the pair (n - 4, n - 2), premise pinned by tests/test_nj_host.py); nj_rowsum_kernel adds two and three cells
    per lane, and the forged columns n - 4 and n - 2 carry most of every row's sum; ties are resolved across the trips of a lane,
    the waves and the scan workgroups' sweep steps ("equal": every q ties, "twins": the smallest q lies once in wave 1 and once in a
    later trip of wave 0, "levels").  The model's first 16 records; the rest between the runs and the layouts"""
    check_trip_case(n, vname)


@pytest.mark.parametrize("blocks", (1, 3))
def test_later_trips_under_the_vertex_hook(blocks):
    """... and with nj_init_kernel and nj_update_kernel in 5 and 2 trips of their own loops"""
    with Selector(0) as sel:
        sel.set_param("vertex_blocks", blocks)
        try:
            for vname in TRIP_SETS:
                check_trip_case(NM.TRIP_SIZES[0], vname)
        finally:
            sel.set_param("vertex_blocks", 0)


def f64_bits(*values):
    return np.array(values, dtype=np.float64).view(np.uint64).tolist()


def test_signed_zero_literals():
    """section 2l evaluated by hand (tests/test_nj_host.py holds the model to the same two): the mirror copies a -0.0 cell, so
    0.5 * -0.0 = -0.0 at n = 2, and five slots of -0.0 give (0, 1, -0.0 + 0.0 / 6 = +0.0, -0.0 - +0.0 = -0.0)"""
    for layout in BOTH_SCANS:
        two = nj_raw(np.array([[0.0, -0.0], [0.0, 0.0]]), *layout)
        assert (int(two["a"][0]), int(two["b"][0])) == (0, 1) and f64_bits(two["len_a"][0], two["len_b"][0]) == f64_bits(-0.0, -0.0), (layout, two)
        five = nj_raw(np.triu(np.full((5, 5), -0.0), 1), *layout)
        assert (int(five["a"][0]), int(five["b"][0])) == (0, 1) and f64_bits(five["len_a"][0], five["len_b"][0]) == f64_bits(0.0, -0.0), (layout, five)


@functools.lru_cache(maxsize=None)
def zero_cases(n):
    return {k: (v, NM.neighbor_joining(v)) for k, v in NM.zero_sets(n).items()}


@pytest.mark.parametrize("n", NM.ZERO_SIZES)
def test_signed_zeros(n):
    """-0.0 in every cell, in a random half of an all-zero matrix, and among the zeros of a four-level matrix: bytes and all"""
    for vname, (dist, want) in zero_cases(n).items():
        got = twice_in_both_scans(dist, want)
        assert len(got) == n - 1, vname


def same_but_for_the_nans(got, want, where):
    """THE OVERFLOW SETS ONLY.  a and b exactly; a length by its bit pattern where the model's is no NaN, and by being a NaN where it is:
    inf - inf gives a NaN whose sign and payload differ between x86 (the model: the default NaN with the sign set) and the GPU (its
    canonical quiet NaN), and section 2l says nothing about them.  No other case of this file may use this comparison"""
    assert np.array_equal(got["a"], want["a"]) and np.array_equal(got["b"], want["b"]), (where, np.flatnonzero((got["a"] != want["a"]) | (got["b"] != want["b"]))[:3])
    for field in ("len_a", "len_b"):
        g, w = got[field], want[field]
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), (where, field, np.flatnonzero(np.isnan(g) != nan)[:3])
        assert np.array_equal(g[~nan].view(np.uint64), w[~nan].view(np.uint64)), (where, field)


@functools.lru_cache(maxsize=None)
def overflow_cases(n):
    return {k: (v, NM.neighbor_joining(v)) for k, v in NM.overflow_sets(n).items()}


@pytest.mark.parametrize("n", NM.OVERFLOW_SIZES)
def test_sums_that_overflow(n):
    """finite cells near 1e308: the row sums are +inf, q is inf - inf = NaN and counts as +inf; where every q is +inf the first two
    active slots are joined.  The run-to-run and layout-to-layout comparisons stay by bytes: the device's NaNs are its own, every time"""
    for vname, (dist, want) in overflow_cases(n).items():
        got = twice_in_both_scans(dist, want, compare=lambda g, w, layout: same_but_for_the_nans(g, w, (n, vname, layout)))
        assert len(got) == n - 1 and np.all(got["a"] < got["b"]), vname
        if vname == "huge" and n >= 65:
            assert np.isnan(got["len_a"]).all() and np.isnan(got["len_b"]).all()
        if vname == "mixed":
            assert np.isinf(got["len_a"]).any() and np.isnan(got["len_a"]).any() and np.isfinite(got["len_a"]).any()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_bad_cells_are_refused(bad):
    dist = matrices(65)["distinct"][0].copy()
    dist[7, 3] = dist[9, 9] = bad                                              # below and on the diagonal: not input
    assert nj_raw(dist).tobytes() == matrices(65)["distinct"][1].tobytes()
    dist[3, 64] = dist[40, 41] = bad
    for layout in ((0, 0), (3, 1)):
        with pytest.raises(SelhipError, match=r"2 cells of the upper triangle are NaN, \+inf or -inf.*cell \(3, 64\) is one") as err:
            nj_raw(dist, *layout)
        assert err.value.code == -1
    with pytest.raises(SelhipError, match=r"cell \(3, 64\)"):
        pkg.neighbor_joining(dist)
    on_dev = torch.from_numpy(matrices(65)["negative"][0]).cuda()              # the wrapper clones a device tensor unless overwrite=True
    res = pkg.neighbor_joining(on_dev, to_host=False)
    assert res["joins"].cpu().numpy().view(NJ_DTYPE).reshape(-1).tobytes() == matrices(65)["negative"][1].tobytes()
    assert np.array_equal(on_dev.cpu().numpy(), matrices(65)["negative"][0])


def check_context(sel):
    timers = ("matrix", "matrix_smh", "linkage")
    sel.timing(1)
    sel.matrix("jaccard")
    sel.linkage("jaccard")
    before = [(sel.kernel_ms(k), sel.kernel_launches(k)) for k in timers]
    assert sel.kernel_ms("nj") < 0
    for measure in ("jaccard", "max_containment", "smh_jaccard"):
        got = sel.neighbor_joining(measure)
        assert got["n_joins"] == sel.n - 1 and got["joins"].dtype == NJ_DTYPE
        assert sel.kernel_ms("nj") > 0
        assert [(sel.kernel_ms(k), sel.kernel_launches(k)) for k in timers] == before
        sim = sel.matrix(measure).cpu().numpy()
        dist = 1.0 - sim
        dist[np.isnan(sim)] = 1.0
        before = [(sel.kernel_ms(k), sel.kernel_launches(k)) for k in timers]
        assert got["joins"].tobytes() == NM.neighbor_joining(dist).tobytes(), measure
    sel.timing(0)
    with pytest.raises(SelhipError, match="no symmetric similarity"):
        sel.neighbor_joining("union")


def test_context_influenza(monkeypatch):
    monkeypatch.chdir(GOLDEN)
    ds = pkg.load_dataset("influenza_filelist.txt", 64)
    with Selector(0) as sel:
        sel.upload(ds.hll, ds.aux, ds.cards)
        check_context(sel)
        mash = lambda j: -torch.log(2 * j / (1 + j)) / 21                      # the distance= route
        dist = mash(sel.matrix("jaccard")).cpu().numpy()
        assert np.isfinite(dist[np.triu_indices(sel.n, 1)]).all()
        assert sel.neighbor_joining("jaccard", distance=mash)["joins"].tobytes() == NM.neighbor_joining(dist).tobytes()
        with pytest.raises(SelhipError, match=r"\+inf"):                       # a J of 0 is a Mash distance of +inf
            sel.neighbor_joining("jaccard", distance=lambda j: mash(j * 0))


def test_context_synthetic_set(oracle):
    """130 synthetic genomes, three of them with empty HLL sketches (J is NaN between them: distance 1.0)"""
    hll, aux = synth("cfg2-spread", 130)
    hll = hll.copy()
    hll[:3] = 0
    with Selector(0) as sel:
        sel.upload(*ranked(oracle, hll, aux, FP_FMA))
        assert np.isnan(sel.matrix("jaccard").cpu().numpy()[0, 1])
        check_context(sel)


def ctx_nj_raw(sel, measure, joins=True, count=True):
    """selhip_ctx_neighbor_joining into a guarded buffer (joins=False: d_joins NULL; count=False: n_joins_out NULL):
    (the records, the count or -5 where none was asked for)"""
    cap = max(sel.n - 1, 0)
    jbuf = torch.full(((cap + 2 * GUARD) * 6,), SENTINEL, dtype=torch.int32, device="cuda")
    f = C.c_int64(-5)
    rc = sel._lib.selhip_ctx_neighbor_joining(sel._ctx, pkg.measure_code(measure), jbuf.data_ptr() + 24 * GUARD if joins else None, C.byref(f) if count else None)
    j = jbuf.cpu().numpy()
    if rc != 0 or not joins:
        assert np.all(j == SENTINEL)                                          # nothing is written
    lib_check(rc, sel._ctx)
    assert np.all(j[:6 * GUARD] == SENTINEL) and np.all(j[6 * (GUARD + cap):] == SENTINEL)
    return j[6 * GUARD:6 * (GUARD + cap)].copy().view(NJ_DTYPE), f.value


@pytest.mark.parametrize("n", (0, 1, 2, 3, 5))
def test_context_small_sets_and_null_arguments(oracle, n):
    """the first n genomes of test_context_synthetic_set's set (three empty sketches in front): no genome and one genome give no
    record and write nothing, two give the last join alone; d_joins NULL and n_joins_out NULL; a pending pass refuses"""
    hll, aux = synth("cfg2-spread", 130)
    hll = hll[:n].copy()
    hll[:3] = 0
    with Selector(0) as sel:
        sel.upload(*ranked(oracle, hll, aux[:n], FP_FMA))
        assert sel.n == n
        if n >= 1:
            check_context(sel)                                                # (n = 1: "nj" counts the call, the other timers stand)
        for measure in ("jaccard", "max_containment", "smh_jaccard"):
            want = NM.neighbor_joining(np.zeros((n, n)))
            if n >= 2:
                sim = sel.matrix(measure).cpu().numpy()
                dist = 1.0 - sim
                dist[np.isnan(sim)] = 1.0
                want = NM.neighbor_joining(dist)
            assert len(want) == max(n - 1, 0)
            got, f = ctx_nj_raw(sel, measure)
            assert f == max(n - 1, 0) and got.tobytes() == want.tobytes(), measure
            got, f = ctx_nj_raw(sel, measure, joins=False)
            assert f == max(n - 1, 0) and len(got) == max(n - 1, 0), measure
            got, f = ctx_nj_raw(sel, measure, count=False)
            assert f == -5 and got.tobytes() == want.tobytes(), measure
        if n >= 2:
            sel.run_async(0.5)
            try:
                with pytest.raises(SelhipError, match="still pending") as err:
                    ctx_nj_raw(sel, "jaccard")
                assert err.value.code == -5                                   # SELHIP_E_STATE
            finally:
                sel.finish()
            assert ctx_nj_raw(sel, "jaccard")[1] == n - 1


@pytest.mark.parametrize("args,kw", [([], dict(measure="jaccard")), (["-E", "smh", "-a", "512"], dict(measure="smh_jaccard", aux_bytes=512))], ids=["jaccard", "smh"])
def test_cli(monkeypatch, tmp_path, args, kw):
    monkeypatch.chdir(GOLDEN)
    want = pkg.nj_from_filelist("influenza_filelist.txt", **kw)
    assert want["n_joins"] == len(want["names"]) - 1 and want["newick"].count(",") == want["n_joins"]
    tree, table = tmp_path / "tree.nwk", tmp_path / "joins.tsv"
    out = subprocess.run([str(BIN / "selection"), "-l", "influenza_filelist.txt", "-N", str(tree), "-J", str(table), "-X", "nj"] + args, cwd=GOLDEN,
                         capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout == "", out.stderr
    assert table.read_text() == want["table"] and tree.read_text() == want["newick"]
