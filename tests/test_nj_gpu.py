"""The neighbour-joining tree on the device (include/selection_hip.h section 2l) against tests/nj_model.py, bit for bit:
selhip_neighbor_joining into guarded buffers, every case twice and byte-equal, over both scan paths (16-byte and 8-byte loads), the
slot kernels under the "vertex_blocks" hook, the refusals, the context entry and the command line."""
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
    rng = np.random.default_rng(2000 + n)
    sets = {"distinct": (rng.permutation(n * n).reshape(n, n) + rng.random((n, n)) / 2) / float(max(n * n, 1))}
    if n <= 513:
        sets["negative"] = 10.0 * rng.random((n, n)) ** 4                     # far from a metric: negative branch lengths
        if n >= 3:
            sets["dyadic"] = NM.dyadic_tree(n, n)[0]
    if n <= 257:                                                              # ties: the smallest (a, b)
        sets["levels"] = rng.choice([0.25, 0.5, 0.75], size=(n, n))
        sets["equal"] = np.full((n, n), 0.5)
    return {k: (v, NM.neighbor_joining(v)) for k, v in sets.items()}


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
