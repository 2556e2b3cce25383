"""Auxiliary HLL sketches folded from the main registers on the device: hll_fold_kernel through selhip_hll_fold
against the numpy model (tests/fold_model.py) at the smallest shapes at which each of its three load shapes can go wrong, the context
entries against a context that uploads the model's fold, and the front ends on the influenza fixtures without their .hll_8 files."""
import functools
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import fold_model as M

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import (CRIT_HLL_A, CRIT_HLL_A_SMH_A, CRIT_HLL_AN, MODE_CB_SMH, MODE_SMH, SelhipError, Selector, SynthConfig)

pytestmark = pytest.mark.gpu

SEL = str(ROOT / "cuda_selection_criteria_amd" / "bin" / "selection")
EXP = GOLDEN / "expected"
DEV = "cuda:0"
NS = (0, 1, 2, 3, 64, 65)


def device_fold(regs: np.ndarray, p_aux: int) -> np.ndarray:
    """selhip_hll_fold of host registers [n, 1 << p] through device memory"""
    n, width = regs.shape
    p = width.bit_length() - 1
    lib = pkg.hip_lib()
    if n == 0:
        pkg._lib.check(lib.selhip_hll_fold(None, 0, p, p_aux, None, None))
        return np.zeros((0, 1 << p_aux), dtype=np.uint8)
    src = torch.from_numpy(np.ascontiguousarray(regs)).to(DEV)
    dst = torch.full((n, 1 << p_aux), 0xEE, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    pkg._lib.check(lib.selhip_hll_fold(src.data_ptr(), n, p, p_aux, dst.data_ptr(), None))
    pkg._lib.check(lib.selhip_device_synchronize())
    return dst.cpu().numpy()


# ---- (a) the building block against the model --------------------------------------------------------------------------------
_LAW = np.minimum(np.random.default_rng(9).geometric(0.5, 256), 40).astype(np.uint8)
_LAW[::3] = 0                                            # a third of the byte values map to an empty register


@functools.lru_cache(maxsize=2)
def block_registers(p):
    """valid registers [65, 1 << p], made once per p: a byte-wise table lookup (values 1..40 <= 64 - 20 + 1, a third empty)"""
    rng = np.random.default_rng(300 + p)
    regs = _LAW[rng.integers(0, 256, size=(max(NS), 1 << p), dtype=np.uint8)]
    regs[1, : (1 << p) // 2] = 0                         # long empty runs: groups whose first non-empty register sits far in
    return regs


BLOCK_CASES = [(14, q) for q in range(4, 15)] + [(4, 4), (5, 4), (5, 5), (10, 4), (10, 7), (10, 10), (20, 4), (20, 9), (20, 15)]


@pytest.mark.parametrize("p,p_aux", BLOCK_CASES)
def test_block_is_the_model(p, p_aux):
    regs = block_registers(p)
    want = M.fold(regs, p_aux)
    assert want.any()
    for n in NS:
        got = device_fold(regs[:n], p_aux)
        assert got.shape == (n, 1 << p_aux)
        assert np.array_equal(got, want[:n]), (p, p_aux, n, np.argwhere(got != want[:n])[:4])


def test_block_beyond_2_31_bytes():
    """byte offsets past 2^31 in every shape: 2 200 MiB of registers, empty but for registers planted behind the 2 GiB mark; the
    output in front of it must stay empty and the rest must be the model's fold of the tail"""
    total, mark = 2200 << 20, 1 << 31
    rng = np.random.default_rng(31)
    pos = np.unique(np.concatenate([rng.integers(mark, total, 5000), [mark, mark + 1, total - 1, total - (1 << 16)]]))
    vals = rng.integers(1, 41, len(pos)).astype(np.uint8)
    buf = torch.zeros(total, dtype=torch.uint8, device=DEV)
    buf[torch.from_numpy(pos).to(DEV)] = torch.from_numpy(vals).to(DEV)
    tail = np.zeros(total - mark, dtype=np.uint8)
    tail[pos - mark] = vals
    lib = pkg.hip_lib()
    for p, p_aux in ((14, 12), (14, 4), (20, 4)):            # in a lane, across lanes, across loads
        n, d = total >> p, p - p_aux
        out = torch.full((total >> d,), 0xEE, dtype=torch.uint8, device=DEV)
        pkg._lib.check(lib.selhip_hll_fold(buf.data_ptr(), n, p, p_aux, out.data_ptr(), None))
        pkg._lib.check(lib.selhip_device_synchronize())
        want = M.fold(tail.reshape(-1, 1 << p), p_aux).reshape(-1)
        assert want.any() and int(torch.count_nonzero(out[: mark >> d])) == 0, (p, p_aux)
        assert np.array_equal(out[mark >> d:].cpu().numpy(), want), (p, p_aux)


# ---- (b) every position of a group ---------------------------------------------------------------------------------------------
def positioned(p, p_aux, kind, seed):
    """registers in which group G (counted over all genomes) has its first non-empty register at offset G mod 2^d:
    kind 0 that register alone, kind 1 a second one at a random larger offset, kind 2 offset 0 non-empty beside both"""
    d = p - p_aux
    n = max(1, (1 << d) >> p_aux)
    groups = n << p_aux
    rng = np.random.default_rng(seed)
    regs = np.zeros((groups, 1 << d), dtype=np.uint8)
    cap = 64 - p + 1
    g = np.arange(groups)
    t1 = g % (1 << d)
    regs[g, t1] = rng.integers(1, cap + 1, groups)
    if kind >= 1:
        t2 = t1 + 1 + rng.integers(0, 1 << d, groups) % np.maximum(1, (1 << d) - 1 - t1)
        has = t2 < (1 << d)
        regs[g[has], t2[has]] = rng.integers(1, cap + 1, int(has.sum()))
    if kind == 2:
        regs[g, 0] = rng.integers(1, cap + 1, groups)
    assert set(t1.tolist()) == set(range(1 << d))
    return regs.reshape(n, 1 << p)


@pytest.mark.parametrize("p_aux", range(4, 14))
def test_every_offset_of_a_group(p_aux):
    p = 14
    d = p - p_aux
    for kind in (0, 1, 2):
        regs = positioned(p, p_aux, kind, 40 * p_aux + kind)
        want = M.fold(regs, p_aux)
        if kind == 0:                                    # the model's answer is known in closed form here
            t = np.arange(regs.shape[0] << p_aux) % (1 << d)
            first = regs.reshape(-1, 1 << d)[np.arange(len(t)), t].astype(np.int64)
            closed = np.where(t == 0, d + first, d - np.floor(np.log2(np.maximum(t, 1))).astype(np.int64))
            assert np.array_equal(want.reshape(-1), closed)
        got = device_fold(regs, p_aux)
        assert np.array_equal(got, want), (p_aux, kind, np.argwhere(got != want)[:4])


# ---- (c) sketches that were built at both precisions from the same hashes ---------------------------------------------------------
@pytest.mark.parametrize("p_aux", range(4, 13))
def test_fold_of_synthetic_main_is_synthetic_aux(p_aux):
    """selhip_synth_generate writes main and auxiliary registers from the same hashes (the generator takes p_aux <= 12)"""
    cfg = SynthConfig("fold-synth", 67, 64, 0.9, 0x5EED0F01 + p_aux, p_aux=p_aux, mode=1, n_sh_lo=3_000, n_sh_hi=120_000)
    hll_t, _, _, _, aux_t = pkg.synth_device(cfg, sort=False)
    out = torch.full_like(aux_t, 0xEE)
    lib = pkg.hip_lib()
    pkg._lib.check(lib.selhip_hll_fold(hll_t.data_ptr(), cfg.n_genomes, 14, p_aux, out.data_ptr(), None))
    pkg._lib.check(lib.selhip_device_synchronize())
    assert aux_t.any() and torch.equal(out, aux_t)


def test_fold_of_hashed_sketches_p13():
    """the precision the synthetic generator does not reach: sketches built by the model's slot() at p = 14 and at p_aux = 13"""
    rng = np.random.default_rng(13)
    main, want = [], []
    for n_h in (1, 50, 4000):
        hashes = rng.integers(0, 1 << 64, n_h, dtype=np.uint64)
        main.append(M.sketch(hashes, 14))
        want.append(M.sketch(hashes, 13))
    assert np.array_equal(device_fold(np.stack(main), 13), np.stack(want))


# ---- (d) the context entries -----------------------------------------------------------------------------------------------------
CFG = SynthConfig("fold-ctx", 129, 128, 0.5, 0x5EED0F00, mode=1, n_sh_lo=8_000, n_sh_hi=60_000)
TAU = 0.5


@pytest.fixture(scope="module")
def planted(oracle):
    hll, aux, _ = pkg.synth_host(CFG)
    cards = oracle.cards(hll)
    perm = pkg.sort_by_card(cards)
    hll, aux, cards = hll[perm], aux[perm], cards[perm]
    return hll, aux, cards, {q: M.fold(hll, q) for q in (4, 5, 8, 12)}


def bits(rec):
    return list(zip(rec["i"].tolist(), rec["k"].tolist(), rec["jaccard"].view(np.uint64).tolist()))


def pair_of_contexts(planted, p_aux, attach=False):
    """(folded, uploaded, kept-alive tensors): two contexts over the planted set, one that folds, one that uploads the model's fold"""
    hll, aux, cards, folds = planted
    a, b = Selector(0), Selector(0)
    keep = None
    if attach:
        keep = (torch.from_numpy(hll).to(DEV), torch.from_numpy(aux.view(np.int64)).to(DEV), torch.from_numpy(cards).to(DEV))
        a.attach(*keep)
    else:
        a.upload(hll, aux, cards)
    a.fold_aux_hll(p_aux)
    b.upload(hll, aux, cards)
    b.upload_aux_hll(folds[p_aux], p_aux)
    return a, b, keep


@pytest.mark.parametrize("attach", [False, True])
@pytest.mark.parametrize("p_aux", [4, 8, 12])
def test_context_fold_equals_upload_allpairs(planted, p_aux, attach):
    a, b, keep = pair_of_contexts(planted, p_aux, attach)
    r, nb = pkg.banding(CFG.m, TAU)
    n_sel = n_cut = 0
    with a, b:
        for crit in (CRIT_HLL_A, CRIT_HLL_AN, CRIT_HLL_A_SMH_A):
            for mode in (MODE_CB_SMH, MODE_SMH):
                a.set_criterion(crit)
                b.set_criterion(crit)
                got, want = a.run(TAU, mode, r, nb), b.run(TAU, mode, r, nb)
                assert bits(got) == bits(want), (crit, mode)
                sa, sb = a.stats(), b.stats()
                assert sa == sb, (crit, mode, sa, sb)
                n_sel += len(want)
                n_cut += sb["evaluated"] - sb["survivors"]
    assert n_sel > 0 and n_cut > 0                       # the criteria both pass and cut pairs here: the sketches were read


def test_context_fold_queries_pairs_topk(planted):
    hll, aux, cards, folds = planted
    p_aux = 8
    r, nb = pkg.banding(CFG.m, TAU)
    q_idx = np.arange(0, len(hll), 4)
    d_idx = np.setdiff1d(np.arange(len(hll)), q_idx)
    rng = np.random.default_rng(3)
    listed = rng.integers(0, len(hll), size=(3000, 2)).astype(np.int32)
    listed = listed[listed[:, 0] != listed[:, 1]]
    n_sel = 0
    with Selector(0) as a, Selector(0) as b:
        # queries against a database, both folded
        a.upload(hll[d_idx], aux[d_idx], cards[d_idx])
        a.upload_queries(hll[q_idx], aux[q_idx], cards[q_idx])
        a.fold_aux_hll(p_aux)
        a.fold_queries_aux_hll(p_aux)
        b.upload(hll[d_idx], aux[d_idx], cards[d_idx])
        b.upload_queries(hll[q_idx], aux[q_idx], cards[q_idx])
        b.upload_aux_hll(folds[p_aux][d_idx], p_aux)
        b.upload_queries_aux_hll(folds[p_aux][q_idx], p_aux)
        for crit in (CRIT_HLL_A, CRIT_HLL_AN, CRIT_HLL_A_SMH_A):
            for mode in (MODE_CB_SMH, MODE_SMH):
                a.set_criterion(crit)
                b.set_criterion(crit)
                got, want = a.run_queries(TAU, mode, r, nb), b.run_queries(TAU, mode, r, nb)
                assert bits(got) == bits(want) and a.stats() == b.stats(), (crit, mode)
                n_sel += len(want)
        assert n_sel > 0
        got, want = a.run_queries(TAU, MODE_SMH, r, nb, top_k=2), b.run_queries(TAU, MODE_SMH, r, nb, top_k=2)
        assert bits(got) == bits(want) and len(want) > 0
        a.set_query_topk(0)
        b.set_query_topk(0)
        # pair-list passes and the all-pairs top-k over the whole set
        a.upload(hll, aux, cards)
        a.fold_aux_hll(p_aux)
        b.upload(hll, aux, cards)
        b.upload_aux_hll(folds[p_aux], p_aux)
        for crit in (CRIT_HLL_A, CRIT_HLL_AN, CRIT_HLL_A_SMH_A):
            a.set_criterion(crit)
            b.set_criterion(crit)
            got, want = a.run_pairs(listed, TAU, MODE_CB_SMH, r, nb), b.run_pairs(listed, TAU, MODE_CB_SMH, r, nb)
            assert bits(got) == bits(want) and a.stats() == b.stats(), crit
        a.set_criterion(CRIT_HLL_A)
        b.set_criterion(CRIT_HLL_A)
        got, want = a.run(TAU, MODE_CB_SMH, r, nb, top_k=3), b.run(TAU, MODE_CB_SMH, r, nb, top_k=3)
        assert bits(got) == bits(want) and len(want) > 0 and a.stats() == b.stats()


def test_context_fold_states_and_ranges(planted):
    hll, aux, cards, folds = planted
    r, nb = pkg.banding(CFG.m, TAU)
    with Selector(0) as a, Selector(0) as b:
        with pytest.raises(SelhipError) as e:            # before an upload
            a.fold_aux_hll(8)
        assert e.value.code == -5
        a.upload(hll, aux, cards)
        with pytest.raises(SelhipError) as e:            # before the queries are loaded
            a.fold_queries_aux_hll(8)
        assert e.value.code == -5
        for bad in (3, 15, 16):
            with pytest.raises(SelhipError) as e:
                a.fold_aux_hll(bad)
            assert e.value.code == -1 and "p_aux" in str(e.value), bad
        a.upload_queries(hll[:5], aux[:5], cards[:5])
        for bad in (3, 15, 16):
            with pytest.raises(SelhipError) as e:
                a.fold_queries_aux_hll(bad)
            assert e.value.code == -1 and "p_aux" in str(e.value), bad
        # while a pass is pending
        a.run_async(TAU, MODE_CB_SMH, r, nb)
        for call in (a.fold_aux_hll, a.fold_queries_aux_hll):
            with pytest.raises(SelhipError) as e:
                call(8)
            assert e.value.code == -5
        a.finish()
        # a later upload of auxiliary sketches replaces the folded ones, and a later fold the uploaded ones
        b.upload(hll, aux, cards)
        b.upload_aux_hll(folds[5], 5)
        b.set_criterion(CRIT_HLL_A)
        a.set_criterion(CRIT_HLL_A)
        want5 = b.run(TAU, MODE_SMH, r, nb)
        st5 = b.stats()
        a.fold_aux_hll(12)
        a.run(TAU, MODE_SMH, r, nb)
        at12 = a.stats()
        a.upload_aux_hll(folds[5], 5)
        assert bits(a.run(TAU, MODE_SMH, r, nb)) == bits(want5) and a.stats() == st5
        assert at12["survivors"] != st5["survivors"]     # (the two precisions do differ on this set: the replacement was visible)
        a.fold_aux_hll(12)
        a.run(TAU, MODE_SMH, r, nb)
        assert a.stats() == at12
        # the main sketches' next upload drops them, as it drops uploaded ones
        a.upload(hll, aux, cards)
        with pytest.raises(SelhipError) as e:
            a.run(TAU, MODE_SMH, r, nb)
        assert e.value.code == -5


def test_context_fold_other_main_precision(oracle):
    """p_hll = 10: the range follows the main precision (4 .. 10), and the pass reads what an upload of the model's fold gives"""
    rng = np.random.default_rng(10)
    n, m, p = 40, 64, 10
    hll = M.random_registers(rng, n, p, 0.7)
    hll[1::2] = np.maximum(hll[0::2], (rng.random((n // 2, 1 << p)) < 0.05).astype(np.uint8) * 3)   # near copies: pairs to select
    aux = rng.integers(0, 1 << 63, size=(n, m), dtype=np.uint64)
    cards = oracle.cards(hll, p)
    perm = pkg.sort_by_card(cards)
    hll, aux, cards = hll[perm], aux[perm], cards[perm]
    with Selector(0) as a, Selector(0) as b:
        a.upload(hll, aux, cards, p_hll=p)
        b.upload(hll, aux, cards, p_hll=p)
        with pytest.raises(SelhipError) as e:
            a.fold_aux_hll(11)
        assert e.value.code == -1
        for p_aux in (4, 7, 10):
            a.fold_aux_hll(p_aux)
            b.upload_aux_hll(M.fold(hll, p_aux), p_aux)
            for crit in (CRIT_HLL_A, CRIT_HLL_AN):
                a.set_criterion(crit)
                b.set_criterion(crit)
                assert bits(a.run(0.5, MODE_SMH, 1, m)) == bits(b.run(0.5, MODE_SMH, 1, m)) and a.stats() == b.stats(), (p_aux, crit)


# ---- (e) the influenza fixtures through the front ends ------------------------------------------------------------------------------
def sel(args, cwd):
    return subprocess.run([SEL] + args, cwd=cwd, capture_output=True, text=True)


@pytest.fixture(scope="module")
def bare(tmp_path_factory):
    """a copy of the influenza fixtures and their list WITHOUT the .hll_8 files"""
    root = tmp_path_factory.mktemp("fold_bare")
    (root / "influenza").mkdir()
    for f in (GOLDEN / "influenza").iterdir():
        if ".hll_" not in f.name:
            shutil.copy(f, root / "influenza" / f.name)
    shutil.copy(GOLDEN / "influenza_filelist.txt", root / "influenza_filelist.txt")
    lines = (GOLDEN / "influenza_filelist.txt").read_text().split()
    return root, lines


@pytest.mark.parametrize("crit", ["hll_a", "hll_an"])
def test_cli_fold_prints_the_expected_bytes(bare, crit):
    root, _ = bare
    base = ["-l", "influenza_filelist.txt", "-a", "256", "-c", crit]
    for h in ("0.9", "0.01"):
        want = (EXP / f"influenza_{crit}_a256_h{h}.fma.txt").read_text()
        assert want
        out = sel(base + ["-h", h, "-D"], GOLDEN)
        assert out.returncode == 0 and out.stdout == want, out.stderr
        out = sel(base + ["-h", h, "-D"], root)          # no .hll_8 file anywhere
        assert out.returncode == 0 and out.stdout == want, out.stderr
        out = sel(base + ["-h", h], root)                # ... which the run without -D needs
        assert out.returncode != 0 and out.stdout == ""
        for extra in (["-B", "4"], ["-B", "3"]):         # the out-of-core driver takes the host twin's fold
            out = sel(base + ["-h", h, "-D"] + extra, root)
            assert out.returncode == 0 and out.stdout == want, (extra, out.stderr)


@pytest.mark.parametrize("crit", ["hll_a", "hll_an"])
def test_python_front_end_fold(bare, crit, monkeypatch):
    root, _ = bare
    monkeypatch.chdir(root)
    want = (EXP / f"influenza_{crit}_a256_h0.9.fma.txt").read_text()
    assert pkg.select_from_filelist("influenza_filelist.txt", 0.9, 256, criterion=crit, fold_aux=True) == want
    with pytest.raises(RuntimeError):
        pkg.select_from_filelist("influenza_filelist.txt", 0.9, 256, criterion=crit)
    monkeypatch.chdir(GOLDEN)
    (root / "pairs.txt").write_text(pkg.select_from_filelist("influenza_filelist.txt", 0.01, 256, criterion=crit))
    listed = pkg.select_pairs_from_filelist("influenza_filelist.txt", str(root / "pairs.txt"), 0.9, 256, criterion=crit)
    monkeypatch.chdir(root)
    assert pkg.select_pairs_from_filelist("influenza_filelist.txt", "pairs.txt", 0.9, 256, criterion=crit, fold_aux=True) == listed == want


@pytest.mark.parametrize("crit", ["hll_a", "hll_an"])
def test_query_and_neighbour_front_ends_fold(bare, crit, tmp_path, monkeypatch):
    root, lines = bare
    (tmp_path / "q.txt").write_text("\n".join(lines[:4]) + "\n")
    (tmp_path / "d.txt").write_text("\n".join(lines[4:]) + "\n")
    for name in ("q.txt", "d.txt"):
        shutil.copy(tmp_path / name, root / name)
    n_lines = 0
    for h in ("0.01",):                                  # (a threshold at which every front end below prints lines)
        args = ["-q", str(tmp_path / "q.txt"), "-l", str(tmp_path / "d.txt"), "-a", "256", "-c", crit, "-h", h]
        with_files = sel(args, GOLDEN)
        assert with_files.returncode == 0, with_files.stderr
        for cwd in (GOLDEN, root):
            out = sel(args + ["-D"], cwd)
            assert out.returncode == 0 and out.stdout == with_files.stdout, out.stderr
        assert sel(args, root).returncode != 0
        out = sel(args + ["-D", "-k", "1"], root)
        assert out.returncode == 0 and out.stdout == sel(args + ["-k", "1"], GOLDEN).stdout
        n_lines += len(with_files.stdout.splitlines())
        nb = ["-l", "influenza_filelist.txt", "-a", "256", "-c", crit, "-h", h, "-K", "2"]
        out = sel(nb + ["-D"], root)
        assert out.returncode == 0 and out.stdout == sel(nb, GOLDEN).stdout and out.stdout, out.stderr
    assert n_lines > 0
    monkeypatch.chdir(root)
    py = pkg.query_from_filelists("q.txt", "d.txt", 0.01, 256, criterion=crit, fold_aux=True)
    monkeypatch.chdir(GOLDEN)
    assert py == pkg.query_from_filelists(str(root / "q.txt"), str(root / "d.txt"), 0.01, 256, criterion=crit) and py
