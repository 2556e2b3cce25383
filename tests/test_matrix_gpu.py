"""Dense matrices on the GPU (selhip_ctx_matrix / selhip_ctx_query_matrix, include/selection_hip.h section 2f).
Expected values: a cell's U is oracle.union_size(a, b) under oracle.set_fma(flavour), its J is (f64(e_a) + f64(e_b) - U) / U with the
truncated cardinalities; everything is compared as uint64 bit patterns (two NaNs count as equal)."""
import functools
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from test_exhaustive_gpu import assert_same, ranked, split
from test_matrix_host import read_matrix, same_bits

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import (CRIT_NONE, CRIT_SMH_A, FP_FMA, FP_STRICT, MODE_CB_SMH, MODE_SMH, SYNTH_CONFIGS, SelhipError,
                                         Selector)

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
EXP = GOLDEN / "expected"
FLAVOURS = [FP_FMA, FP_STRICT]
SENTINEL = -12345.5


@functools.lru_cache(maxsize=None)
def synth(cfg_name, n):
    hll, aux, _ = pkg.synth_host(SYNTH_CONFIGS[cfg_name], g_range=(0, max(n, 1)))
    hll, aux = hll[:n], aux[:n]
    hll.setflags(write=False)
    aux.setflags(write=False)
    return hll, aux


def union_cells(oracle, hll_r, hll_c, fp, cells=None):
    """U of the listed (row, column) cells -- all of them by default -- from the oracle; NaN elsewhere"""
    out = np.full((hll_r.shape[0], hll_c.shape[0]), np.nan)
    oracle.set_fma(fp)
    try:
        if cells is None:
            cells = ((i, k) for i in range(hll_r.shape[0]) for k in range(hll_c.shape[0]))
        for i, k in cells:
            out[i, k] = oracle.union_size(hll_r[i], hll_c[k])
    finally:
        oracle.set_fma(1)
    return out


def jaccard_of(U, cards_r, cards_c, diagonal_one=False):
    e_r = cards_r.astype(np.int64).astype(np.float64)[:, None]
    e_c = cards_c.astype(np.int64).astype(np.float64)[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        J = (e_r + e_c - U) / U
    if diagonal_one:
        J[np.diag_indices(min(J.shape))] = 1.0
    return J


def assert_bits(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = (np.isnan(got) & np.isnan(want)) | (got.view(np.uint64) == want.view(np.uint64))
    assert ok.all(), (what, int((~ok).sum()), np.argwhere(~ok)[:5].tolist())


def self_case(oracle, hll, aux, fp):
    """the ranked set uploaded to a context, and the oracle's U and J matrices"""
    hll, aux, cards = ranked(oracle, hll, aux, fp)
    U = union_cells(oracle, hll, hll, fp)
    return hll, aux, cards, U, jaccard_of(U, cards, cards, diagonal_one=True)


# ---- 1. small shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 63, 64, 65, 129])
@pytest.mark.parametrize("fp", FLAVOURS)
def test_small_shapes(oracle, n, fp):
    hll, aux, cards, U, J = self_case(oracle, *synth("cfg2-spread", n), fp)
    with Selector(0, fp) as sel:
        sel.upload(hll, aux, cards)
        got_j, got_u = sel.matrix("jaccard"), sel.matrix("union")
    assert got_j.shape == (n, n) and got_j.dtype == torch.float64 and got_j.is_cuda
    assert_bits(got_u, U, "union")
    assert_bits(got_j, J, "jaccard")
    for got in (got_j.cpu().numpy(), got_u.cpu().numpy()):
        assert np.array_equal(got.view(np.uint64), got.T.view(np.uint64))            # bit-symmetric
    assert np.all(np.diagonal(got_j.cpu().numpy()) == 1.0)
    oracle.set_fma(fp)
    try:
        diag = np.array([oracle.union_size(hll[g], hll[g]) for g in range(n)])
    finally:
        oracle.set_fma(1)
    assert np.array_equal(np.diagonal(got_u.cpu().numpy()).view(np.uint64), diag.view(np.uint64))


# ---- 2. more than eight spans, a row count that is no multiple of 4 ------------------------------------------------------------------
def test_many_spans_equal_the_none_pass(oracle):
    n = 530
    hll, aux, cards = ranked(oracle, *synth("cfg2", n))
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        M = sel.matrix("jaccard").cpu().numpy()
        sel.set_criterion(CRIT_NONE)
        rec = sel.run(-1.0, MODE_SMH, 1, 1)
    assert len(rec) > n * (n - 1) // 2 - n                      # (all pairs but those of empty sketches, of which cfg2 has none)
    R = np.full((n, n), np.nan)
    R[rec["i"], rec["k"]] = rec["jaccard"]
    R[rec["k"], rec["i"]] = rec["jaccard"]
    off = ~np.eye(n, dtype=bool)
    assert_bits(np.where(off, M, 0.0), np.where(off, R, 0.0), "records")   # present: the record's bits; absent: NaN in the matrix
    assert np.array_equal(M.view(np.uint64), M.T.view(np.uint64)) and np.all(np.diagonal(M) == 1.0)
    rng = np.random.default_rng(20)
    cells = {(int(i), int(k)) for i, k in zip(rng.integers(0, n, 300), rng.integers(0, n, 300))}
    cells |= {(n - 1, k) for k in range(n)} | {(i, n - 1) for i in range(n)}
    U = union_cells(oracle, hll, hll, FP_FMA, sorted(cells))
    J = jaccard_of(U, cards, cards, diagonal_one=True)
    picked = ~np.isnan(U)
    assert picked.sum() == len(cells)
    assert_bits(M[picked], J[picked], "oracle cells")


# ---- 3. reference-pinned -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp,flavour", [(FP_FMA, "fma"), (FP_STRICT, "nofma")])
def test_influenza_union_equals_the_reference(monkeypatch, fp, flavour):
    monkeypatch.chdir(GOLDEN)
    listed = [l.strip() for l in (GOLDEN / "influenza_filelist.txt").read_text().splitlines() if l.strip()]
    names, M = pkg.matrix_from_filelist("influenza_filelist.txt", 512, measure="union", fp_mode=fp)
    assert names == listed                                      # file-list order
    M = M.cpu().numpy()
    assert M.shape == (10, 10)
    seen_u = seen_r = 0
    for line in (EXP / f"influenza_kat_hll.{flavour}.txt").read_text().splitlines():
        t = line.split()
        want = np.float64(float.fromhex(t[-1]))
        if t[0] == "U":
            i, k = int(t[1]), int(t[2])
            assert M[i, k].view(np.uint64) == want.view(np.uint64) and M[k, i].view(np.uint64) == want.view(np.uint64), line
            seen_u += 1
        elif t[0] == "R":
            i = int(t[1])
            assert M[i, i].view(np.uint64) == want.view(np.uint64), line
            seen_r += 1
    assert (seen_u, seen_r) == (45, 10)


# ---- 4. every instantiation ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vmax", [15, 16, 31, 32, 51])
def test_high_registers(oracle, vmax):
    """four, five and six planes, and every optional walk of bs_pair_hist (the recipe of test_exhaustive_gpu.test_high_registers)"""
    rng = np.random.default_rng(100 + vmax)
    n = 70
    hll = np.minimum(rng.geometric(0.5, size=(n, 16384)), vmax).astype(np.uint8)
    hll[1::2] = np.maximum(hll[1::2], hll[0::2])
    hll[::3, ::97] = vmax
    for g, cap_v in zip(range(5, 14), (3, 15, 17, 19, 20, 23, 24, 27, 31)):
        hll[g] = np.minimum(hll[g], min(cap_v, vmax))
    hll, aux, cards, U, J = self_case(oracle, hll, np.zeros((n, 4), dtype=np.uint64), FP_FMA)
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        assert sel.get_param("hll_khi") == vmax + 1
        assert_bits(sel.matrix("union"), U, "union")
        assert_bits(sel.matrix("jaccard"), J, "jaccard")


# ---- 5. empty sketches -----------------------------------------------------------------------------------------------------------------
def test_empty_sketches(oracle):
    hll, aux = synth("cfg2-spread", 150)
    hll = hll.copy()
    hll[:3] = 0
    hll, aux, cards, U, J = self_case(oracle, hll, aux, FP_FMA)
    assert np.all(cards[:3] == 0) and cards[3] > 0
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        got_j, got_u = sel.matrix("jaccard").cpu().numpy(), sel.matrix("union").cpu().numpy()
    for i in range(3):
        for k in range(3):
            assert got_u[i, k] == 0.0
            assert got_j[i, k] == 1.0 if i == k else np.isnan(got_j[i, k])
    assert not np.isnan(got_j[:, 3:]).any()
    assert_bits(got_u, U, "union")
    assert_bits(got_j, J, "jaccard")


# ---- 6. slabs ------------------------------------------------------------------------------------------------------------------------
def test_slabs(oracle):
    n = 200
    hll, aux, cards = ranked(oracle, *synth("cfg2-spread", n))
    slabs = ((0, 5), (5, 64), (64, 130), (130, 200))
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        for measure in ("jaccard", "union"):
            whole = sel.matrix(measure).cpu().numpy()
            buf = torch.full((n, n), SENTINEL, dtype=torch.float64, device="cuda")
            ident = np.arange(n, dtype=np.int32)
            for rows in slabs:
                assert sel.matrix(measure, rows=rows, row_pos=ident, out=buf) is buf
            assert np.array_equal(buf.cpu().numpy().view(np.uint64), whole.view(np.uint64))
            # the default positions: a slab's rows from 0 on
            parts = [sel.matrix(measure, rows=rows).cpu().numpy() for rows in slabs]
            assert [p.shape for p in parts] == [(b - a, n) for a, b in slabs]
            assert np.array_equal(np.concatenate(parts).view(np.uint64), whole.view(np.uint64))
            # one slab alone touches its own rows only (its mirrored stores too)
            for a, b in slabs[1:3]:
                buf.fill_(SENTINEL)
                sel.matrix(measure, rows=(a, b), row_pos=ident, out=buf)
                got = buf.cpu().numpy()
                assert np.array_equal(got[a:b].view(np.uint64), whole[a:b].view(np.uint64))
                assert np.all(got[:a] == SENTINEL) and np.all(got[b:] == SENTINEL)
        # the measurement switch: without mirrored stores a slab writes the columns [0, r0) u [i, n) of each row i
        sel.set_param("matrix_mirror", 0)
        buf.fill_(SENTINEL)
        sel.matrix("union", rows=(64, 130), row_pos=ident, out=buf)
        got = buf.cpu().numpy()
        for i in (64, 65, 100, 129):
            assert np.array_equal(got[i, :64].view(np.uint64), whole[i, :64].view(np.uint64))
            assert np.array_equal(got[i, i:].view(np.uint64), whole[i, i:].view(np.uint64))
            assert np.all(got[i, 64:i] == SENTINEL)
        sel.set_param("matrix_mirror", 1)


# ---- 7. positions, ld, dtype -----------------------------------------------------------------------------------------------------------
def test_positions_ld_dtype(oracle):
    n = 131
    hll, aux, cards = ranked(oracle, *synth("cfg2-spread", n))
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        whole = sel.matrix("jaccard").cpu().numpy()
        # a permutation as both position arrays: out[pos[i], pos[k]] = whole[i, k]
        pos = np.random.default_rng(3).permutation(n).astype(np.int32)
        inv = np.argsort(pos)
        got = sel.matrix("jaccard", row_pos=pos, col_pos=pos).cpu().numpy()
        assert np.array_equal(got.view(np.uint64), whole[inv][:, inv].view(np.uint64))
        # ld = cols + 7: the padding keeps the sentinel
        big = torch.full((n, n + 7), SENTINEL, dtype=torch.float64, device="cuda")
        view = big[:, :n]
        assert view.stride(0) == n + 7
        sel.matrix("jaccard", out=view)
        got = big.cpu().numpy()
        assert np.array_equal(got[:, :n].view(np.uint64), whole.view(np.uint64)) and np.all(got[:, n:] == SENTINEL)
        # f32 = (float) of the f64 value, NaN where it is NaN
        got32 = sel.matrix("jaccard", dtype=torch.float32).cpu().numpy()
        assert got32.dtype == np.float32
        want32 = whole.astype(np.float32)
        assert np.array_equal(np.isnan(got32), np.isnan(want32))
        assert np.array_equal(got32.view(np.uint32)[~np.isnan(want32)], want32.view(np.uint32)[~np.isnan(want32)])
        big32 = torch.full((n, n + 7), SENTINEL, dtype=torch.float32, device="cuda")
        sel.matrix("union", dtype=torch.float32, row_pos=pos, col_pos=pos, out=big32[:, :n])
        u32 = sel.matrix("union").cpu().numpy().astype(np.float32)[inv][:, inv]
        got = big32.cpu().numpy()
        assert np.array_equal(got[:, :n].view(np.uint32), u32.view(np.uint32)) and np.all(got[:, n:] == np.float32(SENTINEL))
        # a position out of range: refused with its index before anything is written
        buf = torch.full((n, n), SENTINEL, dtype=torch.float64, device="cuda")
        for bad_value in (n, -1, 2 ** 31 - 1):
            bad = pos.copy()
            bad[17] = bad_value
            with pytest.raises(SelhipError, match=r"col_pos\[17\]") as ei:
                sel.matrix("jaccard", col_pos=bad, out=buf)
            assert ei.value.code == -1
            with pytest.raises(SelhipError, match=r"row_pos\[17\]"):
                sel.matrix("jaccard", row_pos=bad, col_pos=pos, out=buf)
        # the default positions are checked like given ones: a buffer with too few rows / columns
        with pytest.raises(SelhipError, match=r"row_pos\[100\]"):
            sel.matrix("jaccard", out=buf[:100])
        with pytest.raises(SelhipError, match=r"col_pos\[130\]"):
            sel.matrix("jaccard", out=buf[:, :130].contiguous())
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())


# ---- 8. query matrices -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_q", [1, 5, 67])
def test_query_matrix(oracle, n_q):
    fp = FP_FMA if n_q != 5 else FP_STRICT
    hll, aux = synth("cfg2-spread", 300 + n_q)
    Q, D = split(oracle, hll, aux, n_q, seed=11 + n_q, fp=fp)
    n_d = 300
    U = union_cells(oracle, Q[0], D[0], fp)
    J = jaccard_of(U, Q[2], D[2])
    # the self matrix over Q u D (in its own rank order), cut to the cross cells
    all_hll, all_aux, all_cards = np.concatenate([Q[0], D[0]]), np.concatenate([Q[1], D[1]]), np.concatenate([Q[2], D[2]])
    perm = pkg.sort_by_card(all_cards)                          # perm[rank] = index in Q u D: the position that rank's row and column go to
    with Selector(0, fp) as sel:
        sel.upload(all_hll[perm], all_aux[perm], all_cards[perm])
        union_self = {m: sel.matrix(m, row_pos=perm, col_pos=perm).cpu().numpy()[:n_q, n_q:] for m in ("jaccard", "union")}
    with Selector(0, fp) as sel:
        sel.upload(D[0], D[1], D[2])
        sel.upload_queries(Q[0], Q[1], Q[2])
        got_j, got_u = sel.query_matrix("jaccard"), sel.query_matrix("union")
        assert got_j.shape == (n_q, n_d)
        assert_bits(got_u, U, "union")
        assert_bits(got_j, J, "jaccard")
        assert np.array_equal(got_j.cpu().numpy().view(np.uint64), union_self["jaccard"].view(np.uint64))
        assert np.array_equal(got_u.cpu().numpy().view(np.uint64), union_self["union"].view(np.uint64))
        whole = got_j.cpu().numpy()
        # row slabs into one buffer, and alone
        cuts = sorted({0, min(1, n_q), n_q // 2, n_q})
        buf = torch.full((n_q, n_d), SENTINEL, dtype=torch.float64, device="cuda")
        ident = np.arange(n_q, dtype=np.int32)
        for a, b in zip(cuts[:-1], cuts[1:]):
            sel.query_matrix("jaccard", rows=(a, b), row_pos=ident, out=buf)
        assert np.array_equal(buf.cpu().numpy().view(np.uint64), whole.view(np.uint64))
        a, b = cuts[-2], cuts[-1]
        buf.fill_(SENTINEL)
        sel.query_matrix("jaccard", rows=(a, b), row_pos=ident, out=buf)
        got = buf.cpu().numpy()
        assert np.array_equal(got[a:b].view(np.uint64), whole[a:b].view(np.uint64)) and np.all(got[:a] == SENTINEL)
        # positions and ld
        rp = np.random.default_rng(5).permutation(n_q).astype(np.int32)
        cp = np.random.default_rng(6).permutation(n_d).astype(np.int32)
        big = torch.full((n_q, n_d + 7), SENTINEL, dtype=torch.float64, device="cuda")
        sel.query_matrix("jaccard", row_pos=rp, col_pos=cp, out=big[:, :n_d])
        got = big.cpu().numpy()
        assert np.array_equal(got[:, :n_d].view(np.uint64), whole[np.argsort(rp)][:, np.argsort(cp)].view(np.uint64))
        assert np.all(got[:, n_d:] == SENTINEL)
        bad = cp.copy()
        bad[299] = n_d
        buf.fill_(SENTINEL)
        with pytest.raises(SelhipError, match=r"col_pos\[299\]"):
            sel.query_matrix("jaccard", col_pos=bad, out=buf)
        assert bool((buf == SENTINEL).all())


# ---- 9. neighbours and refusals ------------------------------------------------------------------------------------------------------------
def raw_matrix(sel, fn, r0, r1, out, out_rows, out_cols, ld):
    return getattr(sel._lib, fn)(sel._ctx, 0, 0, r0, r1, out.data_ptr(), out_rows, out_cols, ld, None, None)


def test_neighbours_and_refusals(oracle):
    cfg = SYNTH_CONFIGS["cfg2"]
    hll, aux, cards = ranked(oracle, *synth("cfg2", 200))
    n = 200
    r, b = pkg.banding(cfg.m, cfg.tau)
    buf = torch.full((n, n), SENTINEL, dtype=torch.float64, device="cuda")
    with Selector(0) as sel:
        # p_hll != 14: refused, with a message that names the matrix
        sel.upload(hll[:, :4096], aux, None, p_hll=12)
        with pytest.raises(SelhipError, match="matrix"):
            sel.matrix(out=buf)
        # no bit planes (byte-row stage 2a chosen before the upload): refused as well, no fallback
        sel.set_param("hist_algo", 0)
        sel.upload(hll, aux, cards)
        with pytest.raises(SelhipError, match="matrix") as ei:
            sel.matrix(out=buf)
        assert ei.value.code == -1
        sel.set_param("hist_algo", -1)
        # an smh_a pass returns the same before and after matrix calls; the result list and its count stay
        sel.upload(hll, aux, cards)
        sel.set_criterion(CRIT_SMH_A)
        before, st_before = sel.run(cfg.tau, MODE_CB_SMH, r, b), sel.stats()
        assert len(before) > 0
        sel.timing(True)
        assert_same(sel.run(cfg.tau, MODE_CB_SMH, r, b), before)
        sel.matrix("jaccard", out=buf)
        sel.matrix("union", dtype=torch.float32)
        assert sel.kernel_ms("matrix") > 0
        # matrix calls are counted apart from the passes: one launch per call, and the pass's own per-pass figures stay per pass
        assert sel.kernel_launches("matrix") == 1.0 and sel.kernel_launches("total") == 1.0
        sel.timing(False)
        assert sel.get_param("matrix_mirror") == 1
        assert sel.result_count() == len(before) and sel.stats() == st_before
        assert_same(sel.fetch(), before)
        assert_same(sel.run(cfg.tau, MODE_CB_SMH, r, b), before)
        assert sel.stats() == st_before
        # argument errors, each before anything is written
        buf.fill_(SENTINEL)
        assert raw_matrix(sel, "selhip_ctx_matrix", 0, n, buf, n, n, n - 1) == -1                 # ld < out_cols
        assert "ld" in sel._lib.selhip_last_error(sel._ctx).decode()
        assert raw_matrix(sel, "selhip_ctx_matrix", 5, 4, buf, n, n, n) == -1                     # r0 > r1
        assert raw_matrix(sel, "selhip_ctx_matrix", 0, n + 1, buf, n + 1, n, n) == -1             # a range outside the set
        assert raw_matrix(sel, "selhip_ctx_matrix", -1, 3, buf, n, n, n) == -1
        assert sel._lib.selhip_ctx_matrix(sel._ctx, 0, 0, 0, n, None, n, n, n, None, None) == -1   # null buffer, cells to write
        assert sel._lib.selhip_ctx_matrix(sel._ctx, 2, 0, 0, n, buf.data_ptr(), n, n, n, None, None) == -1   # unknown measure
        assert sel._lib.selhip_ctx_matrix(sel._ctx, 0, 2, 0, n, buf.data_ptr(), n, n, n, None, None) == -1   # unknown dtype
        assert raw_matrix(sel, "selhip_ctx_query_matrix", 0, 0, buf, n, n, n) == -1               # no queries attached
        assert "quer" in sel._lib.selhip_last_error(sel._ctx).decode()
        with pytest.raises(SelhipError):
            sel.query_matrix()
        # an empty range: fine, nothing written (also without a buffer)
        assert raw_matrix(sel, "selhip_ctx_matrix", 7, 7, buf, n, n, n) == 0
        assert raw_matrix(sel, "selhip_ctx_matrix", 7, 7, buf, n, n, n - 1) == -1                 # (its other arguments are checked all the same)
        assert sel._lib.selhip_ctx_matrix(sel._ctx, 0, 0, n, n, None, 0, 0, 0, None, None) == 0
        assert sel.matrix(rows=(9, 9)).shape == (0, n)
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())
    with Selector(0) as sel:                                     # an empty set: a 0 x 0 matrix
        sel.upload(hll[:0], aux[:0], cards[:0])
        assert sel.matrix().shape == (0, 0)


# ---- 10. the CLI -------------------------------------------------------------------------------------------------------------------------
def selection(args, ok=True):
    out = subprocess.run([str(BIN / "selection")] + args, cwd=GOLDEN, capture_output=True, text=True)
    assert (out.returncode == 0) == ok, (out.returncode, out.stderr)
    return out


def test_cli(tmp_path, monkeypatch):
    monkeypatch.chdir(GOLDEN)
    listed = [l.strip() for l in (GOLDEN / "influenza_filelist.txt").read_text().splitlines() if l.strip()]
    for extra, measure in (([], "jaccard"), (["-U"], "union")):
        path = tmp_path / f"{measure}.tsv"
        selection(["-l", "influenza_filelist.txt", "-a", "512", "-M", str(path)] + extra)
        rows, cols, got = read_matrix(path)
        assert rows == listed and cols == listed
        names, want = pkg.matrix_from_filelist("influenza_filelist.txt", 512, measure=measure)
        assert names == listed and same_bits(got, want.cpu().numpy())
    # -F 0: the strict flavour
    selection(["-l", "influenza_filelist.txt", "-a", "512", "-F", "0", "-U", "-M", str(tmp_path / "s.tsv")])
    _, want = pkg.matrix_from_filelist("influenza_filelist.txt", 512, measure="union", fp_mode=FP_STRICT)
    assert same_bits(read_matrix(tmp_path / "s.tsv")[2], want.cpu().numpy())
    # -q: rows = the query list, columns = the database list, each in the order of its file
    q_names, d_names = listed[::3], [x for j, x in enumerate(listed) if j % 3]
    (tmp_path / "q.txt").write_text("\n".join(q_names) + "\n")
    (tmp_path / "d.txt").write_text("\n".join(d_names) + "\n")
    selection(["-l", str(tmp_path / "d.txt"), "-q", str(tmp_path / "q.txt"), "-a", "512", "-M", str(tmp_path / "qd.tsv")])
    rows, cols, got = read_matrix(tmp_path / "qd.tsv")
    assert rows == q_names and cols == d_names
    qn, dn, want = pkg.query_matrix_from_filelists(str(tmp_path / "q.txt"), str(tmp_path / "d.txt"), 512)
    assert qn == q_names and dn == d_names and same_bits(got, want.cpu().numpy())
    _, whole = pkg.matrix_from_filelist("influenza_filelist.txt", 512)
    qi, di = [listed.index(x) for x in q_names], [listed.index(x) for x in d_names]
    assert same_bits(got, whole.cpu().numpy()[qi][:, di])
    # -M runs no selection pass: the options of one are usage errors
    for clash in (["-k", "3"], ["-K", "3"], ["-p", "pairs.txt"], ["-g", "1"], ["-B", "4"], ["-o", "x.selr"], ["-r", "x.selr"],
                  ["-c", "hll_a"], ["-h", "0.9"], ["-n"], ["-A", "sig"]):
        out = selection(["-l", "influenza_filelist.txt", "-a", "512", "-M", str(tmp_path / "no.tsv")] + clash, ok=False)
        assert out.returncode == 2 and "-M" in out.stderr and clash[0] in out.stderr
    assert not (tmp_path / "no.tsv").exists()
