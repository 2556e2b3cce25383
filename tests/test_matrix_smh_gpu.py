"""The SuperMinHash measures of the dense matrices on the GPU (SELHIP_MEASURE_SMH_MATCHES / _SMH_JACCARD of selhip_ctx_matrix /
selhip_ctx_query_matrix, include/selection_hip.h section 2f).  The count of a cell is an exact integer, so every cell is compared with
`==` against the numpy model of smh_matrix_model.py; the Jaccard cell must be count / m in float64, bit for bit."""
import functools
import subprocess

import numpy as np
import pytest
import torch

import smh_matrix_model as model
from conftest import GOLDEN, ROOT
from test_exhaustive_gpu import assert_same, ranked
from test_matrix_host import read_matrix

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import CRIT_SMH_A, MODE_CB_SMH, SYNTH_CONFIGS, SelhipError, Selector

pytestmark = pytest.mark.gpu

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
SENTINEL = -12345.5
MS = [1, 3, 4, 64, 100, 128, 192, 256, 512, 1024, 2048, 4096]
FAST = (128, 256, 512, 1024)                                  # the m of the fast path
COMBOS = [("smh_matches", torch.float64), ("smh_matches", torch.float32), ("smh_jaccard", torch.float64), ("smh_jaccard", torch.float32)]
NP = {torch.float64: np.float64, torch.float32: np.float32}


@functools.lru_cache(maxsize=None)
def no_hll(n, p=14):
    """n empty HLL sketches: these measures never read them"""
    z = np.zeros((n, 1 << p), dtype=np.uint8)
    z.setflags(write=False)
    return z


def upload(sel, aux):
    sel.upload(no_hll(aux.shape[0]), aux, np.zeros(aux.shape[0]))


def exact(got, want, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    bits = np.uint64 if got.dtype == np.float64 else np.uint32
    ok = got.view(bits) == want.view(bits)
    assert ok.all(), (what, int((~ok).sum()), np.argwhere(~ok)[:5].tolist(), got[~ok][:5].tolist(), want[~ok][:5].tolist())


def check_all(sel, A, B, query, what, want=None):
    """both measures in both dtypes against the model (evaluated once; `want` = its counts where the caller has them); returns the
    f64 count matrix"""
    if want is None:
        want = model.match_counts(A, B)
    want = want.astype(np.float64)
    counts = None
    for measure, dt in COMBOS:
        got = (sel.query_matrix if query else sel.matrix)(measure, dtype=dt)
        assert got.dtype == dt and got.is_cuda
        w = want / np.float64(A.shape[1]) if measure == "smh_jaccard" else want
        exact(got, w.astype(NP[dt]), (what, measure, dt))
        if counts is None:
            counts = got.cpu().numpy()
    return counts


# ---- 1. shapes: every m, self matrices ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", MS)
def test_self_shapes(m):
    with Selector(0) as sel:
        for n in (1, 2, 3, 5, 63, 64, 65, 129):
            aux = model.random_rows(n, m, seed=1000 * m + n)
            upload(sel, aux)
            c = check_all(sel, aux, aux, False, (m, n))
            assert sel.get_param("matrix_smh_path_used") == (1 if m in FAST else 0)
            assert np.array_equal(c.view(np.uint64), c.T.view(np.uint64)) and np.all(np.diagonal(c) == m)
            j = sel.matrix("smh_jaccard").cpu().numpy()
            assert np.all(np.diagonal(j) == 1.0) and np.array_equal(j.view(np.uint64), j.T.view(np.uint64))
            if n == 129 and m >= 64:
                off = c[~np.eye(n, dtype=bool)]
                assert off.min() == 0 and off.max() > 0.8 * m                # the counts spread over 0 .. m


# ---- 2. shapes: every m, query matrices ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", MS)
def test_query_shapes(m):
    with Selector(0) as sel:
        for n_d in (1, 64, 65, 200):
            rows = model.random_rows(n_d + 7, m, seed=77 * m + n_d)
            D = rows[7:]
            upload(sel, D)
            for n_q in (1, 5, 7):
                Q = rows[:n_q]
                sel.upload_queries(no_hll(n_q), Q, np.zeros(n_q))
                c = check_all(sel, Q, D, True, (m, n_q, n_d))
                assert c.shape == (n_q, n_d)
                assert sel.get_param("matrix_smh_path_used") == (1 if m in FAST else 0)


# ---- 3. more than eight spans, a row count that is no multiple of the tile; slabs, positions, the switches, the building block -------------
@functools.lru_cache(maxsize=None)
def big_case():
    aux = model.random_rows(530, 512, seed=530)
    aux.setflags(write=False)
    want = model.match_counts(aux, aux).astype(np.float64)
    want.setflags(write=False)
    return aux, want


def test_many_spans():
    aux, want = big_case()
    n = 530
    with Selector(0) as sel:
        upload(sel, aux)
        for measure, dt in COMBOS:
            w = (want / 512.0 if measure == "smh_jaccard" else want).astype(NP[dt])
            exact(sel.matrix(measure, dtype=dt), w, (measure, dt))
        M = sel.matrix("smh_matches").cpu().numpy()
        assert np.array_equal(M.view(np.uint64), M.T.view(np.uint64)) and np.all(np.diagonal(M) == 512)
        # the whole square computed without a mirror ("matrix_smh_form" 3): the same matrix
        sel.set_param("matrix_smh_form", 3)
        exact(sel.matrix("smh_matches"), want, "form 3")
        sel.set_param("matrix_smh_form", 1)
        with pytest.raises(SelhipError):
            sel.set_param("matrix_smh_form", 2)
        assert sel.get_param("matrix_smh_form") == 1
        # the building block on the device: 500 random pairs
        rng = np.random.default_rng(9)
        pairs = rng.integers(0, n, size=(500, 2)).astype(np.int32)
        d_aux = torch.from_numpy(aux.view(np.int64).copy()).cuda()
        d_pairs = torch.from_numpy(pairs).cuda()
        d_mc = torch.zeros(500, dtype=torch.int32, device="cuda")
        pkg._lib.check(sel._lib.selhip_smh_match_counts(d_aux.data_ptr(), 512, d_pairs.data_ptr(), 500, d_mc.data_ptr(), None))
        torch.cuda.synchronize()
        assert np.array_equal(d_mc.cpu().numpy().astype(np.float64), M[pairs[:, 0], pairs[:, 1]])


@pytest.mark.parametrize("m", [512, 100])
def test_slabs_and_mirror_switch(m):
    n = 200
    aux = model.random_rows(n, m, seed=200 + m)
    whole = model.expected(aux, aux)
    slabs = ((0, 5), (5, 64), (64, 130), (130, 200))
    ident = np.arange(n, dtype=np.int32)
    with Selector(0) as sel:
        upload(sel, aux)
        for measure in ("smh_matches", "smh_jaccard"):
            w = model.expected(aux, aux, measure)
            buf = torch.full((n, n), SENTINEL, dtype=torch.float64, device="cuda")
            for rows in slabs:
                assert sel.matrix(measure, rows=rows, row_pos=ident, out=buf) is buf
            exact(buf, w, "slabs into one buffer")
            parts = [sel.matrix(measure, rows=rows).cpu().numpy() for rows in slabs]
            assert [p.shape for p in parts] == [(b - a, n) for a, b in slabs]
            exact(np.concatenate(parts), w, "slabs from row 0")
            for a, b in slabs[1:3]:                              # one slab alone touches its own rows only (its mirrored stores too)
                buf.fill_(SENTINEL)
                sel.matrix(measure, rows=(a, b), row_pos=ident, out=buf)
                got = buf.cpu().numpy()
                exact(got[a:b], w[a:b], "a slab alone")
                assert np.all(got[:a] == SENTINEL) and np.all(got[b:] == SENTINEL)
        # without mirrored stores a slab writes the columns [0, r0) u [i, n) of each row i, whatever "matrix_smh_form" says
        for form in (1, 3):
            sel.set_param("matrix_smh_form", form)
            sel.set_param("matrix_mirror", 0)
            buf.fill_(SENTINEL)
            sel.matrix("smh_matches", rows=(64, 130), row_pos=ident, out=buf)
            got = buf.cpu().numpy()
            for i in range(64, 130):
                assert np.array_equal(got[i, :64], whole[i, :64]) and np.array_equal(got[i, i:], whole[i, i:])
                assert np.all(got[i, 64:i] == SENTINEL)
            assert np.all(got[:64] == SENTINEL) and np.all(got[130:] == SENTINEL)
            sel.set_param("matrix_mirror", 1)
        sel.set_param("matrix_smh_form", 1)


@pytest.mark.parametrize("m", [512, 100])
def test_positions_ld_and_refusals(m):
    n = 131
    aux = model.random_rows(n, m, seed=131 + m)
    whole = model.expected(aux, aux)
    with Selector(0) as sel:
        upload(sel, aux)
        pos = np.random.default_rng(3).permutation(n).astype(np.int32)
        inv = np.argsort(pos)
        exact(sel.matrix("smh_matches", row_pos=pos, col_pos=pos), whole[inv][:, inv], "permutation")
        big = torch.full((n, n + 7), SENTINEL, dtype=torch.float64, device="cuda")
        sel.matrix("smh_matches", out=big[:, :n])
        got = big.cpu().numpy()
        exact(got[:, :n], whole, "ld")
        assert np.all(got[:, n:] == SENTINEL)
        big32 = torch.full((n, n + 7), SENTINEL, dtype=torch.float32, device="cuda")
        sel.matrix("smh_jaccard", dtype=torch.float32, row_pos=pos, col_pos=pos, out=big32[:, :n])
        got = big32.cpu().numpy()
        exact(got[:, :n], model.expected(aux, aux, "smh_jaccard", np.float32)[inv][:, inv], "f32, positions, ld")
        assert np.all(got[:, n:] == np.float32(SENTINEL))
        # refused before anything is written: positions, ld, ranges, a null buffer
        buf = torch.full((n, n), SENTINEL, dtype=torch.float64, device="cuda")
        for bad_value in (n, -1, 2 ** 31 - 1):
            bad = pos.copy()
            bad[17] = bad_value
            with pytest.raises(SelhipError, match=r"col_pos\[17\]") as ei:
                sel.matrix("smh_matches", col_pos=bad, out=buf)
            assert ei.value.code == -1
            with pytest.raises(SelhipError, match=r"row_pos\[17\]"):
                sel.matrix("smh_jaccard", row_pos=bad, col_pos=pos, out=buf)
        with pytest.raises(SelhipError, match=r"row_pos\[100\]"):
            sel.matrix("smh_matches", out=buf[:100])
        with pytest.raises(SelhipError, match=r"col_pos\[130\]"):
            sel.matrix("smh_matches", out=buf[:, :130].contiguous())
        raw = lambda measure, dtype, r0, r1, ptr, rows, cols, ld: sel._lib.selhip_ctx_matrix(sel._ctx, measure, dtype, r0, r1, ptr, rows, cols, ld, None, None)  # noqa: E731
        p = buf.data_ptr()
        assert raw(16, 0, 0, n, p, n, n, n - 1) == -1 and "ld" in sel._lib.selhip_last_error(sel._ctx).decode()
        assert raw(16, 0, 5, 4, p, n, n, n) == -1
        assert raw(17, 0, 0, n + 1, p, n + 1, n, n) == -1
        assert raw(16, 0, -1, 3, p, n, n, n) == -1
        assert raw(16, 0, 0, n, None, n, n, n) == -1                                   # null buffer, cells to write
        assert raw(16, 0, 0, n, p + 4, n, n, n) == -1                                  # misaligned for f64
        # unknown codes
        for measure in (2, 15, 18, -1):
            assert raw(measure, 0, 0, n, p, n, n, n) == -1
        assert raw(16, 2, 0, n, p, n, n, n) == -1 and raw(17, 2, 0, n, p, n, n, n) == -1
        # a query matrix without queries
        assert sel._lib.selhip_ctx_query_matrix(sel._ctx, 16, 0, 0, 0, p, n, n, n, None, None) == -1
        assert "quer" in sel._lib.selhip_last_error(sel._ctx).decode()
        with pytest.raises(SelhipError):
            sel.query_matrix("smh_matches")
        # empty ranges: fine, nothing written (also without a buffer); their other arguments are checked all the same
        assert raw(16, 0, 7, 7, p, n, n, n) == 0 and raw(16, 0, 7, 7, p, n, n, n - 1) == -1
        assert raw(17, 0, n, n, None, 0, 0, 0) == 0
        assert sel.matrix("smh_matches", rows=(9, 9)).shape == (0, n)
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())
    with Selector(0) as sel:                                     # an empty set: a 0 x 0 matrix
        sel.upload(no_hll(0), aux[:0], np.zeros(0))
        assert sel.matrix("smh_matches").shape == (0, 0)


# ---- 4. every bucket position ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [128, 256, 512, 1024, 100])
def test_every_bucket_position(m):
    with Selector(0) as sel:
        for name, aux, row0 in (("single", model.planted_single(m, 40 + m), 1), ("all but one", model.planted_all_but_one(m, 41 + m), m - 1)):
            upload(sel, aux)
            c = check_all(sel, aux, aux, False, (m, name))
            assert np.all(c[0, 1:] == row0) and np.all(c[1:, 0] == row0), name
            # ... and as queries against the base row alone, and the base row as the one query against all
            sel.upload_queries(no_hll(m), aux[1:], np.zeros(m))
            q = sel.query_matrix("smh_matches").cpu().numpy()
            assert np.all(q[:, 0] == row0), name
            exact(q, c[1:], name)                                # (c equals the model: checked above)


# ---- 5. buckets equal in one dword only ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [128, 512, 100, 3])
def test_half_equal_buckets(m):
    aux = model.half_equal(70, m, seed=5 + m)
    want = model.match_counts(aux, aux)
    assert want[0, 1] < m and want[0, 2] < m
    with Selector(0) as sel:
        upload(sel, aux)
        check_all(sel, aux, aux, False, m)
        sel.upload_queries(no_hll(5), aux[:5], np.zeros(5))
        check_all(sel, aux[:5], aux, True, m)


# ---- 6. empty sketches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [512, 100, 4])
def test_empty_sketches(m):
    aux = model.random_rows(70, m, seed=6 + m)
    aux[[0, 1, 33, 69]] = model.EMPTY
    aux[5, ::2] = model.EMPTY                                    # a filled sketch that holds the empty value in half of its buckets
    with Selector(0) as sel:
        upload(sel, aux)
        c = check_all(sel, aux, aux, False, m)
        assert c[0, 1] == m and c[33, 69] == m and c[0, 0] == m
        assert c[0, 5] == (m + 1) // 2 and c[0, 2] == 0
        assert sel.matrix("smh_jaccard").cpu().numpy()[1, 33] == 1.0


# ---- 7. the passes' state -----------------------------------------------------------------------------------------------------------------
def test_passes_are_left_alone(oracle):
    cfg = SYNTH_CONFIGS["cfg2"]
    n = 200
    hll, aux, _ = pkg.synth_host(cfg, g_range=(0, n))
    hll, aux, cards = ranked(oracle, hll[:n], aux[:n])
    r, b = pkg.banding(cfg.m, cfg.tau)
    want = model.expected(aux, aux)
    buf = torch.full((n, n), SENTINEL, dtype=torch.float64, device="cuda")
    with Selector(0) as sel:
        sel.upload(hll, aux, cards)
        sel.set_criterion(CRIT_SMH_A)
        before, st_before = sel.run(cfg.tau, MODE_CB_SMH, r, b), sel.stats()
        assert len(before) > 0
        sel.timing(True)
        assert_same(sel.run(cfg.tau, MODE_CB_SMH, r, b), before)
        exact(sel.matrix("smh_matches", out=buf), want, "after a pass")
        # one launch per call, under a name of its own; the HLL kernel's timer and the pass's per-pass figures are not touched
        assert sel.kernel_launches("matrix_smh") == 1.0 and sel.kernel_ms("matrix_smh") > 0
        assert sel.kernel_launches("matrix") == 0.0 and sel.kernel_ms("matrix") == -1.0
        assert sel.kernel_launches("total") == 1.0
        sel.matrix("smh_jaccard", dtype=torch.float32)
        assert sel.kernel_launches("matrix_smh") == 1.0
        sel.matrix("jaccard")
        assert sel.kernel_launches("matrix") == 1.0 and sel.kernel_launches("matrix_smh") == 1.0
        sel.timing(False)
        assert sel.result_count() == len(before) and sel.stats() == st_before
        assert_same(sel.fetch(), before)
        assert_same(sel.run(cfg.tau, MODE_CB_SMH, r, b), before)
        assert sel.stats() == st_before
        # a pending pass: SELHIP_E_STATE, nothing written
        buf.fill_(SENTINEL)
        sel.run_async(cfg.tau, MODE_CB_SMH, r, b)
        with pytest.raises(SelhipError) as ei:
            sel.matrix("smh_matches", out=buf)
        assert ei.value.code == -5
        sel.finish()
        assert_same(sel.fetch(), before)
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())


# ---- 8. independence from the HLL state ------------------------------------------------------------------------------------------------
def test_independent_of_the_hll_state():
    n, m = 70, 512
    aux = model.random_rows(n, m, seed=8)
    want = model.expected(aux, aux)
    with Selector(0) as sel:
        # sketches at another p_hll
        sel.upload(no_hll(n, 12), aux, None, p_hll=12)
        exact(sel.matrix("smh_matches"), want, "p_hll 12")
        with pytest.raises(SelhipError, match="matrix"):
            sel.matrix("jaccard")
        with pytest.raises(SelhipError, match="matrix"):
            sel.matrix("union")
        # no bit planes
        sel.set_param("hist_algo", 0)
        upload(sel, aux)
        exact(sel.matrix("smh_matches"), want, "hist_algo 0")
        exact(sel.matrix("smh_jaccard"), want / m, "hist_algo 0")
        sel.upload_queries(no_hll(5), aux[:5], np.zeros(5))
        exact(sel.query_matrix("smh_matches"), want[:5], "hist_algo 0, queries")
        with pytest.raises(SelhipError, match="matrix") as ei:
            sel.matrix("jaccard")
        assert ei.value.code == -1
        with pytest.raises(SelhipError, match="matrix"):
            sel.query_matrix("union")
        sel.set_param("hist_algo", -1)
    # attached device arrays are read in place; an 8-byte-offset view is refused at the attach (the fast path's 16-byte loads never see it)
    with Selector(0) as sel:
        hll_t = torch.zeros((n, 16384), dtype=torch.uint8, device="cuda")
        flat = torch.zeros(n * m + 1, dtype=torch.int64, device="cuda")
        flat[1:] = torch.from_numpy(aux.view(np.int64).reshape(-1).copy()).cuda()
        cards_t = torch.zeros(n, dtype=torch.float64, device="cuda")
        with pytest.raises(SelhipError, match="aligned"):
            sel.attach(hll_t, flat[1:].view(n, m), cards_t)
        aux_t = flat[1:].view(n, m).clone()
        sel.attach(hll_t, aux_t, cards_t)
        exact(sel.matrix("smh_matches"), want, "attached")
        assert sel.get_param("matrix_smh_path_used") == 1
        sel.upload_queries(no_hll(3), aux[:3], np.zeros(3))
        with pytest.raises(SelhipError, match="aligned"):
            sel.attach_queries(hll_t[:3], flat[1:1 + 3 * m].view(3, m), cards_t[:3])


# ---- 9. the fixtures and the command line ---------------------------------------------------------------------------------------------------
def selection(args, ok=True):
    out = subprocess.run([str(BIN / "selection")] + args, cwd=GOLDEN, capture_output=True, text=True)
    assert (out.returncode == 0) == ok, (out.returncode, out.stderr)
    return out


@pytest.mark.parametrize("m", [4, 64, 512])
def test_influenza_and_cli(tmp_path, monkeypatch, m):
    monkeypatch.chdir(GOLDEN)
    listed = [l.strip() for l in (GOLDEN / "influenza_filelist.txt").read_text().splitlines() if l.strip()]
    ds = pkg.load_dataset("influenza_filelist.txt", m)
    file_order = np.argsort(ds.order)                           # file_order[line] = rank
    rows = ds.aux[file_order]
    counts = model.expected(rows, rows)
    names, got = pkg.matrix_from_filelist("influenza_filelist.txt", 8 * m, measure="smh_matches")
    assert names == listed
    exact(got, counts, "file-list order")
    _, got_j = pkg.matrix_from_filelist("influenza_filelist.txt", 8 * m, measure="smh_jaccard", dtype=torch.float32)
    exact(got_j, model.expected(rows, rows, "smh_jaccard", np.float32), "jaccard f32")
    for est, want in (("smh_matches", counts), ("smh", counts / m)):
        path = tmp_path / f"{est}.tsv"
        selection(["-l", "influenza_filelist.txt", "-a", str(8 * m), "-M", str(path), "-E", est])
        r_names, c_names, table = read_matrix(path)
        assert r_names == listed and c_names == listed
        exact(table, want, est)
    assert "\t" + str(m) + "\t" in (tmp_path / "smh_matches.tsv").read_text().splitlines()[1] + "\t"      # a count prints as an integer
    # -q: rows = the query list, columns = the database list, each in the order of its file
    q_names, d_names = listed[::3], [x for j, x in enumerate(listed) if j % 3]
    (tmp_path / "q.txt").write_text("\n".join(q_names) + "\n")
    (tmp_path / "d.txt").write_text("\n".join(d_names) + "\n")
    qi, di = [listed.index(x) for x in q_names], [listed.index(x) for x in d_names]
    qn, dn, got = pkg.query_matrix_from_filelists(str(tmp_path / "q.txt"), str(tmp_path / "d.txt"), 8 * m, measure="smh_matches")
    assert qn == q_names and dn == d_names
    exact(got, counts[qi][:, di], "query lists")
    for est, want in (("smh_matches", counts), ("smh", counts / m)):
        path = tmp_path / f"q_{est}.tsv"
        selection(["-l", str(tmp_path / "d.txt"), "-q", str(tmp_path / "q.txt"), "-a", str(8 * m), "-M", str(path), "-E", est])
        r_names, c_names, table = read_matrix(path)
        assert r_names == q_names and c_names == d_names
        exact(table, want[qi][:, di], "-q " + est)
    # -E hll is the default
    if m == 512:
        selection(["-l", "influenza_filelist.txt", "-M", str(tmp_path / "a.tsv")])
        selection(["-l", "influenza_filelist.txt", "-M", str(tmp_path / "b.tsv"), "-E", "hll", "-a", "512"])
        assert (tmp_path / "a.tsv").read_bytes() == (tmp_path / "b.tsv").read_bytes()
