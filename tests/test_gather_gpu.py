"""The winner-takes-all screen on the device (include/selection_hip.h section 2m) against tests/gather_model.py, bit for bit: rows forged
directly as u64 arrays, both entries, both mask kernels (m = 128 NCH and every other m), the staged and the streamed pick route."""
import functools
import subprocess

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
import gather_model as GM

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import CRIT_SMH_C, MODE_SMH, Selector

pytestmark = pytest.mark.gpu

E = GM.EMPTY
SENTINEL = -77


def forge(n_q, n_d, m, seed, n_src=5):
    """database rows = strains of n_src source rows (each with its own share of mutated buckets, some rows unfilled in places), queries =
    bucket-wise mixtures of the sources with a tenth of their buckets unfilled"""
    rng = np.random.default_rng(seed)
    src = rng.integers(1, 1 << 62, (n_src, m)).astype(np.uint64)
    D = src[rng.integers(0, n_src, n_d)]
    noise = rng.random((n_d, m)) < rng.random((n_d, 1))
    D[noise] = rng.integers(1, 1 << 62, int(noise.sum())).astype(np.uint64)
    D[rng.random((n_d, m)) < 0.02] = E
    Q = src[rng.integers(0, n_src, (n_q, m)), np.arange(m)[None, :]]
    Q[rng.random((n_q, m)) < 0.1] = E
    return Q, D


def raw(Q, D, c_min, max_picks, null=(), shift=0):
    """selhip_gather into guarded buffers -> the model's triple; `null`: the outputs passed as NULL (returned as None); shift: u64
    words between a 16-byte boundary and the rows"""
    n_q, m = Q.shape
    dev = lambda a: torch.from_numpy(np.concatenate([np.zeros(shift, np.uint64), a.reshape(-1)]).view(np.int64)).cuda()[shift:]
    q, d = dev(Q), dev(D)
    bufs = [torch.full((n, ), SENTINEL, dtype=torch.int32, device="cuda") for n in (n_q * max_picks * 4 + 8, n_q + 8, n_q + 8)]
    ptr = [None if k in null else b.data_ptr() + 16 for k, b in enumerate(bufs)]
    rc = pkg.hip_lib().selhip_gather(q.data_ptr() if n_q else None, n_q, d.data_ptr() if len(D) else None, len(D), m, c_min, max_picks, *ptr, None)
    assert rc == 0, pkg.hip_lib().selhip_last_error(None).decode()
    picks, n_picks, left = (b.cpu().numpy() for b in bufs)
    for k, b in enumerate((picks, n_picks, left)):
        assert np.all(b[:4] == SENTINEL) and np.all(b[-4:] == SENTINEL) and (k not in null or np.all(b == SENTINEL))
    n_picks, left = n_picks[4:-4], left[4:-4]
    rows = picks[4:-4].reshape(n_q, max_picks, 4)
    if 1 not in null:                                                          # the records behind a query's last pick are not written
        assert all(np.all(rows[i, n_picks[i]:] == SENTINEL) for i in range(n_q))
    flat = None if 0 in null or 1 in null else np.concatenate([rows[i, :n_picks[i]] for i in range(n_q)] + [np.zeros((0, 4), np.int32)])
    return (None if flat is None else np.ascontiguousarray(flat).view(GM.GATHER_DTYPE).reshape(-1), None if 1 in null else n_picks, None if 2 in null else left)


def same(got, want, what):
    for g, w, name in zip(got, want, ("picks", "n_picks", "unexplained")):
        assert g is None or (g.dtype == w.dtype and g.tobytes() == w.tobytes()), (what, name, g[:4], w[:4])


def via_context(Q, D, c_min, max_picks, lds_cap=0):
    with Selector(0) as sel:
        sel.upload(np.zeros((len(D), 1 << 14), np.uint8), D, np.zeros(len(D)))
        sel.upload_queries(np.zeros((len(Q), 1 << 14), np.uint8), Q, np.zeros(len(Q)))
        reported = sel.get_param("gather_lds_cap")
        sel.set_param("gather_lds_cap", lds_cap)
        assert reported >= 32 * 1024 and sel.get_param("gather_lds_cap") == (lds_cap or reported)
        res = sel.gather(c_min, max_picks)
    return res["picks"], res["n_picks"], res["unexplained"]


# m: one case per NCH of the fast path and the generic kernel's 96, 100 (a partial last word), 2 048, 4 096 (live beyond the scalar form);
# n_d: the 64-column spans and their tails; n_q: one row past a wave's rows (12, 6, 3) and one past a tile (48, 24, 12)
@pytest.mark.parametrize("m, n_q, n_d", [(128, 49, 200), (256, 49, 65), (512, 13, 63), (512, 49, 200), (1024, 13, 200), (1024, 1, 1), (96, 13, 65),
                                         (100, 49, 200), (2048, 13, 63), (4096, 1, 200), (4096, 5, 65)])
def test_shapes_against_the_model(m, n_q, n_d):
    Q, D = forge(n_q, n_d, m, seed=m + n_q + n_d)
    for c_min, max_picks in ((1, 64), (3, 64), (16, 2)):
        want = GM.gather(Q, D, c_min, max_picks)
        same(raw(Q, D, c_min, max_picks), want, (c_min, max_picks))
    assert len(GM.gather(Q, D, 1, 64)[0]) > n_q or n_d == 1                   # the sets do decompose
    same(via_context(Q, D, 3, 64), GM.gather(Q, D, 3, 64), "context")
    if m in (128, 100):                                                       # rows off the 16-byte grid take the generic kernel
        same(raw(Q, D, 1, 64, shift=1), GM.gather(Q, D, 1, 64), "unaligned")


@functools.lru_cache(maxsize=None)
def segments(m):
    """four queries whose candidate segments hold 0, 1, 257 and 600 entries of a 700-row database: row d shares 4 + d % 7 buckets of
    query 2 for d < 257 and of query 3 for 50 <= d < 650 -- equal counts in neighbouring lanes (d, d + 7), in different waves
    (d, d + 70) and between a lane's first and a later candidate (d, d + 259) -- and rows 300 and 40 share the same 40 buckets of query 3
    and 2: the tie at the top goes to the smaller rank, then nothing of the twin is left"""
    rng = np.random.default_rng(m)
    Q = rng.integers(1, 1 << 62, (4, m)).astype(np.uint64)
    D = rng.integers(1, 1 << 62, (700, m)).astype(np.uint64)
    D[5, :10] = Q[1, :10]
    for q, lo, hi in ((2, 0, 257), (3, 50, 650)):
        for d in range(lo, hi):
            at = rng.choice(m, 4 + d % 7, replace=False)
            D[d, at] = Q[q, at]
    top = rng.choice(m, 40, replace=False)
    for q, d in ((3, 300), (3, 560), (2, 40), (2, 41)):
        D[d] = rng.integers(1, 1 << 62, m).astype(np.uint64)
        D[d, top] = Q[q, top]
    return Q, D, GM.gather(Q, D, 1, 64), GM.gather(Q, D, 6, 300)


@pytest.mark.parametrize("m", (512, 2048))
@pytest.mark.parametrize("lds_cap", (0, 8))
def test_segment_lengths_staged_and_streamed(m, lds_cap):
    Q, D, want, want6 = segments(m)
    assert want[1].tolist()[:2] == [0, 1] and want[0][want[0]["q"] == 3][0]["d"] == 300 and want[0][want[0]["q"] == 2][0]["d"] == 40
    assert not np.any((want[0]["q"] == 3) & (want[0]["d"] == 560)) and want6[1][3] > 20
    same(via_context(Q, D, 1, 64, lds_cap), want, "c_min 1")
    same(via_context(Q, D, 6, 300, lds_cap), want6, "c_min 6")
    same(raw(Q, D, 6, 300), want6, "context-free")


def test_chain_cut_and_threshold_by_hand():
    """m = 128: A shares buckets 0..49, B 50..89, C 40..59 and 90..92, F 90..99.  c_min = 5: A (50), B (40), then C -- 13 left after A, 3
    after B -- is below c_min and F takes 10; 28 unexplained.  max_picks = 2 stops behind B.  c_min = m takes only a whole copy"""
    Q = np.arange(1, 129, dtype=np.uint64)[None, :] << np.uint64(33)
    D = np.full((5, 128), 7, dtype=np.uint64)
    for d, at in enumerate((range(90, 100), list(range(40, 60)) + [90, 91, 92], range(50, 90), range(0, 50))):
        D[d, list(at)] = Q[0, list(at)]
    D[4] = Q[0]
    D[4, 0] ^= np.uint64(1)                                                    # all but one bucket: not a whole copy
    got = raw(Q, D[:4], 5, 64)
    assert [tuple(p) for p in got[0].tolist()] == [(0, 3, 50, 50), (0, 2, 40, 40), (0, 0, 10, 10)] and got[2].tolist() == [28]
    assert [tuple(p) for p in raw(Q, D[:4], 5, 2)[0].tolist()] == [(0, 3, 50, 50), (0, 2, 40, 40)]
    assert len(raw(Q, D, 128, 64)[0]) == 0
    D[4] = Q[0]
    assert [tuple(p) for p in raw(Q, D, 128, 64)[0].tolist()] == [(0, 4, 128, 128)]


@pytest.mark.parametrize("m", (256, 100))
def test_dwords_empty_buckets_and_empty_rows(m):
    rng = np.random.default_rng(m)
    Q = rng.integers(1, 1 << 62, (3, m)).astype(np.uint64)
    Q[1, ::3] = E                                                             # some buckets unfilled
    Q[2] = E                                                                  # an empty query
    D = np.stack([Q[0] ^ np.uint64(1 << 40), Q[0] ^ np.uint64(1), Q[0], Q[1], np.full(m, E), Q[0]])
    half = np.arange(m) % 2 == 0
    D[2, half] ^= np.uint64(1 << 63)                                          # equal in the low dword only, on half the buckets
    D[5, ~half] ^= np.uint64(2)                                               # equal in the high dword only, on the other half
    want = GM.gather(Q, D, 1, 8)
    assert [tuple(p) for p in want[0].tolist()] == [(0, 2, m // 2, m // 2), (0, 5, m // 2, m // 2), (1, 3, m - len(Q[1, ::3]), m - len(Q[1, ::3]))]
    assert want[2].tolist() == [0, 0, 0]
    same(raw(Q, D, 1, 8), want, "forged")
    same(via_context(Q, D, 1, 8), want, "forged, context")


def test_empty_sides_and_null_outputs():
    Q, D = forge(13, 65, 512, seed=9)
    want = GM.gather(Q, D, 2, 16)
    for null in ((0,), (1,), (2,), (0, 1, 2)):
        same(raw(Q, D, 2, 16, null), want, null)
    none = np.zeros((0, 512), dtype=np.uint64)
    same(raw(Q, none, 2, 16), GM.gather(Q, none, 2, 16), "n_d = 0")
    assert raw(Q, none, 2, 16)[2].tolist() == (Q != E).sum(axis=1).tolist()
    same(raw(none, D, 2, 16), GM.gather(none, D, 2, 16), "n_q = 0")


def test_context_call_leaves_the_context_alone_and_matches_the_matrix():
    Q, D = forge(13, 200, 512, seed=11)
    Q = np.where(Q == E, np.uint64(12345), Q)      # every query bucket filled: the matrix cell also counts buckets unfilled on both sides, M(d) never does
    want = GM.gather(Q, D, 3, 64)
    with Selector(0) as sel:
        with pytest.raises(pkg.SelhipError, match="no queries attached"):
            sel.upload(np.zeros((len(D), 1 << 14), np.uint8), D, np.arange(1.0, len(D) + 1))     # (a pass leaves genomes of cardinality 0 out)
            sel.gather()
        sel.upload_queries(np.zeros((len(Q), 1 << 14), np.uint8), Q, np.arange(1.0, len(Q) + 1))
        sel.set_criterion(CRIT_SMH_C)
        sel.set_min_matches(50)
        sel.set_estimator("smh")
        before = sel.run_queries(-1.0, MODE_SMH, 7, 3)
        state = (sel.result_count(), sel.stats())
        res = sel.gather(3, 64)
        same((res["picks"], res["n_picks"], res["unexplained"]), want, "context")
        assert (sel.result_count(), sel.stats()) == state and state[0] > 0
        assert sel.run_queries(-1.0, MODE_SMH, 7, 3).tobytes() == before.tobytes()
        cells = sel.query_matrix("smh_matches").cpu().numpy()
        assert np.array_equal(cells[res["picks"]["q"], res["picks"]["d"]], res["picks"]["matches"].astype(cells.dtype))
        with pytest.raises(pkg.SelhipError, match="c_min"):
            sel.gather(0)
    same(raw(Q, D, 3, 64), want, "context-free")


def test_command_line_writes_what_the_package_writes(monkeypatch, tmp_path):
    monkeypatch.chdir(GOLDEN)
    lst = "influenza_filelist.txt"
    want = pkg.gather_from_filelists(lst, lst, 512, 1, 8)
    assert want["table"].count("\n") == len(want["picks"]) >= len(want["query_names"])
    out = tmp_path / "out.tsv"
    run = subprocess.run([str(ROOT / "cuda_selection_criteria_amd" / "bin" / "selection"), "-l", lst, "-q", lst, "-a", "512", "-w", str(out), "-k", "8"], cwd=GOLDEN,
                         capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout == "", run
    assert out.read_text() == want["table"]
