"""Sketches merged by group on the device: selhip_merge_sketches against the numpy model (tests/merge_model.py) at
the smallest shapes at which its counting sort, its levels and its two row paths can go wrong; the context entry behind both
clusterings; the merged rows as the set of a second context; and the builder identity.  Every comparison is bit for bit.  The two
kernels that take a lane per member row (the count and the scatter of the counting sort) are grid-stride loops: the primitive and the
context entry also run with the process-wide hook "vertex_blocks" at 1 and 3 blocks, so that 335 rows take two trips and the 4 102
rows of test_three_levels seventeen and six."""
import ctypes as C

import numpy as np
import pytest
import torch

import merge_model as M
from test_exhaustive_host import flat_oracle_select

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import CRIT_NONE, CRIT_SMH_A, FP_FMA, MERGE_SEGMENT, MODE_CB_SMH, SelhipError, Selector, SynthConfig, hll_fold
from cuda_selection_criteria_amd._lib import Merged, check

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S = MERGE_SEGMENT
FILL = 0xEE
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
SIZES = (0, 1, 2, S - 1, S, S + 1, 2 * S + 3)          # one group of each size in one call
VERTEX_BLOCKS = (0, 1, 3)      # the row kernels' grid: sized from n, one block, three blocks


@pytest.fixture
def vertex_hook():
    """sets the process-wide grid of the kernels that take a lane per row (0 = automatic) and puts the default back"""
    with Selector(0) as sel:
        def set_hook(vertex_blocks):
            sel.set_param("vertex_blocks", vertex_blocks)
            assert sel.get_param("vertex_blocks") == vertex_blocks
        yield set_hook
        set_hook(0)
        sel.set_param("cluster_blocks", 0)


def edge_groups(seed, sizes=SIZES, loose=9):
    """ids interleaved in random order: group g has sizes[g] members, `loose` rows are in no group"""
    ids = np.concatenate([np.full(c, g, dtype=np.int32) for g, c in enumerate(sizes)] + [np.full(loose, -1, dtype=np.int32)])
    return np.random.default_rng(seed).permutation(ids), len(sizes)


def random_rows(seed, n, p=None, m=None, p_aux=None):
    """(hll, smh, aux): HLL bytes from the full range 0 .. 255, u64 buckets with ~0 and 0 among them; None where the width is None"""
    rng = np.random.default_rng(seed)
    hll = rng.integers(0, 256, (n, 1 << p), dtype=np.uint8) if p else None
    aux = rng.integers(0, 256, (n, 1 << p_aux), dtype=np.uint8) if p_aux else None
    smh = None
    if m:
        smh = rng.integers(0, 1 << 64, (n, m), dtype=np.uint64)
        smh[rng.random((n, m)) < 0.05] = U64_MAX
        smh[rng.random((n, m)) < 0.05] = 0
    return hll, smh, aux


def to_dev(a):
    if a is None:
        return None
    a = a.view(np.int64) if a.dtype == np.uint64 else a
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def filled(shape, dtype):
    """a device tensor of `shape` plus one spare row whose every BYTE is FILL (an empty output still has an address)"""
    item = torch.empty(0, dtype=dtype).element_size()
    cols = int(np.prod(shape[1:], dtype=np.int64)) if len(shape) > 1 else 1
    flat = torch.full(((shape[0] + 1) * cols * item,), FILL, dtype=torch.uint8, device=DEV).view(dtype)
    return flat.view(shape[0] + 1, cols) if len(shape) > 1 else flat


def raw_merge(d_hll, d_smh, d_aux, d_groups, n, G, stream=None):
    """selhip_merge_sketches over device tensors into FILL-ed outputs; returns (rc, outputs as numpy, one spare row included)"""
    lib = pkg.hip_lib()
    p = d_hll.shape[1].bit_length() - 1 if d_hll is not None else 14
    m = d_smh.shape[1] if d_smh is not None else 0
    p_aux = d_aux.shape[1].bit_length() - 1 if d_aux is not None else 0
    o_hll = filled((G, d_hll.shape[1]), torch.uint8) if d_hll is not None else None
    o_smh = filled((G, m), torch.int64) if d_smh is not None else None
    o_aux = filled((G, d_aux.shape[1]), torch.uint8) if d_aux is not None else None
    o_size = filled((G,), torch.int32)
    ptr = lambda t: t.data_ptr() if t is not None else None
    if stream is None:
        torch.cuda.synchronize()
    rc = lib.selhip_merge_sketches(ptr(d_hll), ptr(d_smh), ptr(d_aux), n, p, m, p_aux, ptr(d_groups), G, ptr(o_hll), ptr(o_smh), ptr(o_aux),
                                   ptr(o_size), C.c_void_p(stream.cuda_stream) if stream is not None else None)
    host = lambda t: None if t is None else t.cpu().numpy()
    out = {"hll": host(o_hll), "smh": None if o_smh is None else host(o_smh).view(np.uint64), "aux_hll": host(o_aux), "sizes": host(o_size).reshape(-1)}
    return rc, out


def assert_is_model(out, want, G, what=""):
    """the first G rows are the model's, and the spare row behind them kept its fill"""
    for key in ("hll", "smh", "aux_hll", "sizes"):
        assert (out[key] is None) == (want[key] is None), (what, key)
        if want[key] is None:
            continue
        got = out[key][:G]
        assert got.shape == want[key].shape, (what, key, got.shape, want[key].shape)
        assert np.array_equal(got, want[key]), (what, key, np.argwhere(got != want[key])[:4])
        assert (out[key][G:].view(np.uint8) == FILL).all(), (what, key, "wrote past its rows")


def check_primitive(seed, groups, G, p=None, m=None, p_aux=None, what="", hook=None):
    """hook: the vertex_hook fixture's setter -- the call then runs under every grid of VERTEX_BLOCKS"""
    n = len(groups)
    hll, smh, aux = random_rows(seed, n, p, m, p_aux)
    want = M.merge_all(hll, smh, aux, groups, G)
    rows = to_dev(hll), to_dev(smh), to_dev(aux), to_dev(groups) if n else torch.zeros(1, dtype=torch.int32, device=DEV)
    for blocks in VERTEX_BLOCKS if hook else (0,):
        if hook:
            hook(blocks)
        rc, out = raw_merge(*rows, n, G)
        assert rc == 0, (what, blocks, pkg.hip_lib().selhip_last_error(None).decode())
        assert_is_model(out, want, G, (what, blocks))
    return hll, smh, aux, want


# ---- 1. the primitive --------------------------------------------------------------------------------------------------------------
# (p, m, p_aux): all kinds together at every row shape, then each kind alone
SHAPES = [(4, 1, 4), (4, 3, 8), (14, 96, 4), (14, 512, 8), (4, 2048, 4), (14, None, None), (None, 96, None), (None, 3, None), (None, None, 8),
          (4, None, None)]


@pytest.mark.parametrize("p,m,p_aux", SHAPES)
def test_primitive_is_the_model(vertex_hook, p, m, p_aux):
    groups, G = edge_groups(17)
    assert list(M.sizes(groups, G)) == list(SIZES) and (groups == -1).sum() == 9
    hll, smh, aux, want = check_primitive(100 + 7 * (p or 0) + (m or 0) + 3 * (p_aux or 0), groups, G, p, m, p_aux, (p, m, p_aux), hook=vertex_hook)
    if hll is not None:
        assert not want["hll"][0].any() and np.array_equal(want["hll"][1], hll[groups == 1][0])      # empty: zeros; singleton: a copy
        assert p != 14 or (want["hll"][6] == 255).mean() > 0.3                                     # 131 random bytes: the maximum is often 255
    if smh is not None:
        assert (want["smh"][0] == U64_MAX).all() and np.array_equal(want["smh"][1], smh[groups == 1][0])


def test_primitive_p20():
    check_primitive(20, np.array([1, 0, 1], dtype=np.int32), 2, p=20, m=3, what="p = 20")


def test_primitive_every_byte_value():
    """the packed 16-bit maximum on the even and on the odd bytes is exact for all 256 x 256 pairs of byte values, in every byte lane"""
    a, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    rows = np.concatenate([np.roll(a.reshape(-1, 16), k, axis=1) for k in range(4)] + [np.roll(b.reshape(-1, 16), k, axis=1) for k in range(4)])
    half = len(rows) // 2
    groups = np.concatenate([np.arange(half), np.arange(half)]).astype(np.int32)
    want = M.merge(rows, groups, half, "max")
    assert np.array_equal(want, np.maximum(rows[:half], rows[half:]))
    rc, out = raw_merge(to_dev(rows), None, None, to_dev(groups), len(rows), half)
    assert rc == 0 and np.array_equal(out["hll"][:half], want)


def test_three_levels(vertex_hook):
    """one group of S^2 + 1 members: S + 1 partial rows, then 2, then the row (p = 4 and m = 2 keep it to a few hundred KiB)"""
    n = S * S + 1
    groups = np.zeros(n + 5, dtype=np.int32)
    groups[[3, 77, n // 2, n, n + 4]] = -1
    hll, smh, _, want = check_primitive(33, groups, 1, p=4, m=2, what="three levels", hook=vertex_hook)
    assert want["sizes"][0] == n
    # ... and beside other groups, ids interleaved: the partial rows of every group lie in group order
    groups = np.random.default_rng(5).permutation(np.concatenate([np.zeros(3, dtype=np.int32), np.full(n, 1, dtype=np.int32),
                                                                  np.full(S + 1, 3, dtype=np.int32), np.full(4, -1, dtype=np.int32)]))
    check_primitive(34, groups, 4, p=4, m=3, p_aux=4, what="three levels, four groups", hook=vertex_hook)


def test_empty_shapes():
    # n == 0 with G = 3: all-empty groups
    rc, out = raw_merge(torch.zeros((1, 16), dtype=torch.uint8, device=DEV), torch.zeros((1, 3), dtype=torch.int64, device=DEV), None, None, 0, 3)
    assert rc == 0
    assert not out["hll"][:3].any() and (out["smh"][:3] == U64_MAX).all() and not out["sizes"][:3].any()
    assert (out["hll"][3:] == FILL).all() and (out["smh"][3:].view(np.uint8) == FILL).all()
    # G == 0: nothing is written
    groups = np.full(7, -1, dtype=np.int32)
    hll, smh, _ = random_rows(1, 7, 4, 3)
    rc, out = raw_merge(to_dev(hll), to_dev(smh), None, to_dev(groups), 7, 0)
    assert rc == 0 and (out["hll"] == FILL).all() and (out["smh"].view(np.uint8) == FILL).all() and (out["sizes"].view(np.uint8) == FILL).all()
    # through the wrapper
    got = pkg.merge_sketches(np.zeros((0, 16), dtype=np.uint8), None, None, np.zeros(0, dtype=np.int32), 2)
    assert got["hll"].shape == (2, 16) and not got["hll"].any() and list(got["sizes"]) == [0, 0]


@pytest.mark.parametrize("bad,count,index", [({5: 7}, 1, 5), ({0: -2, 300: 7, 12: 1 << 30}, 3, None), ({334: -(1 << 31)}, 1, 334)])
def test_bad_id_writes_nothing(bad, count, index):
    groups, G = edge_groups(17)
    for at, value in bad.items():
        groups[at] = value
    hll, smh, aux = random_rows(2, len(groups), 4, 3, 4)
    rc, out = raw_merge(to_dev(hll), to_dev(smh), to_dev(aux), to_dev(groups), len(groups), G)
    msg = pkg.hip_lib().selhip_last_error(None).decode()
    assert rc == -1 and f"holds {count} invalid entries" in msg and f"outside [-1, {G})" in msg, msg
    named = int(msg.split("entry ")[1].split(" ")[0])
    assert named in bad and (index is None or named == index), msg
    for key in ("hll", "smh", "aux_hll", "sizes"):
        assert (out[key].view(np.uint8) == FILL).all(), key
    with pytest.raises(SelhipError, match="invalid entries"):
        pkg.merge_sketches(hll, smh, aux, groups, G)
    # G == 0 with a member: every id but -1 is invalid
    rc, _ = raw_merge(to_dev(hll), None, None, to_dev(np.zeros(len(groups), dtype=np.int32)), len(groups), 0)
    assert rc == -1 and f"holds {len(groups)} invalid entries" in pkg.hip_lib().selhip_last_error(None).decode()


def test_wrapper_and_host_twin_agree():
    groups, G = edge_groups(23)
    hll, smh, aux = random_rows(3, len(groups), 10, 5, 4)
    dev, host = pkg.merge_sketches(hll, smh, aux, groups, G), pkg.merge_sketches(hll, smh, aux, groups, G, device=None)
    want = M.merge_all(hll, smh, aux, groups, G)
    for key in want:
        assert np.array_equal(dev[key], want[key]) and np.array_equal(host[key], want[key]), key


def test_unaligned_buckets_take_the_plain_path():
    """an even m in an array that is only 8-byte aligned: legal, the 8-byte path"""
    groups, G = edge_groups(29)
    _, smh, _ = random_rows(4, len(groups), m=4)
    pad = torch.zeros(len(groups) * 4 + 1, dtype=torch.int64, device=DEV)
    d_smh = pad[1:].view(len(groups), 4)
    assert d_smh.data_ptr() % 16 == 8
    d_smh.copy_(to_dev(smh))
    rc, out = raw_merge(None, d_smh, None, to_dev(groups), len(groups), G)
    assert rc == 0 and np.array_equal(out["smh"][:G], M.merge(smh, groups, G, "min"))


# ---- 2. on a non-default stream, the inputs produced on it right before the call ----------------------------------------------------
def test_on_a_side_stream():
    groups, G = edge_groups(31)
    n = len(groups)
    side = torch.cuda.Stream(device=DEV)
    d_groups = to_dev(groups)
    base_hll, base_smh = torch.zeros((n, 1 << 14), dtype=torch.uint8, device=DEV), torch.zeros((n, 96), dtype=torch.int64, device=DEV)
    hll, smh, _ = random_rows(6, n, 14, 96)
    src_hll, src_smh = to_dev(hll), to_dev(smh)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        base_hll.copy_(src_hll, non_blocking=True)                 # the inputs are written on the side stream ...
        base_smh.copy_(src_smh, non_blocking=True)
        rc, out = raw_merge(base_hll, base_smh, None, d_groups, n, G, stream=side)       # ... and the merge is enqueued behind them
    assert rc == 0
    assert_is_model(out, M.merge_all(hll, smh, None, groups, G), G, "side stream")


# ---- 3. the context entry ------------------------------------------------------------------------------------------------------------
def snapshot(sel):
    return sel.fetch().tobytes(), sel.stats(), sel.last_attempts(), sel.result_count(), sel.get_param("clusters_last")


@pytest.fixture(scope="module")
def synth_set():
    cfg = SynthConfig("merge", 300, 256, 0.9, 0x5EED4E46, p_aux=8, mode=1, n_sh_lo=3_000, n_sh_hi=60_000)
    hll_t, aux_t, cards_t, _, ah_t = pkg.synth_device(cfg)
    return cfg, (hll_t, aux_t, cards_t, ah_t), (hll_t.cpu().numpy(), aux_t.cpu().numpy().view(np.uint64), ah_t.cpu().numpy())


def device_cards(rows_t):
    lib = pkg.hip_lib()
    ctx = C.c_void_p()
    check(lib.selhip_ctx_create(C.byref(ctx), 0))
    try:
        out = torch.empty(rows_t.shape[0], dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        check(lib.selhip_hll_cards(ctx, rows_t.data_ptr(), rows_t.shape[0], 14, out.data_ptr()), ctx)
    finally:
        lib.selhip_ctx_destroy(ctx)
    return out.cpu().numpy()


def assert_context_merge(sel, res, groups, G, hll, aux, aux_hll, what):
    got = {k: None if v is None else v.cpu().numpy() for k, v in res.items()}
    assert np.array_equal(got["hll"], M.merge(hll, groups, G, "max")), what
    assert np.array_equal(got["aux"].view(np.uint64), M.merge(aux, groups, G, "min")), what
    assert np.array_equal(got["sizes"], M.sizes(groups, G)), what
    if aux_hll is None:
        assert got["aux_hll"] is None, what
    else:
        assert np.array_equal(got["aux_hll"], M.merge(aux_hll, groups, G, "max")), what
    h = pkg.host_lib()
    host_cards = np.array([h.selhost_hll_report(np.ascontiguousarray(row).ctypes.data, 14, FP_FMA) for row in got["hll"]])
    assert np.array_equal(got["cards"].view(np.uint64), host_cards.view(np.uint64)), what
    assert np.array_equal(got["cards"].view(np.uint64), device_cards(res["hll"]).view(np.uint64)), what
    return got


@pytest.mark.parametrize("linkage", ["single", "greedy"])
def test_context_merge_behind_a_clustering(synth_set, vertex_hook, linkage):
    cfg, (hll_t, aux_t, cards_t, ah_t), (hll, aux, aux_hll) = synth_set
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        sel.attach(hll_t, aux_t, cards_t)
        sel.set_criterion(CRIT_SMH_A)
        rec = sel.run(cfg.tau, MODE_CB_SMH, r, b)
        assert len(rec) > 0
        res = sel.cluster_greedy() if linkage == "greedy" else sel.cluster()
        G = res["n_clusters"]
        assert 1 < G < cfg.n_genomes and res["sizes"].max() > 1
        before = snapshot(sel) + (sel.get_param("greedy_clusters_last"),)
        for blocks in VERTEX_BLOCKS[::-1]:                                              # (the default grid last: the calls below run under it)
            vertex_hook(blocks)
            merged = sel.merge(res)
            assert snapshot(sel) + (sel.get_param("greedy_clusters_last"),) == before      # list, statistics, attempts, "clusters_last": as they were
            got = assert_context_merge(sel, merged, res["clusters"], G, hll, aux, None, (linkage, blocks))
        assert np.array_equal(got["sizes"], res["sizes"])
        # a device tensor of ids, n_groups from the ids, host arrays out
        host = sel.merge(torch.from_numpy(res["clusters"]).to(DEV), to_host=True)
        assert all(np.array_equal(host[k], got[k].view(host[k].dtype)) for k in ("hll", "aux", "cards", "sizes"))
        # the auxiliary sketches: attached, then folded -- the fold of the merged main rows
        sel.attach_aux_hll(ah_t, 8)
        assert_context_merge(sel, sel.merge(res), res["clusters"], G, hll, aux, aux_hll, linkage + " aux attached")
        sel.fold_aux_hll(5)
        folded = sel.merge(res, to_host=True)
        assert np.array_equal(folded["aux_hll"], hll_fold(folded["hll"], 5)) and np.array_equal(folded["hll"], got["hll"])
        assert snapshot(sel) + (sel.get_param("greedy_clusters_last"),) == before


def test_context_groups_of_any_kind(synth_set, vertex_hook):
    """ids that are no clustering: empty groups, genomes in no group, a group longer than the segment"""
    cfg, (hll_t, aux_t, cards_t, _), (hll, aux, _) = synth_set
    n = cfg.n_genomes
    groups = np.random.default_rng(8).permutation(np.concatenate([np.full(S + 5, 2), np.full(3, 0), np.full(n - S - 8 - 10, 4), np.full(10, -1)])).astype(np.int32)
    with Selector(0) as sel:
        sel.attach(hll_t, aux_t, cards_t)
        for blocks in VERTEX_BLOCKS[::-1]:                                              # (the default grid last: the calls below run under it)
            vertex_hook(blocks)
            got = assert_context_merge(sel, sel.merge(groups, 6), groups, 6, hll, aux, None, ("any ids", blocks))
        assert list(got["sizes"][[1, 3, 5]]) == [0, 0, 0] and list(got["cards"][[1, 3, 5]]) == [0.0, 0.0, 0.0]
        with pytest.raises(SelhipError, match="invalid entries") as err:
            sel.merge(groups, 4)
        assert err.value.code == -1
        # NULL outputs: only the cardinalities (the registers go to scratch), only the sizes
        cards = torch.full((6,), -1.0, dtype=torch.float64, device=DEV)
        sizes = torch.full((6,), -1, dtype=torch.int32, device=DEV)
        d_groups = torch.from_numpy(groups).to(DEV)
        lib = pkg.hip_lib()
        check(lib.selhip_ctx_merge_groups(sel._ctx, d_groups.data_ptr(), 6, C.byref(Merged(None, None, None, cards.data_ptr(), None))), sel._ctx)
        assert np.array_equal(cards.cpu().numpy().view(np.uint64), got["cards"].view(np.uint64)) and (sizes == -1).all()
        check(lib.selhip_ctx_merge_groups(sel._ctx, d_groups.data_ptr(), 6, C.byref(Merged(None, None, None, None, sizes.data_ptr()))), sel._ctx)
        assert np.array_equal(sizes.cpu().numpy(), got["sizes"])


def test_context_state_rules(synth_set):
    cfg, (hll_t, aux_t, cards_t, ah_t), (hll, aux, _) = synth_set
    n = cfg.n_genomes
    r, b = pkg.banding(cfg.m, cfg.tau)
    groups = (np.arange(n) % 7).astype(np.int32)
    lib = pkg.hip_lib()
    with Selector(0) as sel:
        with pytest.raises(SelhipError, match="no sketches") as err:                      # before upload / attach
            sel.merge(np.zeros(0, dtype=np.int32), 1)
        assert err.value.code == -5
        sel.attach(hll_t, aux_t, cards_t)
        want = assert_context_merge(sel, sel.merge(groups, 7), groups, 7, hll, aux, None, "before any pass")
        # d_aux_hll without auxiliary sketches
        spare = torch.zeros((7, 256), dtype=torch.uint8, device=DEV)
        d_groups = torch.from_numpy(groups).to(DEV)
        rc = lib.selhip_ctx_merge_groups(sel._ctx, d_groups.data_ptr(), 7, C.byref(Merged(None, None, spare.data_ptr(), None, None)))
        assert rc == -5 and "auxiliary" in lib.selhip_last_error(sel._ctx).decode() and not spare.any()
        assert lib.selhip_ctx_merge_groups(sel._ctx, d_groups.data_ptr(), 7, None) == -1
        assert lib.selhip_ctx_merge_groups(sel._ctx, d_groups.data_ptr(), -1, C.byref(Merged())) == -1
        # while a pass is pending; it works after finish
        sel.run_async(cfg.tau, MODE_CB_SMH, r, b)
        with pytest.raises(SelhipError, match="pending") as err:
            sel.merge(groups, 7)
        assert err.value.code == -5
        sel.finish()
        same = lambda res: all(np.array_equal(res[k].cpu().numpy().view(np.uint8), want[k].view(np.uint8)) for k in ("hll", "aux", "cards", "sizes"))
        assert same(sel.merge(groups, 7))
        # behind a query pass: the database set is merged, and the query pass's list stays
        sel.upload_queries(hll[:5], aux[:5], cards_t.cpu().numpy()[:5])
        assert len(sel.run_queries(cfg.tau, MODE_CB_SMH, r, b)) > 0
        before = snapshot(sel)
        assert same(sel.merge(groups, 7)) and snapshot(sel) == before
        # timing: "merge" per merge call, the passes' figures untouched
        sel.timing(1)
        sel.run(cfg.tau, MODE_CB_SMH, r, b)
        names = ("prep", "stage1", "total", "hist", "select", "cluster", "greedy", "matrix")
        ms, launches = [sel.kernel_ms(k) for k in names], [sel.kernel_launches(k) for k in names]
        assert sel.kernel_ms("merge") < 0
        sel.merge(groups, 7)
        sel.merge(groups, 7)
        assert sel.kernel_ms("merge") > 0 and sel.kernel_launches("merge") == 1.0          # one timed scope per call, two calls
        assert [sel.kernel_ms(k) for k in names] == ms and [sel.kernel_launches(k) for k in names] == launches
        sel.timing(0)


# ---- 4. the round trip: the merged rows are a valid set ---------------------------------------------------------------------------
def test_merged_rows_as_a_second_context(oracle, synth_set):
    cfg, (hll_t, aux_t, cards_t, _), (hll, aux, _) = synth_set
    r, b = pkg.banding(cfg.m, cfg.tau)
    with Selector(0) as sel:
        sel.attach(hll_t, aux_t, cards_t)
        sel.run(cfg.tau, MODE_CB_SMH, r, b, fetch=False)
        res = sel.cluster()
        merged = sel.merge(res)
    G = res["n_clusters"]
    model_hll = M.merge(hll, res["clusters"], G, "max")
    model_cards = oracle.cards(model_hll)
    order_want = pkg.sort_by_card(model_cards)
    sel2, order = pkg.selector_from_rows(merged["hll"], merged["aux"], merged["cards"])
    with sel2:
        assert np.array_equal(order, order_want) and sel2.n == G and sel2.m == cfg.m
        assert np.array_equal(sel2.cards().view(np.uint64), model_cards[order_want].view(np.uint64))
        sel2.set_criterion(CRIT_NONE)
        for tau in (0.5, 0.05):
            got = sel2.run(tau, MODE_CB_SMH, 1, 1)
            want, _ = flat_oracle_select(oracle, model_hll[order_want], model_cards[order_want], tau, True, FP_FMA)
            assert len(want) > 0 or tau == 0.5
            assert np.array_equal(got["i"], want["i"]) and np.array_equal(got["k"], want["k"])
            assert np.array_equal(got["jaccard"].view(np.uint64), want["jaccard"].view(np.uint64))
        # the SuperMinHash rows too: an smh_a pass over the merged set against the same pass of the reference loop over the model's rows
        sel2.set_criterion(CRIT_SMH_A)
        model_aux = M.merge(aux, res["clusters"], G, "min")[order_want]
        got = sel2.run(0.3, MODE_CB_SMH, 2, cfg.m // 2)
        want, _ = oracle.select(model_hll[order_want], model_aux, model_cards[order_want], 0.3, 2, cfg.m // 2, use_cb=True, criterion=0)
        assert np.array_equal(got["i"], want["i"]) and np.array_equal(got["k"], want["k"])
        assert np.array_equal(got["jaccard"].view(np.uint64), want["jacc"].view(np.uint64))


# ---- 5. the builder identity on the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [8, 64])
def test_merge_of_two_built_sketches_is_the_built_union(m):
    from cuda_selection_criteria_amd.build import build_from_codes
    rng = np.random.default_rng(900 + m)
    a = rng.integers(0, 4, 400).astype(np.uint8)
    b = np.concatenate([a[:200], rng.integers(0, 4, 260).astype(np.uint8)])             # shares k-mers with a
    b[330] = 4                                                                         # a reset inside
    hll, smh, aux = build_from_codes([a, b, np.concatenate([a, [4], b]).astype(np.uint8)], m, 8)
    assert smh.shape == (3, m) and not np.array_equal(hll[0], hll[2]) and not np.array_equal(smh[1], smh[2])
    got = pkg.merge_sketches(hll[:2], smh[:2], aux[:2], np.zeros(2, dtype=np.int32), 1)
    assert np.array_equal(got["hll"][0], hll[2]) and np.array_equal(got["aux_hll"][0], aux[2])
    assert np.array_equal(got["smh"][0], smh[2]), np.argwhere(got["smh"][0] != smh[2])[:4]
