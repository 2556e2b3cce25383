"""The drop-in launchers (include/selection_hip.h section 1; csrc/abi_compat.inc) on explicit lists that are not the canonical triangle
of a few hundred thousand pairs: lists longer than one internal chunk of 2^20 entries (the second chunk's `pairs + off`, the reset of
its survivor counter, *out_count accumulating), the static workspace across calls with longer and shorter lists, entries in either
orientation, repeated, with x == y, with an empty sketch on either side, cards that do not ascend -- and the launcher form of
pairs_direct_kernel, an instantiation of its own, at band shapes that straddle its 16-bucket steps.

All four launchers run in every group.  Expected records come from launcher_model.py (held to the oracle by
test_launcher_model_host.py); records are compared as multisets of (x, y, float32 bits), no tolerance.  The explicit-list form is
asynchronous on the null stream: every read follows a synchronize.  No out-of-range rank is ever passed: by contract the launchers
check none."""
import numpy as np
import pytest

import cuda_selection_criteria_amd as pkg
import launcher_model as LM
import pairlist_scale_model as PS
import precision_model as pm
from pairlist_scale_model import CHUNK, P_HLL, RB, TAU_CB, TOTAL
from test_pairlist_gpu import ODD_SHAPES

from cuda_selection_criteria_amd import ALGO_STREAM, FP_FMA, MODE_SMH, Selector

pytestmark = pytest.mark.gpu

# name, CB, bits of *out_count
LAUNCHERS = [("launch_kernel_smh", False, 32), ("launch_kernel_CBsmh", True, 32), ("launch_kernel_smh64", False, 64), ("launch_kernel_CBsmh64", True, 64)]
TAU_OF = {False: -1.0, True: TAU_CB}          # the long lists: every entry with an equal band is a record of smh; CBsmh takes a real tau
SENTINEL = -7
_DEV = {}


class Device:
    """a sketch set on the device, an output array of `cap` records filled with SENTINEL, and both counters"""

    def __init__(self, hll, aux, cards, cap):
        import torch
        dev = torch.device("cuda", 0)
        self.torch = torch
        self.hll = torch.from_numpy(np.array(hll)).to(dev)                     # (copies: the shared sets are read-only arrays)
        self.aux = torch.from_numpy(np.array(aux).view(np.int64)).to(dev)
        self.cards = torch.from_numpy(np.array(cards)).to(dev)
        self.m, self.m_hll = aux.shape[1], hll.shape[1]
        self.out = torch.full((cap, 3), SENTINEL, dtype=torch.int32, device=dev)
        self.cnt = {32: torch.full((1,), -1, dtype=torch.int32, device=dev), 64: torch.full((1,), -1, dtype=torch.int64, device=dev)}

    def launch(self, name, bits, d_pairs, total, tau, r, nb):
        """one call; (records sorted as a multiset, count) after a synchronize; the rest of `out` must still hold SENTINEL"""
        lib = pkg.hip_lib()
        self.out.fill_(SENTINEL)
        self.cnt[bits].fill_(-1)
        assert total <= self.out.shape[0]
        rc = getattr(lib, name)(self.hll.data_ptr(), self.aux.data_ptr(), self.cards.data_ptr(), d_pairs.data_ptr(), total,
                                float(np.float32(tau)), self.m, self.m_hll, r, nb, self.out.data_ptr(), self.cnt[bits].data_ptr(), 256)
        assert rc == 0, lib.selhip_last_error(None)
        self.torch.cuda.synchronize()
        cnt = int(self.cnt[bits].item())
        assert 0 <= cnt <= total, cnt
        assert bool((self.out[cnt:] == SENTINEL).all())                       # nothing written behind the records
        return LM.sort_records(self.out[:cnt].cpu().numpy()), cnt


def scale_device(Sc):
    import torch
    if "scale" not in _DEV:
        _DEV["scale"] = (Device(Sc.hll, Sc.aux, Sc.cards, TOTAL), torch.from_numpy(Sc.L).to("cuda"))
    return _DEV["scale"]


def scale_expected(Sc, off, length, use_cb):
    sl = slice(off, off + length)
    return LM.expected(Sc.oracle, Sc.cards, Sc.L[sl], TAU_OF[use_cb], use_cb, Sc.lit[sl], Sc.J[sl])


def chunks_of(total):
    """(offset, length) of the launcher's chunks"""
    step = min(total, CHUNK)
    return [(off, min(step, total - off)) for off in range(0, total, step)]


# ---- 1. the chunk loop ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 37, TOTAL], ids=["2^20-1", "2^20", "2^20+1", "2^20+37", "whole"])
def test_chunk_loop(oracle, P):
    Sc = PS.scale(oracle)
    dv, d_L = scale_device(Sc)
    chunks = chunks_of(P)
    assert len(chunks) == (2 if P > CHUNK else 1)
    # the groups per wave of every chunk: the rule, confirmed by a context pass over the chunk's own entries
    with Selector(0, FP_FMA) as sel:
        sel.upload(Sc.hll, Sc.aux, Sc.cards, p_hll=P_HLL)
        for off, length in chunks:
            sel.run_pairs(d_L[off:off + length], -1.0, MODE_SMH, *RB, algo=ALGO_STREAM, fetch=False)
            assert (sel.get_param("pairs_gpw"), sel.get_param("pairs_grid")) == PS.direct_shape(length)
    print(f"launchers: P={P} chunks={[(off, length, PS.direct_shape(length)) for off, length in chunks]}")
    want = {cb: scale_expected(Sc, 0, P, cb) for cb in (False, True)}
    per_chunk = {cb: [len(scale_expected(Sc, off, length, cb)) for off, length in chunks] for cb in (False, True)}
    for name, use_cb, bits in LAUNCHERS:
        got, cnt = dv.launch(name, bits, d_L, P, TAU_OF[use_cb], *RB)
        print(f"  {name}: {cnt} records, by chunk {per_chunk[use_cb]}")
        assert cnt == len(want[use_cb]) == sum(per_chunk[use_cb]) and cnt > 0
        if len(chunks) == 2 and P > CHUNK + 37:
            assert per_chunk[use_cb][1] > 0                                    # the second chunk contributes records
        assert np.array_equal(got, want[use_cb])


def test_second_chunk_of_one_entry_is_a_record(oracle):
    """2^20 + 1 entries whose last entry -- the whole second chunk -- has a record under both launchers: a list shifted so that it ends on one"""
    Sc = PS.scale(oracle)
    dv, d_L = scale_device(Sc)
    hit = np.nonzero(Sc.lit & (Sc.J >= TAU_CB) & (np.arange(TOTAL) >= CHUNK))[0]
    end = int(hit[0])
    off = end - CHUNK                                                         # the list is entries [off, end]: the second chunk is entry `end`
    assert off >= 0 and end < TOTAL
    for name, use_cb, bits in LAUNCHERS:
        want = scale_expected(Sc, off, CHUNK + 1, use_cb)
        last = scale_expected(Sc, end, 1, use_cb)
        assert len(last) == 1
        got, cnt = dv.launch(name, bits, d_L[off:], CHUNK + 1, TAU_OF[use_cb], *RB)
        assert cnt == len(want) and np.array_equal(got, want)
        assert bool((got == last[0]).all(axis=1).any())


# ---- 2. the static workspace across calls ----------------------------------------------------------------------------------------------
def test_workspace_reuse(oracle):
    """one process, in order: the whole list (the workspace grows to a chunk), 5 entries, 70 001 entries, an empty list"""
    Sc = PS.scale(oracle)
    dv, d_L = scale_device(Sc)
    for name, use_cb, bits in LAUNCHERS:
        for P in (TOTAL, 5, 70001, 0):
            want = scale_expected(Sc, 0, P, use_cb)
            got, cnt = dv.launch(name, bits, d_L, P, TAU_OF[use_cb], *RB)
            print(f"  {name}: P={P} {cnt} records")
            assert cnt == len(want), (name, P)
            assert np.array_equal(got, want), (name, P)
            if P == 0:
                assert cnt == 0 and bool((dv.out == SENTINEL).all())          # *out_count == 0 and `out` untouched
            if P == 70001:
                assert cnt > 0
    # five entries that do have records, after the long calls
    hit = np.nonzero(Sc.lit & (Sc.J >= TAU_CB))[0]
    start = int(hit[hit < TOTAL - 5][100])
    for name, use_cb, bits in LAUNCHERS:
        want = scale_expected(Sc, start, 5, use_cb)
        got, cnt = dv.launch(name, bits, d_L[start:], 5, TAU_OF[use_cb], *RB)
        assert cnt == len(want) >= 1 and np.array_equal(got, want)


# ---- 3. lists that are not the triangle -------------------------------------------------------------------------------------------------
def test_not_the_triangle(oracle):
    import torch
    hll, aux, cards, empty, twin = LM.awkward_set(oracle, P_HLL)
    n = len(cards)
    L = LM.awkward_list(n, empty)
    assert 2000 < len(L) < 10000
    eq, J = LM.per_entry(oracle, hll, aux, cards, L, *pm.RB, p=P_HLL)
    dv = Device(hll, aux, cards, len(L))
    d_L = torch.from_numpy(L).to("cuda")
    # the same genomes in ascending-card order, the list renamed: the launchers must not care about the order of `cards`
    order = np.argsort(cards, kind="stable")
    rank_of = np.empty(n, dtype=np.int32)
    rank_of[order] = np.arange(n, dtype=np.int32)
    dv_sorted = Device(hll[order], aux[order], cards[order], len(L))
    d_L_sorted = torch.from_numpy(np.ascontiguousarray(rank_of[L])).to("cuda")
    assert np.all(np.diff(cards[order]) >= 0) and np.any(np.diff(cards) < 0)
    for tau in (0.5, -1.0):
        for name, use_cb, bits in LAUNCHERS:
            want = LM.expected(oracle, cards, L, tau, use_cb, eq, J)
            got, cnt = dv.launch(name, bits, d_L, len(L), tau, *pm.RB)
            print(f"  {name} tau={tau}: {cnt} records of {len(L)} entries; x == y {int((want[:, 0] == want[:, 1]).sum())}, "
                  f"reversed {int((want[:, 0] > want[:, 1]).sum())}, with the empty sketch {int((want[:, 0] == empty).sum())}")
            assert cnt == len(want) > 0
            assert np.array_equal(got, want), (name, tau)
            assert (want[:, 0] == want[:, 1]).any() and (want[:, 0] > want[:, 1]).any() and not (want[:, 1] == empty).any()
            assert len(np.unique(want, axis=0)) < len(want)                   # repeated entries: repeated records
            assert bool((want[:, 0] == empty).any()) == (tau < 0)
            got_sorted, _ = dv_sorted.launch(name, bits, d_L_sorted, len(L), tau, *pm.RB)
            back = got_sorted.copy()
            back[:, :2] = order[got_sorted[:, :2]]
            assert np.array_equal(LM.sort_records(back), want), (name, tau, "ascending cards")


# ---- 4. the launcher form at the odd band shapes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,r,nb", ODD_SHAPES, ids=[f"{r}x{nb}" for _, r, nb in ODD_SHAPES])
def test_launcher_form_any_band_shape(oracle, m, r, nb):
    import torch
    n = 60
    hll, _, cards = pm.sketch_set(P_HLL, n, 8, 4242)
    rng = np.random.default_rng(m * 1000 + r)
    aux = rng.integers(0, 1 << 64, size=(n, m), dtype=np.uint64)
    straddling = [b for b in range(nb) if (b * r) // 16 != (b * r + r - 1) // 16]
    plant = {"first": 0, "last": nb - 1}
    if straddling:
        plant["straddle"] = straddling[len(straddling) // 2]
    planted, near = [], []
    for g, band in zip(range(0, 4 * len(plant), 4), plant.values()):
        aux[g + 1, band * r:(band + 1) * r] = aux[g, band * r:(band + 1) * r]
        planted.append((g, g + 1))
        aux[g + 3, band * r:(band + 1) * r - 1] = aux[g + 2, band * r:(band + 1) * r - 1]      # equal in all but its last bucket
        near.append((g + 2, g + 3))
    ii, kk = np.triu_indices(n, 1)
    L = np.stack([ii, kk], axis=1).astype(np.int32)
    flip = rng.random(len(L)) < 0.5
    L[flip] = L[flip][:, ::-1]
    L = np.ascontiguousarray(L[rng.permutation(len(L))])
    eq, J = LM.per_entry(oracle, hll, aux, cards, L, r, nb, p=P_HLL)
    assert int(eq.sum()) == len(plant)                                        # (random buckets: nothing else is equal, the near pairs least of all)
    dv = Device(hll, aux, cards, len(L))
    d_L = torch.from_numpy(L).to("cuda")
    for name, use_cb, bits in LAUNCHERS:
        tau = -1.0
        want = LM.expected(oracle, cards, L, tau, use_cb, eq, J)
        got, cnt = dv.launch(name, bits, d_L, len(L), tau, r, nb)
        assert cnt == len(want) == int(eq.sum())
        assert np.array_equal(got, want), name
        listed = {(min(x, y), max(x, y)) for x, y in got[:, :2].tolist()}
        assert set(planted) <= listed and (r == 1 or not set(near) & listed)
