"""The entries of libselhip.so that take no context (include/selection_hip.h sections 3, 4, 4b; selhip_hll_cards takes one for its stream
alone), each as entry(S, stream) -> (what the device gave, what the models say) on the data of one stream_harness.Sets.  Used by
tests/test_threads_gpu.py, which runs them from three threads at once, and by tests/threads_child.py, the fresh process in which their
first calls meet.  A plain helper module like tests/*_model.py; needs torch and a GPU.

The caller runs an entry under torch.cuda.stream(stream): the inputs are copied, the outputs poisoned and read back on that stream, and
the library is handed the same stream.  Expected values are the ones tests/test_streams_gpu.py compares the same entries with
(stream_harness.Sets: the oracle, tests/*_model.py, numpy); nothing is compared with a second run of the code under test."""
import ctypes as C

import numpy as np

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import FP_FMA, PAIR_DTYPE
from cuda_selection_criteria_amd._lib import BuildInfo, check

import merge_model
import stream_harness as H

N_BLOCK = H.N_BLOCK
N_GROUPS = 9
SPLIT_CHUNK = 64                              # end positions per chunk of the split builder: every genome of Sets.build_codes is split


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype in (np.uint64, np.uint32):
        a = a.view(np.int64 if a.dtype == np.uint64 else np.int32)
    return torch.from_numpy(a).cuda()


def poisoned(shape, dtype):
    import torch
    return torch.full(shape, -7 if dtype in (torch.int32, torch.int64, torch.float64) else 0xA5, dtype=dtype, device="cuda")


def ptr(stream):
    return C.c_void_p(stream.cuda_stream)


def bare_set(name, seed, m=64, p_aux=8, tau=H.TAU):
    """a Sets that holds no sketches: what the generator and the builder entries need (synth_cfg, block_synth, build_codes, block_build)"""
    S = H.Sets.__new__(H.Sets)
    S.name, S.seed, S.m, S.p_aux, S.tau = name, seed, m, p_aux, tau
    return S


ENTRIES = {}


def entry(name):
    def register(fn):
        ENTRIES[name] = fn
        return fn
    return register


@entry("selhip_smh_a_pairs")
def _smh_a_pairs(S, st):
    import torch
    aux, pairs, out = dev(S.D.aux), dev(S.block_pairs), poisoned((N_BLOCK,), torch.uint8)
    check(pkg.hip_lib().selhip_smh_a_pairs(aux.data_ptr(), S.m, S.r, S.b, pairs.data_ptr(), N_BLOCK, out.data_ptr(), ptr(st)))
    return out.cpu().numpy(), S.block_flags


@entry("selhip_hll_union_hist")
def _union_hist(S, st):
    import torch
    hll, pairs, out = dev(S.D.hll), dev(S.block_pairs), poisoned((N_BLOCK, 64), torch.int32)
    check(pkg.hip_lib().selhip_hll_union_hist(hll.data_ptr(), 14, pairs.data_ptr(), N_BLOCK, out.data_ptr(), ptr(st)))
    return out.cpu().numpy().view(np.uint32), S.block_hist


@entry("selhip_hll_bitslice+union_hist_planes")
def _planes(S, st):
    import torch
    n = S.n_d
    hll, pairs = dev(S.D.hll), dev(S.block_pairs)
    planes, gmax, out = poisoned((n, 6, 512), torch.int32), poisoned((n,), torch.uint8), poisoned((N_BLOCK, 64), torch.int32)
    khi = C.c_int(0)
    lib = pkg.hip_lib()
    check(lib.selhip_hll_bitslice(hll.data_ptr(), n, planes.data_ptr(), gmax.data_ptr(), C.byref(khi), ptr(st)))
    check(lib.selhip_hll_union_hist_planes(planes.data_ptr(), gmax.data_ptr(), khi.value, pairs.data_ptr(), N_BLOCK, out.data_ptr(), ptr(st)))
    return out.cpu().numpy().view(np.uint32), S.block_hist


@entry("selhip_ertl_estimate")
def _estimate(S, st):
    import torch
    counts, out = dev(S.block_hist), poisoned((N_BLOCK,), torch.float64)
    check(pkg.hip_lib().selhip_ertl_estimate(counts.data_ptr(), N_BLOCK, 14, FP_FMA, out.data_ptr(), ptr(st)))
    return out.cpu().numpy(), S.block_estimates


@entry("selhip_smh_match_counts")
def _matches(S, st):
    import torch
    aux, pairs, out = dev(S.D.aux), dev(S.block_pairs), poisoned((N_BLOCK,), torch.int32)
    check(pkg.hip_lib().selhip_smh_match_counts(aux.data_ptr(), S.m, pairs.data_ptr(), N_BLOCK, out.data_ptr(), ptr(st)))
    return out.cpu().numpy(), S.block_matches


@entry("selhip_hll_fold")
def _fold(S, st):
    import torch
    hll, out = dev(S.D.hll[:64]), poisoned((64, 1 << S.p_aux), torch.uint8)
    check(pkg.hip_lib().selhip_hll_fold(hll.data_ptr(), 64, 14, S.p_aux, out.data_ptr(), ptr(st)))
    return out.cpu().numpy(), S.block_fold


@entry("selhip_hll_cards")
def _cards(S, st):
    """report() of every genome on the device; the context is there for its stream (made and destroyed around the call)"""
    import torch
    hll, out = dev(S.D.hll), poisoned((S.n_d,), torch.float64)
    with pkg.Selector(0, stream=st.cuda_stream) as sel:
        check(sel._lib.selhip_hll_cards(sel._ctx, hll.data_ptr(), S.n_d, 14, out.data_ptr()), sel._ctx)
        got = out.cpu().numpy()
    return got, S.D.cards


@entry("selhip_permute_rows")
def _permute(S, st):
    import torch
    src, perm, out = dev(S.D.aux), dev(S.perm), poisoned((S.n_d, S.m), torch.int64)
    check(pkg.hip_lib().selhip_permute_rows(src.data_ptr(), out.data_ptr(), perm.data_ptr(), S.n_d, S.m * 8, ptr(st)))
    return out.cpu().numpy().view(np.uint64), S.block_permute


@entry("selhip_synth_generate")
def _synth(S, st):
    import torch
    n = S.synth_cfg.n_genomes
    hll, aux = poisoned((n, 1 << 14), torch.uint8), poisoned((n, S.m), torch.int64)
    aux_hll = poisoned((n, 1 << S.p_aux), torch.uint8)
    sp = S.synth_cfg.struct()
    check(pkg.hip_lib().selhip_synth_generate(C.byref(sp), 0, n, hll.data_ptr(), aux.data_ptr(), aux_hll.data_ptr(), ptr(st)))
    return {"hll": hll.cpu().numpy(), "aux": aux.cpu().numpy().view(np.uint64), "aux_hll": aux_hll.cpu().numpy()}, S.block_synth


def _build_outputs(S, n):
    import torch
    return poisoned((n, 1 << 14), torch.uint8), poisoned((n, 64), torch.int64), poisoned((n, 1 << S.p_aux), torch.uint8)


def _build_rows(hll, smh, aux_hll):
    return {"hll": hll.cpu().numpy(), "smh": smh.cpu().numpy().view(np.uint64), "aux_hll": aux_hll.cpu().numpy()}


@entry("selhip_build_sketches")
def _build(S, st):
    codes, off = dev(S.build_codes[0]), dev(S.build_codes[1])
    n = len(S.build_codes[1]) - 1
    hll, smh, aux_hll = _build_outputs(S, n)
    check(pkg.hip_lib().selhip_build_sketches(codes.data_ptr(), off.data_ptr(), n, 31, 64, S.p_aux, hll.data_ptr(), smh.data_ptr(), aux_hll.data_ptr(), ptr(st)))
    return _build_rows(hll, smh, aux_hll), S.block_build


@entry("selhip_build_sketches_split")
def _build_split(S, st):
    """the same genomes, every one cut into chunks of 64 end positions: the same rows, byte for byte"""
    codes, off = dev(S.build_codes[0]), dev(S.build_codes[1])
    n = len(S.build_codes[1]) - 1
    hll, smh, aux_hll = _build_outputs(S, n)
    info = BuildInfo()
    check(pkg.hip_lib().selhip_build_sketches_split(codes.data_ptr(), off.data_ptr(), None, n, 31, 64, S.p_aux, SPLIT_CHUNK, hll.data_ptr(),
                                                    smh.data_ptr(), aux_hll.data_ptr(), C.byref(info), ptr(st)))
    assert info.split_genomes == n and info.fallback_genomes == 0, (info.split_genomes, info.fallback_genomes)
    return _build_rows(hll, smh, aux_hll), S.block_build


@entry("selhip_components")
def _components(S, st):
    return pkg.components(dev(S.edges), S.n_d), S.components                     # (the helper takes torch's current stream)


@entry("selhip_greedy_representatives")
def _greedy(S, st):
    is_rep, rounds = pkg.greedy_representatives(dev(S.edges), S.n_d, keys=S.keys)
    assert rounds >= 1
    return is_rep, S.greedy_reps


@entry("selhip_spanning_forest")
def _forest(S, st):
    res = pkg.spanning_forest(dev(S.edges), S.n_d, values=S.forest_values)
    want = S.block_forest
    assert res["edges"].dtype == PAIR_DTYPE and res["n_edges"] == len(want["edges"])
    return {"edges": res["edges"], "labels": res["labels"]}, want


@entry("selhip_linkage")
def _linkage(S, st):
    """average linkage of the set's own matrix (Sets.linkage_dist) in both layouts of stream_harness.LINKAGE_LAYOUTS: per-call scratch,
    and a host loop that launches round after round from words it reads back, beside the other threads' calls"""
    import torch
    n = S.linkage_dist.shape[0]
    src, got = dev(S.linkage_dist), {}
    for tag, (ld_extra, offset) in H.LINKAGE_LAYOUTS.items():
        ld = n + ld_extra
        buf = torch.full((n * ld + 2 + offset,), float("nan"), dtype=torch.float64, device="cuda")
        view = buf[offset:offset + n * ld].view(n, ld)
        assert (ld % 2 == 0 and view.data_ptr() % 16 == 0) == (tag == "wide")
        view[:, :n].copy_(src)
        merges, sizes = poisoned((n - 1, PAIR_DTYPE.itemsize), torch.uint8), poisoned((n - 1,), torch.int32)
        f, rounds = C.c_int64(-5), C.c_int64(-5)
        check(pkg.hip_lib().selhip_linkage(view.data_ptr(), n, ld, pkg.LINKAGE_AVERAGE, float("inf"), merges.data_ptr(), sizes.data_ptr(),
                                           C.byref(f), C.byref(rounds), ptr(st)))
        m, s = merges.cpu().numpy(), sizes.cpu().numpy()
        assert 0 <= f.value <= n - 1 and np.all(m[f.value:] == 0xA5) and np.all(s[f.value:] == -7), (tag, f.value)
        got.update({f"merges-{tag}": np.ascontiguousarray(m[:f.value]).reshape(-1).view(PAIR_DTYPE), f"sizes-{tag}": s[:f.value],
                    f"rounds-{tag}": rounds.value})
    return got, S.block_linkage


def merge_groups(S):
    return np.random.default_rng(S.seed + 9).integers(-1, N_GROUPS, S.n_d).astype(np.int32)


@entry("selhip_merge_sketches")
def _merge(S, st):
    D, groups = S.D, merge_groups(S)
    got = pkg.merge_sketches(D.hll, D.aux, D.aux_hll, groups, N_GROUPS)
    return got, merge_model.merge_all(D.hll, D.aux, D.aux_hll, groups, N_GROUPS)


# the entries whose first call in a process goes through a std::call_once (csrc/abi_blocks.inc: selhip_synth_generate,
# selhip_build_sketches; csrc/host_build.hpp: the split builder's main launch)
CALL_ONCE = ("selhip_synth_generate", "selhip_build_sketches", "selhip_build_sketches_split")
# what three threads of a fresh process call first (tests/threads_child.py): those, and selhip_linkage, whose first call loads its seven
# kernels and takes its scratch while the other threads do the same
FIRST_CALLS = CALL_ONCE + ("selhip_linkage",)
