"""Sketch construction on the GPU: the `build_sketch` step of the reference (src/build_sketch.cpp) behind
selhip_build_sketches and selhip_build_sketches_split (include/selection_hip.h section 4b).  FASTA parsing happens in
libselhost (C++)."""
from __future__ import annotations

from typing import Sequence

import numpy as np

import ctypes as C

from ._lib import SPLIT_AUTO, SPLIT_OFF, BuildInfo, check, hip_lib, host_lib


def fasta_codes(path: str) -> np.ndarray:
    """one byte per base: 0..3 = A,C,G,T (either case), 4 = k-mer window reset (other character / record start)"""
    h = host_lib()
    n = h.selhost_fasta_codes(str(path).encode(), None, 0)
    if n < 0:
        raise RuntimeError(h.selhost_last_error().decode())
    out = np.empty(max(n, 1), dtype=np.uint8)
    h.selhost_fasta_codes(str(path).encode(), out.ctypes.data, n)
    return out[:n]


def smh_vecsize(m_arg: int) -> int:
    return int(host_lib().selhost_smh_vecsize(m_arg))


def split_chunk(split) -> int:
    """the chunk argument of selhip_build_sketches_split for split = "auto" | "off" | end positions per chunk"""
    if split == "auto":
        return SPLIT_AUTO
    if split == "off":
        return SPLIT_OFF
    if isinstance(split, (int, np.integer)) and not isinstance(split, bool) and split > 0:
        return int(split)
    raise ValueError(f'split must be None, "auto", "off" or a positive number of end positions per chunk, not {split!r}')


def split_plan(lengths: Sequence[int], k: int = 31, m: int = 0, p_aux: int = 0, split="auto", resident_blocks: int = 512):
    """the plan selhip_build_sketches_split makes for genomes of these lengths (plain arithmetic, no device):
    (info dict, chunks per genome).  m: the rounded bucket count, 0 without SuperMinHash rows"""
    n = len(lengths)
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.asarray(lengths, dtype=np.int64))
    counts = np.zeros(max(n, 1), dtype=np.int64)
    info = BuildInfo()
    check(hip_lib().selhip_build_split_plan(offsets.ctypes.data, n, k, m, p_aux, split_chunk(split), resident_blocks,
                                            counts.ctypes.data, C.byref(info)))
    return info_dict(info), counts[:n]


def info_dict(info: BuildInfo) -> dict:
    return {name: int(getattr(info, name)) for name, _ in BuildInfo._fields_}


def build_from_codes(codes_list: Sequence[np.ndarray], m: int = 0, p_aux: int = 0, k: int = 31, device: int = 0, split=None,
                     info: bool = False):
    """codes_list: one uint8 array per genome, 0..3 = A,C,G,T, 4 = k-mer window reset.  One selhip_build_sketches call, or with
    split = "auto" | "off" | end positions per chunk one selhip_build_sketches_split call (long genomes cut across workgroups: the
    same bytes).  returns (hll u8 [n,16384], smh u64 [n, vecsize(m)] or None, aux u8 [n, 1<<p_aux] or None) as numpy arrays; info=True
    (with split): a fourth element, the selhip_build_info_t of the call as a dict"""
    import torch

    if info and split is None:
        raise ValueError("info=True needs split: selhip_build_sketches reports nothing")
    chunk = None if split is None else split_chunk(split)

    lib = hip_lib()
    codes = [np.ascontiguousarray(c, dtype=np.uint8).reshape(-1) for c in codes_list]
    n = len(codes)
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(c) for c in codes], dtype=np.int64)
    flat = np.concatenate(codes) if n else np.zeros(0, dtype=np.uint8)
    dev = torch.device("cuda", device)
    mv = smh_vecsize(m) if m else 0
    with torch.cuda.device(dev):
        d_codes = torch.from_numpy(flat if flat.size else np.zeros(1, dtype=np.uint8)).to(dev)
        d_off = torch.from_numpy(offsets).to(dev)
        d_hll = torch.zeros((n, 16384), dtype=torch.uint8, device=dev)
        d_smh = torch.zeros((n, mv), dtype=torch.int64, device=dev) if mv else None
        d_aux = torch.zeros((n, 1 << p_aux), dtype=torch.uint8, device=dev) if p_aux else None
        torch.cuda.synchronize(dev)
        binfo = BuildInfo()
        if chunk is None:
            check(lib.selhip_build_sketches(d_codes.data_ptr(), d_off.data_ptr(), n, k, mv, p_aux, d_hll.data_ptr(),
                                            d_smh.data_ptr() if mv else None, d_aux.data_ptr() if p_aux else None, None))
        else:
            check(lib.selhip_build_sketches_split(d_codes.data_ptr(), d_off.data_ptr(), offsets.ctypes.data, n, k, mv, p_aux, chunk,
                                                  d_hll.data_ptr(), d_smh.data_ptr() if mv else None,
                                                  d_aux.data_ptr() if p_aux else None, C.byref(binfo), None))
        check(lib.selhip_device_synchronize())
        out = (d_hll.cpu().numpy(), d_smh.cpu().numpy().view(np.uint64) if mv else None,
               d_aux.cpu().numpy() if p_aux else None)
        return out + (info_dict(binfo),) if info else out


def build_sketches(fasta_paths: Sequence[str], m: int = 0, p_aux: int = 0, device: int = 0, k: int = 31, split=None, info: bool = False):
    """FASTA(.gz) files -> codes -> build_from_codes; same triple (and the info dict with info=True)"""
    return build_from_codes([fasta_codes(p) for p in fasta_paths], m, p_aux, k, device, split, info)
