"""The plan of the split sketch builder without a GPU: selhip_build_split_plan (csrc/host_plan.hpp: split_plan) against the model in
build_split_model.py, the exact-cover property of its work items, the auto rule's two promises (nothing under 65 536 end positions is
cut; the partial rows fit the scratch cap), the refusals, the declarations and the option of the build_sketch program."""
import ctypes as C
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import build_split_model as model
import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import _lib
from cuda_selection_criteria_amd.build import split_chunk, split_plan

LIBDIR = ROOT / "cuda_selection_criteria_amd" / "lib"
BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
BADARG, NOMEM = -1, -6


def lib_plan(lengths, k, m, p_aux, chunk, resident):
    """(status, info dict, counts) of selhip_build_split_plan; the counts array is pre-filled so that a write shows"""
    n = len(lengths)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum(np.asarray(lengths, dtype=np.int64))
    counts = np.full(max(n, 1), -7, dtype=np.int64)
    info = _lib.BuildInfo()
    rc = pkg.hip_lib().selhip_build_split_plan(off.ctypes.data, n, k, m, p_aux, chunk, resident, counts.ctypes.data, C.byref(info))
    return rc, {name: int(getattr(info, name)) for name, _ in _lib.BuildInfo._fields_}, [int(c) for c in counts[:n]]


def edge_lengths(k, chunk):
    return [0, k - 1, k, chunk + k - 2, chunk + k - 1, chunk + k]


def test_plan_matches_the_model():
    rng = random.Random(2501)
    cases = 0
    for k in (1, 16, 31, 32):
        for chunk in (64, 128, 4096, 65536, model.AUTO, model.OFF):
            c_edge = chunk if chunk > 0 else model.CHUNK_MIN
            for trial in range(6):
                lengths = edge_lengths(k, c_edge) + [rng.randrange(0, 5 * c_edge) for _ in range(rng.randrange(0, 12))]
                rng.shuffle(lengths)
                if trial == 0:
                    lengths = []
                m, p_aux = rng.choice([(0, 0), (8, 5), (64, 8), (512, 12)])
                resident = rng.choice([1, 7, 256, 512])
                rc, info, counts = lib_plan(lengths, k, m, p_aux, chunk, resident)
                want_info, want_counts = model.plan(lengths, k, m, p_aux, chunk, resident)
                assert rc == 0 and info == want_info and counts == want_counts, (k, chunk, lengths, info, want_info)
                cases += 1
    assert cases == 4 * 6 * 6


def test_edge_lengths_by_hand():
    """L = 0, k-1, k: one chunk; C + k-2 and C + k-1 end positions' worth: still one (C - 1 and C end positions); C + k: two"""
    k, chunk = 31, 128
    rc, info, counts = lib_plan(edge_lengths(k, chunk), k, 64, 0, chunk, 256)
    assert rc == 0 and counts == [1, 1, 1, 1, 1, 2]
    assert info == dict(chunk=128, items=7, split_genomes=1, chunks=2, fallback_genomes=0, levels=1, threads=1024)
    assert [model.levels_of(c) for c in (0, 1, 2, 64, 65, 4096, 4097)] == [0, 0, 1, 1, 2, 2, 3]
    rc, info, _ = lib_plan([64 * 65 + 30, 90], k, 0, 0, 64, 1)
    assert rc == 0 and info["levels"] == 2 and info["chunks"] == 65
    rc, info, _ = lib_plan([90] * 2046 + [200], k, 0, 0, 64, 1)          # 2 046 direct + 3 partial: 2 049 items
    assert rc == 0 and (info["items"], info["threads"]) == (2049, 256)


def test_every_end_position_in_exactly_one_item():
    rng = random.Random(2502)
    for k, chunk in ((31, 64), (31, 128), (1, 64), (32, 192), (16, 4096)):
        lengths = edge_lengths(k, chunk) + [rng.randrange(0, 6 * chunk) for _ in range(10)]
        rc, info, counts = lib_plan(lengths, k, 0, 0, chunk, 256)
        assert rc == 0
        items = model.items(lengths, k, info["chunk"], counts)
        assert len(items) == info["items"]
        seen = [np.zeros(L, dtype=np.int32) for L in lengths]
        for it in items:
            start, length, g, kind = it
            assert 0 <= start and start + length <= lengths[g], it                 # the sub-array lies inside the genome
            for e in model.item_end_positions(it, k):
                seen[g][e] += 1
        for g, L in enumerate(lengths):
            assert (seen[g][:k - 1] == 0).all() and (seen[g][k - 1:] == 1).all(), (k, chunk, L)
        partial = [it for it in items if it[3] == "partial"]
        assert items[:len(partial)] == partial                                     # partial items first ...
        direct = [it[1] for it in items[len(partial):]]
        assert direct == sorted(direct, reverse=True)                              # ... then whole genomes, longest first


def test_auto_never_cuts_below_65536_end_positions():
    k = 31
    assert model.CHUNK_MIN == _lib.SPLIT_CHUNK_MIN == 65536
    for resident in (1, 256, 512, 100000):
        lengths = [0, 13000, 65536 + k - 1, 65536 + k, 300000, 5_000_000]
        rc, info, counts = lib_plan(lengths, k, 512, 0, model.AUTO, resident)
        assert rc == 0 and info["chunk"] >= 65536 and info["chunk"] % 65536 == 0
        assert counts[:3] == [1, 1, 1]                                             # 65 565 bases: 65 536 end positions, one chunk
        for L, c in zip(lengths, counts):
            assert c == 1 or model.end_positions(L, k) > 65536
    rc, info, counts = lib_plan(lengths, k, 512, 0, model.AUTO, 100000)
    assert info["chunk"] == 65536 and counts == [1, 1, 1, 2, 5, 77]
    rc, info, counts = lib_plan([13000] * 12, k, 512, 0, model.AUTO, 256)          # twelve 13-kbase genomes: the old launch
    assert rc == 0 and info["split_genomes"] == 0 and info["items"] == 12
    # one round of resident workgroups: 256 genomes of 1 Mbase on 256 workgroups are left whole, one genome of 256 Mbase is cut in 256
    rc, info, _ = lib_plan([1_000_000] * 256, k, 512, 0, model.AUTO, 256)
    assert rc == 0 and info["split_genomes"] == 0
    rc, info, _ = lib_plan([256_000_000], k, 512, 0, model.AUTO, 256)
    assert rc == 0 and info["chunk"] == 1_048_576 and info["chunks"] == 245 and info["levels"] == 2


def test_auto_respects_the_scratch_cap():
    k = 31
    assert model.SCRATCH_MAX == _lib.SPLIT_SCRATCH_MAX == 1 << 30
    lengths = [3_000_000_000, 2_000_000_000, 70000]
    for m, p_aux in ((0, 0), (512, 0), (2048, 12)):
        rc, info, counts = lib_plan(lengths, k, m, p_aux, model.AUTO, 1 << 20)     # a device so wide that the rule alone says 65 536
        assert rc == 0 and info["chunks"] * model.row_bytes(m, p_aux) <= 1 << 30
        assert info["chunk"] > 65536 and info == model.plan(lengths, k, m, p_aux, model.AUTO, 1 << 20)[0]
        # the doubling stopped at the first chunk length that fits
        assert sum(c for c in (model.chunks_of(L, k, info["chunk"] // 2) for L in lengths) if c >= 2) * model.row_bytes(m, p_aux) > 1 << 30
    # an explicit chunk beyond the cap: the out-of-memory status, a message, nothing written
    rc, info, counts = lib_plan(lengths, k, 512, 0, 65536, 256)
    assert rc == NOMEM and "partial rows" in pkg.hip_lib().selhip_last_error(None).decode()
    assert counts == [-7] * 3 and info["chunk"] == 0
    with pytest.raises(model.Refused, match="nomem"):
        model.plan(lengths, k, 512, 0, 65536, 256)
    assert 65536 * 16384 == 1 << 30
    assert lib_plan([64 * 65536 + 30], k, 0, 0, 64, 1)[0] == 0                     # 65 536 chunks of HLL rows: exactly the cap
    assert lib_plan([64 * 65537 + 30], k, 0, 0, 64, 1)[0] == NOMEM


def test_refusals():
    lib = pkg.hip_lib()
    for chunk in (1, 63, 65, 100, 65535, -2, -64):
        rc, info, counts = lib_plan([5000, 100], 31, 64, 0, chunk, 256)
        assert rc == BADARG and counts == [-7, -7], chunk
        assert "multiple of 64" in lib.selhip_last_error(None).decode()
        with pytest.raises(model.Refused, match="badarg"):
            model.plan([5000, 100], 31, 64, 0, chunk, 256)
    for k in (0, 33):
        assert lib_plan([5000], k, 64, 0, 64, 256)[0] == BADARG
    info = _lib.BuildInfo()
    off = np.array([0, 100, 50], dtype=np.int64)                                   # descending offsets
    assert lib.selhip_build_split_plan(off.ctypes.data, 2, 31, 0, 0, 64, 256, None, C.byref(info)) == BADARG
    assert "offsets" in lib.selhip_last_error(None).decode()
    off = np.array([-1, 100, 200], dtype=np.int64)
    assert lib.selhip_build_split_plan(off.ctypes.data, 2, 31, 0, 0, 64, 256, None, C.byref(info)) == BADARG
    off = np.array([0, 100, 200], dtype=np.int64)
    assert lib.selhip_build_split_plan(off.ctypes.data, 2, 31, 0, 0, 64, 256, None, None) == BADARG
    assert lib.selhip_build_split_plan(None, 2, 31, 0, 0, 64, 256, None, C.byref(info)) == BADARG
    assert lib.selhip_build_split_plan(off.ctypes.data, 2, 31, 0, 0, 64, 256, None, C.byref(info)) == 0 and info.chunks == 4
    # the entry refuses before any device call (no GPU here): chunk, then the alignment of what the finish kernel stores 16 bytes at a time
    fake = dict(codes=1 << 20, off=2 << 20, hll=3 << 20, smh=4 << 20, aux=5 << 20)

    def entry(chunk=64, n=1, k=31, m=64, p_aux=8, **over):
        a = dict(fake)
        a.update(over)
        return lib.selhip_build_sketches_split(a["codes"], a["off"], None, n, k, m, p_aux, chunk, a["hll"], a["smh"], a["aux"], None, None)

    for kw in (dict(chunk=100), dict(chunk=-2), dict(chunk=63), dict(k=0), dict(k=33), dict(m=48), dict(m=4096), dict(p_aux=3), dict(p_aux=13),
               dict(codes=None), dict(off=None), dict(hll=None), dict(n=-1), dict(hll=fake["hll"] + 8), dict(aux=fake["aux"] + 4), dict(smh=fake["smh"] + 4)):
        assert entry(**kw) == BADARG, kw
        assert lib.selhip_last_error(None).decode().startswith("selhip_build_sketches_split:"), kw
    assert entry(n=0) == 0 and entry(n=0, chunk=model.OFF) == 0 and entry(n=0, chunk=model.AUTO) == 0


def test_declarations_and_constants():
    header = (ROOT / "include" / "selection_hip.h").read_text()
    for word in ("#define SELHIP_SPLIT_AUTO 0", "#define SELHIP_SPLIT_OFF  (-1)",
                 "typedef struct { int64_t chunk, items, split_genomes, chunks, fallback_genomes; int32_t levels, threads; } selhip_build_info_t;",
                 "int selhip_build_sketches_split(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets /* or NULL: copied back once */,",
                 "int selhip_build_split_plan(const int64_t* h_offsets, int64_t n_genomes, int k, int m, int p_aux, int64_t chunk, int64_t resident_blocks,"):
        assert word in header, word
    nomem = [ln for ln in header.splitlines() if ln.startswith("#define SELHIP_E_NOMEM")]
    assert len(nomem) == 1 and int(nomem[0].split()[2]) == _lib.E_NOMEM == NOMEM
    assert (_lib.SPLIT_AUTO, _lib.SPLIT_OFF) == (model.AUTO, model.OFF) == (0, -1)
    assert C.sizeof(_lib.BuildInfo) == 5 * 8 + 2 * 4
    plan_src = (ROOT / "cuda_selection_criteria_amd" / "csrc" / "host_plan.hpp").read_text()
    assert f"constexpr long long kSplitRounds = {model.ROUNDS};" in plan_src
    assert "constexpr unsigned long long kSplitScratchMax = 1ull << 30;" in plan_src
    assert "constexpr long long kSplitChunkMin = (long long)kSketchSeg * 1024;" in plan_src
    assert model.MERGE_SEGMENT == _lib.MERGE_SEGMENT
    nm = subprocess.run(["nm", "-D", "--defined-only", str(LIBDIR / "libselhip.so")], capture_output=True, text=True, check=True).stdout
    for name in ("selhip_build_sketches_split", "selhip_build_split_plan"):
        assert f" T {name}\n" in nm and name in _lib.HIP_SYMBOLS and getattr(pkg.hip_lib(), name) is not None
    assert (split_chunk("auto"), split_chunk("off"), split_chunk(4096)) == (0, -1, 4096)
    for bad in (0, -64, "on", True, 1.5):
        with pytest.raises(ValueError):
            split_chunk(bad)
    info, counts = split_plan([5000, 100], k=31, m=64, split=128)
    assert info["chunks"] == 39 and list(counts) == [39, 1]
    with pytest.raises(pkg.SelhipError):
        split_plan([5000], split=100)
    with pytest.raises(ValueError):
        pkg.build.build_from_codes([], info=True)


def test_build_sketch_cli_refuses_a_malformed_split(tmp_path):
    """status 2, before the file list is opened (there is none) and before the device check (there may be no device)"""
    for bad in ("bogus", "100", "-64", "0", "64x", ""):
        r = subprocess.run([str(BIN / "build_sketch"), "-s", bad, "-l", str(tmp_path / "no_such_list.txt")], capture_output=True, text=True)
        assert r.returncode == 2 and "-s takes" in r.stderr, (bad, r.returncode, r.stderr)
    r = subprocess.run([str(BIN / "build_sketch"), "-x"], capture_output=True, text=True)
    assert r.returncode == 0 and "-s auto|off|" in r.stdout
