"""Sketches merged by group, what needs no GPU: the host twin selhost_merge_sketches against the numpy model
(tests/merge_model.py), the two merge identities against the sequential build oracle and against the golden files, fold and merge
commuting, every refusal of the argument rules, and the declared symbols."""
import ctypes as C
import gzip
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import merge_model as M

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import hll_fold, merge_sketches

LIBDIR = ROOT / "cuda_selection_criteria_amd" / "lib"
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)


def random_rows(rng, n, p, m, p_aux):
    """HLL bytes from the full range 0 .. 255; u64 buckets with ~0 and 0 among them"""
    hll = rng.integers(0, 256, (n, 1 << p), dtype=np.uint8)
    smh = rng.integers(0, 1 << 64, (n, m), dtype=np.uint64)
    smh[rng.random((n, m)) < 0.1] = U64_MAX
    smh[rng.random((n, m)) < 0.1] = 0
    aux = rng.integers(0, 256, (n, 1 << p_aux), dtype=np.uint8) if p_aux else None
    return hll, smh, aux


def interleaved_groups(rng, n):
    """ids in no order: group 0 empty, group 1 a singleton, group 2 a pair, some rows in no group, group 3 all the rest"""
    g = np.full(n, 3, dtype=np.int32)
    at = rng.permutation(n)
    g[at[0]] = 1
    g[at[1:3]] = 2
    g[at[3:8]] = -1
    return g, 4


def assert_merged(got, want, what=""):
    for key in ("hll", "smh", "aux_hll", "sizes"):
        assert (got[key] is None) == (want[key] is None), (what, key)
        if want[key] is not None:
            assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key, got[key].shape, want[key].shape)
            assert np.array_equal(got[key], want[key]), (what, key, np.argwhere(got[key] != want[key])[:4])


# ---- 1. the host twin is the model ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [4, 10, 14])
@pytest.mark.parametrize("m", [1, 3, 96, 512])
def test_host_twin_is_the_model(p, m):
    for p_aux in (0, 4, 8):
        rng = np.random.default_rng(1000 * p + 10 * m + p_aux)
        hll, smh, aux = random_rows(rng, 40, p, m, p_aux)
        groups, G = interleaved_groups(rng, 40)
        want = M.merge_all(hll, smh, aux, groups, G)
        assert list(want["sizes"]) == [0, 1, 2, 32]
        assert not want["hll"][0].any() and (want["smh"][0] == U64_MAX).all()          # the empty group
        assert np.array_equal(want["hll"][1], hll[groups == 1][0])                       # the singleton: a row copy
        assert_merged(merge_sketches(hll, smh, aux, groups, G, device=None), want, (p, m, p_aux))
        # every kind alone
        assert_merged(merge_sketches(hll, None, None, groups, G, device=None), M.merge_all(hll, None, None, groups, G))
        assert_merged(merge_sketches(None, smh, None, groups, G, device=None), M.merge_all(None, smh, None, groups, G))


def test_host_twin_empty_shapes():
    hll = np.zeros((0, 16), dtype=np.uint8)
    smh = np.zeros((0, 3), dtype=np.uint64)
    out = merge_sketches(hll, smh, None, np.zeros(0, dtype=np.int32), 3, device=None)
    assert out["hll"].shape == (3, 16) and not out["hll"].any() and (out["smh"] == U64_MAX).all() and not out["sizes"].any()
    hll = np.full((2, 16), 7, dtype=np.uint8)
    out = merge_sketches(hll, None, None, np.array([-1, -1], dtype=np.int32), 0, device=None)
    assert out["hll"].shape == (0, 16) and out["sizes"].shape == (0,)


# ---- 2. the identities against the sequential build oracle -----------------------------------------------------------------
@pytest.fixture(scope="module")
def build_oracle():
    import oracle_py
    return oracle_py.BuildOracle()


def write_fasta(path, codes):
    lut = np.frombuffer(b"ACGTN", dtype=np.uint8)
    path.write_bytes(b">g\n" + lut[np.asarray(codes, dtype=np.uint8)].tobytes() + b"\n")
    return path


def oracle_sketch(build_oracle, path, m):
    hll, aux, smh, _ = build_oracle.sketch(path, m=m, p_aux=8)
    return hll, aux, smh


def code_pairs():
    rng = np.random.default_rng(2024)
    base = rng.integers(0, 4, 400).astype(np.uint8)
    shared = np.concatenate([base[:250], rng.integers(0, 4, 150).astype(np.uint8)])      # 220 k-mers of base are in it too
    with_reset = rng.integers(0, 4, 300).astype(np.uint8)
    with_reset[140] = 4
    other = rng.integers(0, 4, 350).astype(np.uint8)
    empty = np.zeros(0, dtype=np.uint8)
    return {"shared": (base, shared), "reset": (with_reset, other), "empty-left": (empty, other), "empty-right": (base, empty),
            "same": (base, base.copy()), "disjoint": (other, base)}


@pytest.mark.parametrize("name", list(code_pairs()))
def test_merge_is_the_sketch_of_the_concatenation(build_oracle, tmp_path, name):
    a, b = code_pairs()[name]
    fa, fb = write_fasta(tmp_path / "a.fna", a), write_fasta(tmp_path / "b.fna", b)
    fab = write_fasta(tmp_path / "ab.fna", np.concatenate([a, [4], b]))
    groups = np.array([0, 0], dtype=np.int32)
    for m in (8, 64, 512):
        ha, xa, sa = oracle_sketch(build_oracle, fa, m)
        hb, xb, sb = oracle_sketch(build_oracle, fb, m)
        hu, xu, su = oracle_sketch(build_oracle, fab, m)
        assert sa.shape == (m,)
        if len(a) >= 31 and len(b) >= 31 and name != "same":
            assert not np.array_equal(ha, hu) and not np.array_equal(sa, su)           # the union is neither member
        got = merge_sketches(np.stack([ha, hb]), np.stack([sa, sb]), np.stack([xa, xb]), groups, 1, device=None)
        assert np.array_equal(got["hll"][0], hu), (name, m)
        assert np.array_equal(got["aux_hll"][0], xu), (name, m)
        assert np.array_equal(got["smh"][0], su), (name, m, np.argwhere(got["smh"][0] != su)[:4])
        assert_merged(got, M.merge_all(np.stack([ha, hb]), np.stack([sa, sb]), np.stack([xa, xb]), groups, 1))


# ---- 3. the golden files ---------------------------------------------------------------------------------------------------------
def read_registers(path):
    raw = gzip.open(path, "rb").read()
    p = int(np.frombuffer(raw[16:20], dtype=np.uint32)[0])
    assert len(raw) == 28 + (1 << p), (path, len(raw), p)
    return np.frombuffer(raw[28:], dtype=np.uint8)


def read_buckets(path):
    raw = gzip.open(path, "rb").read()
    cnt = int(np.frombuffer(raw[:4], dtype=np.uint32)[0])
    assert len(raw) == 4 + 8 * cnt
    return np.frombuffer(raw[4:], dtype=np.uint64)


@pytest.mark.parametrize("members", [(0, 1), (2, 5, 7)])
def test_merge_of_the_fixtures_is_the_sketch_of_their_records(build_oracle, tmp_path, members):
    fastas = sorted((GOLDEN / "influenza_fasta").glob("*.fna.gz"))
    chosen = [fastas[j] for j in members]
    stems = [GOLDEN / "influenza" / f.name for f in chosen]
    hll = np.stack([read_registers(str(s) + ".hll") for s in stems])
    smh = np.stack([read_buckets(str(s) + ".smh512") for s in stems])
    aux = np.stack([read_registers(str(s) + ".hll_8") for s in stems])
    groups = np.zeros(len(chosen), dtype=np.int32)
    got = merge_sketches(hll, smh, aux, groups, 1, device=None)
    # the records of all members in one FASTA
    union = tmp_path / "union.fna"
    union.write_bytes(b"".join(gzip.open(f, "rb").read() for f in chosen))
    hu, xu, su, n_kmers = build_oracle.sketch(union, m=512, p_aux=8)
    assert n_kmers > 0 and not any(np.array_equal(hu, row) for row in hll)
    assert np.array_equal(got["hll"][0], hu) and np.array_equal(got["aux_hll"][0], xu) and np.array_equal(got["smh"][0], su)
    # ... and through the file formats: written by selhost_write_*, read back
    h = pkg.host_lib()
    base = str(tmp_path / "merged")
    assert h.selhost_write_hll((base + ".hll").encode(), got["hll"][0].ctypes.data, 14) == 0
    assert h.selhost_write_hll((base + ".hll_8").encode(), got["aux_hll"][0].ctypes.data, 8) == 0
    assert h.selhost_write_smh((base + ".smh512").encode(), got["smh"][0].ctypes.data, 512) == 0
    assert np.array_equal(read_registers(base + ".hll"), hu) and np.array_equal(read_registers(base + ".hll_8"), xu)
    assert np.array_equal(read_buckets(base + ".smh512"), su)
    back = np.zeros(16384, dtype=np.uint8)
    p_out, hdr, val = C.c_uint32(), (C.c_uint32 * 4)(), C.c_double()
    assert h.selhost_read_hll((base + ".hll").encode(), back.ctypes.data, back.size, C.byref(p_out), hdr, C.byref(val)) == 0
    assert p_out.value == 14 and np.array_equal(back, hu)
    buckets = np.zeros(512, dtype=np.uint64)
    assert h.selhost_read_smh((base + ".smh512").encode(), buckets.ctypes.data, 512) == 512 and np.array_equal(buckets, su)


# ---- 4. fold and merge commute -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p_aux", [4, 8, 12])
def test_fold_and_merge_commute(p_aux):
    rng = np.random.default_rng(50 + p_aux)
    ranks = np.minimum(rng.geometric(0.5, (30, 1 << 14)), 51).astype(np.uint8)        # legal ranks of p = 14, a third of the registers empty
    ranks[rng.random(ranks.shape) < 0.33] = 0
    groups, G = interleaved_groups(rng, 30)
    merged_then_folded = hll_fold(merge_sketches(ranks, None, None, groups, G, device=None)["hll"], p_aux)
    folded_then_merged = merge_sketches(hll_fold(ranks, p_aux), None, None, groups, G, device=None)["hll"]
    assert merged_then_folded.any() and np.array_equal(merged_then_folded, folded_then_merged)


# ---- 5. every refusal --------------------------------------------------------------------------------------------------------------
def call(lib_fn, hll, smh, aux, n, p, m, p_aux, group, G, hll_out, smh_out, aux_out, size_out, *tail):
    ptr = lambda a: a if a is None or isinstance(a, (int, C.c_void_p)) else a.ctypes.data
    return lib_fn(ptr(hll), ptr(smh), ptr(aux), n, p, m, p_aux, ptr(group), G, ptr(hll_out), ptr(smh_out), ptr(aux_out), ptr(size_out), *tail)


def badarg_cases():
    """(what, overrides) on top of a valid call over 4 rows, p = 4, m = 3, p_aux = 4, G = 2"""
    return [("hll in only", dict(hll_out=None)), ("hll out only", dict(hll=None)), ("smh in only", dict(smh_out=None)),
            ("smh out only", dict(smh=None)), ("aux in only", dict(aux_out=None)), ("aux out only", dict(aux=None)),
            ("p 3", dict(p=3)), ("p 21", dict(p=21)), ("p_aux 3", dict(p_aux=3)), ("p_aux 21", dict(p_aux=21)), ("m 0", dict(m=0)),
            ("n < 0", dict(n=-1)), ("G < 0", dict(G=-1)), ("null group", dict(group=None))]


def valid_args():
    a = dict(hll=np.full((4, 16), 1, dtype=np.uint8), smh=np.full((4, 3), 5, dtype=np.uint64), aux=np.full((4, 16), 2, dtype=np.uint8), n=4, p=4, m=3,
             p_aux=4, group=np.array([0, 1, 1, -1], dtype=np.int32), G=2, hll_out=np.full((2, 16), 0xEE, dtype=np.uint8),
             smh_out=np.full((2, 3 * 8), 0xEE, dtype=np.uint8).view(np.uint64), aux_out=np.full((2, 16), 0xEE, dtype=np.uint8),
             size_out=np.full(2 * 4, 0xEE, dtype=np.uint8).view(np.int32))
    return a


ORDER = ("hll", "smh", "aux", "n", "p", "m", "p_aux", "group", "G", "hll_out", "smh_out", "aux_out", "size_out")


def test_host_twin_refusals():
    h = pkg.host_lib()
    a = valid_args()
    assert call(h.selhost_merge_sketches, *[a[k] for k in ORDER]) == 0
    assert list(a["size_out"]) == [1, 2] and (a["hll_out"] == 1).all() and (a["smh_out"] == 5).all()
    for what, over in badarg_cases():
        a = valid_args()
        a.update(over)
        assert call(h.selhost_merge_sketches, *[a[k] for k in ORDER]) == -1, what
        assert h.selhost_last_error().decode().startswith("merge_sketches:"), what
        for key in ("hll_out", "smh_out", "aux_out", "size_out"):
            if a[key] is not None:
                assert (a[key].view(np.uint8) == 0xEE).all(), (what, key)
    # misaligned: an 8-byte array at an odd multiple of 4, an int32 array at an odd address
    a = valid_args()
    raw = np.zeros(4 * 3 * 8 + 8, dtype=np.uint8)
    a["smh"] = C.c_void_p(raw.ctypes.data + 4)
    assert call(h.selhost_merge_sketches, *[a[k] for k in ORDER]) == -1 and "8-byte aligned" in h.selhost_last_error().decode()
    a = valid_args()
    a["group"] = C.c_void_p(raw.ctypes.data + 1)
    assert call(h.selhost_merge_sketches, *[a[k] for k in ORDER]) == -1 and "4-byte aligned" in h.selhost_last_error().decode()


@pytest.mark.parametrize("bad,count,index", [([0, 2, 1, -1], 1, 1), ([-2, 0, 5, 1], 2, 0), ([0, 1, 1, 1 << 30], 1, 3)])
def test_host_twin_bad_id(bad, count, index):
    h = pkg.host_lib()
    a = valid_args()
    a["group"] = np.array(bad, dtype=np.int32)
    assert call(h.selhost_merge_sketches, *[a[k] for k in ORDER]) == -1
    msg = h.selhost_last_error().decode()
    assert f"holds {count} invalid entries" in msg and "outside [-1, 2)" in msg and f"entry {index} is one" in msg, msg
    for key in ("hll_out", "smh_out", "aux_out", "size_out"):
        assert (a[key].view(np.uint8) == 0xEE).all(), key
    with pytest.raises(ValueError, match="invalid entries"):
        merge_sketches(a["hll"], None, None, bad, 2, device=None)


def test_device_entry_refusals_without_a_device():
    """the argument checks of selhip_merge_sketches come before any HIP call (fake, suitably aligned addresses)"""
    lib = pkg.hip_lib()
    fake = dict(hll=C.c_void_p(4096), smh=C.c_void_p(8192), aux=C.c_void_p(12288), n=4, p=4, m=3, p_aux=4, group=C.c_void_p(16384), G=2,
                hll_out=C.c_void_p(20480), smh_out=C.c_void_p(24576), aux_out=C.c_void_p(28672), size_out=C.c_void_p(32768))
    for what, over in badarg_cases():
        a = dict(fake)
        a.update(over)
        assert call(lib.selhip_merge_sketches, *[a[k] for k in ORDER], None) == -1, what
        assert lib.selhip_last_error(None).decode().startswith("selhip_merge_sketches:"), what
    for key, off, word in (("hll", 8, "16-byte"), ("hll_out", 4, "16-byte"), ("aux", 8, "16-byte"), ("aux_out", 1, "16-byte"), ("smh", 4, "8-byte"),
                           ("smh_out", 2, "8-byte"), ("group", 2, "4-byte"), ("size_out", 1, "4-byte")):
        a = dict(fake)
        a[key] = C.c_void_p(fake[key].value + off)
        assert call(lib.selhip_merge_sketches, *[a[k] for k in ORDER], None) == -1, key
        assert word in lib.selhip_last_error(None).decode(), (key, lib.selhip_last_error(None).decode())
    assert call(lib.selhip_merge_sketches, None, None, None, 0, 14, 0, 0, None, 0, None, None, None, None, None) == 0    # nothing to do
    assert lib.selhip_ctx_merge_groups(None, None, 0, None) == -1


# ---- 6. declarations -----------------------------------------------------------------------------------------------------------------
def test_symbols_and_the_segment_constant():
    hip_header = (ROOT / "include" / "selection_hip.h").read_text()
    for word in ("int selhip_merge_sketches(const uint8_t* d_hll, const uint64_t* d_smh, const uint8_t* d_aux_hll, int64_t n, int p, int m, int p_aux,",
                 "int selhip_ctx_merge_groups(selhip_ctx* ctx, const int32_t* d_group, int64_t n_groups, const selhip_merged_t* out);",
                 "} selhip_merged_t;", "2i. Sketches merged by group"):
        assert word in hip_header, word
    seg = [ln for ln in hip_header.splitlines() if ln.startswith("#define SELHIP_MERGE_SEGMENT")]
    assert len(seg) == 1 and int(seg[0].split()[2]) == pkg.MERGE_SEGMENT == pkg._lib.MERGE_SEGMENT
    host_header = (ROOT / "include" / "selection_host.h").read_text()
    assert "int selhost_merge_sketches(const uint8_t* hll, const uint64_t* smh, const uint8_t* aux_hll, int64_t n, int p, int m, int p_aux," in host_header
    hip = subprocess.run(["nm", "-D", "--defined-only", str(LIBDIR / "libselhip.so")], capture_output=True, text=True, check=True).stdout
    for name in ("selhip_merge_sketches", "selhip_ctx_merge_groups"):
        assert f" T {name}\n" in hip, name
        assert name in pkg._lib.HIP_SYMBOLS and getattr(pkg.hip_lib(), name) is not None
    host = subprocess.run(["nm", "-D", "--defined-only", str(LIBDIR / "libselhost.so")], capture_output=True, text=True, check=True).stdout
    assert " T selhost_merge_sketches\n" in host and "selhost_merge_sketches" in pkg._lib.HOST_SYMBOLS
    assert C.sizeof(pkg._lib.Merged) == 5 * C.sizeof(C.c_void_p)
    for fn in (pkg.Selector.merge, pkg.merge_sketches, pkg.selector_from_rows, pkg.merge_from_filelist, pkg.read_groups, pkg.write_merged):
        assert callable(fn)
    assert pkg.cluster_names(1) == ["cluster_0"] and pkg.cluster_names(11)[:2] == ["cluster_00", "cluster_01"] and pkg.cluster_names(0) == []


def test_read_groups(tmp_path):
    names = ["x/a", "x/b", "x/c", "x/d"]
    f = tmp_path / "groups.tsv"
    f.write_text("x/c\tbeta\nx/a\talpha\n\nx/d\tbeta\n")
    groups, gnames = pkg.read_groups(str(f), names)
    assert list(groups) == [1, -1, 0, 0] and gnames == ["beta", "alpha"]
    for text, line in (("x/a\talpha\nx/zzz\talpha\n", 2), ("x/a alpha\n", 1), ("x/a\t\n", 1), ("x/a\tal/pha\n", 1)):
        f.write_text(text)
        with pytest.raises(ValueError, match=f"groups.tsv:{line}:"):
            pkg.read_groups(str(f), names)
