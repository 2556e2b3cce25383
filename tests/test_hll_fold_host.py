"""Auxiliary HLL sketches folded from the main registers, what needs no GPU: the host twin selhost_hll_fold /
hll_fold against every auxiliary fixture in the tree and against the numpy model (tests/fold_model.py), the identity on hashes, the
declared symbols, and every refusal of the front ends."""
import ctypes as C
import gzip
import inspect
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import fold_model as M

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import Selector, hll_fold

SEL = str(ROOT / "cuda_selection_criteria_amd" / "bin" / "selection")
LIBDIR = ROOT / "cuda_selection_criteria_amd" / "lib"


def read_registers(path):
    """(p, registers) of a .hll / .hll_<p> file: gz, 28-byte header (u32 bf[4], u32 p, f64 value), 1 << p bytes"""
    raw = gzip.open(path, "rb").read()
    p = int(np.frombuffer(raw[16:20], dtype=np.uint32)[0])
    assert len(raw) == 28 + (1 << p), (path, len(raw), p)
    return p, np.frombuffer(raw[28:], dtype=np.uint8)


def aux_fixtures():
    out = sorted(GOLDEN.glob("influenza/*.hll_*")) + sorted(GOLDEN.glob("synth_fasta/*.hll_*"))
    return out


def test_fixture_census():
    files = aux_fixtures()
    assert len(files) == 34, len(files)
    assert sum(f.parent.name == "influenza" for f in files) == 10
    assert sorted({int(f.name.rsplit("_", 1)[1]) for f in files}) == [4, 5, 8, 12]


@pytest.mark.parametrize("aux_file", aux_fixtures(), ids=lambda f: f.name)
def test_fold_is_the_fixture(aux_file):
    p_aux, want = read_registers(aux_file)
    assert p_aux == int(aux_file.name.rsplit("_", 1)[1])
    p, main = read_registers(aux_file.with_name(aux_file.name.rsplit(".hll_", 1)[0] + ".hll"))
    assert p == 14
    got = hll_fold(main, p_aux)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert np.array_equal(M.fold(main, p_aux), want)                       # the model too: it is the other reference of this suite


@pytest.mark.parametrize("p", [4, 5, 10, 14, 20])
def test_host_twin_is_the_model(p):
    rng = np.random.default_rng(1000 + p)
    n = 3 if p < 20 else 1
    for fill in (0.6, 0.02):                                               # dense, and sparse: most groups led by empty registers
        regs = M.random_registers(rng, n, p, fill)
        for p_aux in range(4, min(p, 15) + 1):
            got = hll_fold(regs, p_aux)
            assert got.dtype == np.uint8 and got.shape == (n, 1 << p_aux)
            assert np.array_equal(got, M.fold(regs, p_aux)), (p, p_aux, fill)


@pytest.mark.parametrize("p", [4, 5, 10, 14, 15])
def test_identity_empty_and_saturated(p):
    rng = np.random.default_rng(p)
    regs = M.random_registers(rng, 2, p)
    assert np.array_equal(hll_fold(regs, p), regs)                         # d = 0
    for p_aux in range(4, min(p, 15) + 1):
        assert not hll_fold(np.zeros((2, 1 << p), dtype=np.uint8), p_aux).any()
        sat = np.zeros(1 << p, dtype=np.uint8)
        sat[0] = 64 - p + 1                                                # the largest rank the builder writes, at offset 0 of group 0
        out = hll_fold(sat, p_aux)
        assert out.shape == (1 << p_aux,) and out[0] == 64 - p_aux + 1 and not out[1:].any()


def test_fold_of_a_sketch_is_the_sketch_of_the_hashes():
    """the identity itself, from hll.h:886-888 restated in fold_model.slot: building at p and folding = building at p_aux"""
    rng = np.random.default_rng(77)
    hashes = [int(x) for x in rng.integers(0, 1 << 64, 3000, dtype=np.uint64)]
    hashes += [0, 1, (1 << 64) - 1, 1 << 63, (1 << 50) - 1, 1 << 49, 1 << 44]   # all-zero tails: the rank caps
    for p in (14, 20, 10):
        main = M.sketch(hashes, p)
        for p_aux in (4, 5, 8, min(p, 12), min(p, 15)):
            want = M.sketch(hashes, p_aux)
            assert np.array_equal(M.fold(main, p_aux), want), (p, p_aux)
            assert np.array_equal(hll_fold(main, p_aux), want), (p, p_aux)


def test_host_twin_refusals():
    h = pkg.host_lib()
    buf = np.zeros(1 << 14, dtype=np.uint8)
    out = np.zeros(1 << 14, dtype=np.uint8)
    for p, p_aux in ((14, 3), (14, 15), (20, 16), (3, 3), (21, 8), (8, 9)):
        assert h.selhost_hll_fold(buf.ctypes.data, 1, p, p_aux, out.ctypes.data) == -1, (p, p_aux)
    assert h.selhost_hll_fold(None, 1, 14, 8, out.ctypes.data) == -1
    assert h.selhost_hll_fold(buf.ctypes.data, 1, 14, 8, None) == -1
    assert h.selhost_hll_fold(buf.ctypes.data, -1, 14, 8, out.ctypes.data) == -1
    assert h.selhost_hll_fold(None, 0, 14, 8, None) == 0
    for bad in (3, 15, 16, -1):
        with pytest.raises(ValueError):
            hll_fold(buf, bad)
    with pytest.raises(ValueError):
        hll_fold(np.zeros(100, dtype=np.uint8), 4)


def test_symbols_and_wrappers():
    hip_header = (ROOT / "include" / "selection_hip.h").read_text()
    for word in ("int selhip_hll_fold(const uint8_t* d_hll, int64_t n_genomes, int p, int p_aux, uint8_t* d_out, void* hip_stream);",
                 "int selhip_ctx_fold_aux_hll(selhip_ctx* ctx, int p_aux);", "int selhip_ctx_fold_queries_aux_hll(selhip_ctx* ctx, int p_aux);",
                 "unspecified", "NOT refreshed"):
        assert word in hip_header, word
    host_header = (ROOT / "include" / "selection_host.h").read_text()
    assert "int selhost_hll_fold(const uint8_t* in, int64_t n, unsigned p, unsigned p_aux, uint8_t* out);" in host_header
    hip = subprocess.run(["nm", "-D", "--defined-only", str(LIBDIR / "libselhip.so")], capture_output=True, text=True, check=True).stdout
    for name in ("selhip_hll_fold", "selhip_ctx_fold_aux_hll", "selhip_ctx_fold_queries_aux_hll"):
        assert f" T {name}\n" in hip, name
        assert name in pkg._lib.HIP_SYMBOLS and getattr(pkg.hip_lib(), name) is not None
    host = subprocess.run(["nm", "-D", "--defined-only", str(LIBDIR / "libselhost.so")], capture_output=True, text=True, check=True).stdout
    assert " T selhost_hll_fold\n" in host and "selhost_hll_fold" in pkg._lib.HOST_SYMBOLS
    assert callable(Selector.fold_aux_hll) and callable(Selector.fold_queries_aux_hll) and callable(pkg.hll_fold)
    for fn in (pkg.select_from_filelist, pkg.query_from_filelists, pkg.select_pairs_from_filelist):
        assert inspect.signature(fn).parameters["fold_aux"].default is False
    # the rule is written once: the shared header, called by the kernel and by the host twin
    csrc = ROOT / "cuda_selection_criteria_amd" / "csrc"
    for user in (csrc / "kernel_fold.cuh", csrc / "host" / "selection_host.cpp"):
        text = user.read_text()
        assert "selhip::fold_contrib(" in text and "selhip::fold_combine(" in text, user


def test_block_refusals_without_a_device():
    # argument checks come before any HIP call
    lib = pkg.hip_lib()
    for p, p_aux in ((14, 3), (14, 15), (20, 16), (3, 3), (21, 8)):
        assert lib.selhip_hll_fold(C.c_void_p(4096), 1, p, p_aux, C.c_void_p(8192), None) == -1, (p, p_aux)
    assert lib.selhip_hll_fold(None, 1, 14, 8, C.c_void_p(8192), None) == -1
    assert lib.selhip_hll_fold(C.c_void_p(4096), 1, 14, 8, None, None) == -1
    assert lib.selhip_hll_fold(None, 0, 14, 8, None, None) == 0            # n == 0 launches nothing
    assert lib.selhip_ctx_fold_aux_hll(None, 8) == -1 and lib.selhip_ctx_fold_queries_aux_hll(None, 8) == -1


def test_python_refusals_before_any_file(tmp_path):
    missing = str(tmp_path / "no_such_list.txt")
    for crit, extra in (("smh_a", {}), ("none", {}), ("smh_c", dict(min_matches=1))):
        with pytest.raises(ValueError, match="fold_aux"):
            pkg.select_from_filelist(missing, 0.9, 256, criterion=crit, fold_aux=True, **extra)
        with pytest.raises(ValueError, match="fold_aux"):
            pkg.query_from_filelists(missing, missing, 0.9, 256, criterion=crit, fold_aux=True, **extra)
        with pytest.raises(ValueError, match="fold_aux"):
            pkg.select_pairs_from_filelist(missing, missing, 0.9, 256, criterion=crit, fold_aux=True, **extra)
    for crit in ("hll_a", "hll_an"):                                       # accepted: gets as far as reading the list
        with pytest.raises(RuntimeError, match="selhost error"):
            pkg.select_from_filelist(missing, 0.9, 256, criterion=crit, fold_aux=True)
        with pytest.raises(RuntimeError, match="selhost error"):
            pkg.query_from_filelists(missing, missing, 0.9, 256, criterion=crit, fold_aux=True)
        with pytest.raises(RuntimeError, match="selhost error"):
            pkg.select_pairs_from_filelist(missing, missing, 0.9, 256, criterion=crit, fold_aux=True)


def run(args):
    return subprocess.run([SEL] + args, capture_output=True, text=True)


def test_cli_refusals():
    base = ["-l", "/nonexistent/list.txt", "-h", "0.9", "-a", "256"]
    for args in (base + ["-D"],                                            # the default criterion is smh_a
                 base + ["-c", "smh_a", "-D"],
                 base + ["-c", "none", "-D"],
                 base + ["-c", "smh_c", "-C", "1", "-D"],
                 ["-q", "/nonexistent/q.txt"] + base + ["-c", "smh_a", "-D"],
                 base + ["-c", "none", "-K", "3", "-D"],
                 ["-l", "/nonexistent/list.txt", "-M", "/nonexistent/out.tsv", "-D"],
                 ["-l", "/nonexistent/list.txt", "-q", "/nonexistent/q.txt", "-M", "/nonexistent/out.tsv", "-D"],
                 ["-r", "/nonexistent/results.bin", "-D"],
                 ["-r", "/nonexistent/results.bin", "-c", "hll_a", "-D"],
                 ["-l", "/nonexistent/list.txt", "-c", "hll_a", "-a", "8", "-D"],          # p_aux = 3
                 ["-l", "/nonexistent/list.txt", "-c", "hll_an", "-a", "32768", "-D"]):     # p_aux = 15 > p = 14
        out = run(args)
        assert out.returncode == 2 and out.stdout == "" and "-D" in out.stderr, (args, out)
        assert "nonexistent" not in out.stderr and "input file" not in out.stderr, (args, out.stderr)
    # accepted: the run gets as far as the list
    for extra in (["-c", "hll_a", "-D"], ["-c", "hll_an", "-D"], ["-c", "hll_a", "-D", "-K", "3"], ["-c", "hll_a", "-D", "-B", "4"],
                  ["-c", "hll_an", "-D", "-p", "/nonexistent/pairs.txt"]):
        out = run(base + extra)
        assert out.returncode not in (0, 2) and "No valid input file provided" in out.stderr, (extra, out)
    usage = run(["-x"])
    assert usage.returncode == 0 and "-D" in usage.stdout and "folded from the .hll registers" in usage.stdout
