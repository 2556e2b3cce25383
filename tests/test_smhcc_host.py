"""Criterion smh_c's per-pair threshold for a minimum containment (selhip_ctx_set_min_containment), the parts that need no GPU: the
symbols and the header text, selhip_smhc_threshold against the numpy model of tests/smhcc_model.py, the reference values, the two
properties the fast kernel's coarse test rests on (monotone in the larger cardinality; unimodal along a sorted database), and the
refusals and pinned messages of the wrappers and of the CLI."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import smhcc_model as CC

import cuda_selection_criteria_amd as pkg

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
SEL = str(BIN / "selection")
G08, G05, G09 = (float(np.float32(x)) for x in (0.8, 0.5, 0.9))
GAMMAS = (-1.0, 0.0, 0.01, G05, G08, G09, 0.99, 1.0, 1.5)
MS = (64, 100, 128, 512, 1024)


def test_symbols_and_header():
    lib = pkg.hip_lib()
    assert lib.selhip_ctx_set_min_containment(None, 0.5) == -1            # SELHIP_E_BADARG: no context
    assert lib.selhip_smhc_threshold(512, G08, 6500, 13000) == 187
    assert hasattr(pkg.Selector, "set_min_containment") and callable(pkg.containment_matches)
    header = (ROOT / "include" / "selection_hip.h").read_text()
    assert "int selhip_ctx_set_min_containment(selhip_ctx* ctx, double gamma);" in header
    assert "int selhip_smhc_threshold(int m, double gamma, uint64_t e_lo, uint64_t e_hi);" in header
    for word in ("num = (gamma * (double)m) * a", "den = (a + b) - gamma * a", "if (a == 0) return m + 1", "(int)ceil(q)", "smhc_rule_used",
                 "NaN clears it", "SELHIP_E_STATE", "#define SELHIP_CRIT_SMH_C        5"):
        assert word in header, word
    rule = (ROOT / "cuda_selection_criteria_amd" / "csrc" / "pair_value.hpp").read_text()
    assert "SELHIP_HD int smhc_threshold(" in rule


def test_reference_values():
    for (a, b), want in (((6500, 13000), 187), ((13000, 13000), 342), ((1000, 100000), 5), ((13000, 13300), 335)):
        assert pkg.containment_matches(512, G08, a, b) == want, (a, b)
        assert int(CC.threshold(512, G08, a, b)) == want, (a, b)
    got = pkg.containment_matches(512, G08, [6500, 13000, 1000, 13000], [13000, 13000, 100000, 13300])
    assert got.dtype == np.int32 and got.tolist() == [187, 342, 5, 335]
    assert isinstance(pkg.containment_matches(512, G08, 6500, 13000), int)


def test_threshold_equals_model():
    rng = np.random.default_rng(17)
    n = 3000
    m = rng.choice([1, 3, 64, 100, 128, 192, 256, 512, 1024, 2048], size=n)
    gamma = rng.choice(list(GAMMAS) + [2.0, 3.0, 1e-9, -1e-9, 0.75], size=n)
    gamma[: n // 3] = rng.random(n // 3) * 2.2 - 0.1
    a = rng.integers(0, 2_000_000, size=n, dtype=np.uint64)
    b = a + rng.integers(0, 2_000_000, size=n, dtype=np.uint64)
    a[::17] = 0                                                              # an empty smaller genome
    b[::51] = 0
    b[5::13] = a[5::13]                                                      # equal cardinalities
    a[7::19] = rng.integers(1, 40, size=len(a[7::19]))                       # small against large: den <= 0 once gamma >= 1 + b / a never, ...
    gamma[3::23] = 1.0 + b[3::23].astype(np.float64) / np.maximum(a[3::23], 1).astype(np.float64)       # ... here den is 0 or next to it
    gamma[4::29] = 2.0 + b[4::29].astype(np.float64) / np.maximum(a[4::29], 1).astype(np.float64)       # and here below it
    big = np.array([1 << 40, (1 << 53) + 1, (1 << 63) + 12345], dtype=np.uint64)
    m, gamma = np.concatenate([m, [512, 512, 512]]), np.concatenate([gamma, [G08, G08, G08]])
    a, b = np.concatenate([a, big]), np.concatenate([b, big * np.uint64(1) + np.uint64(7)])
    want = CC.threshold(m, gamma, a, b)
    got = pkg.containment_matches(m, gamma, a, b)
    assert got.tolist() == want.tolist()
    assert np.all((got >= 0) & (got <= m + 1))
    seen = set(np.sign(want - 0).tolist()) | {"top" for w, mm in zip(want, m) if w == mm + 1}
    assert {0, 1, "top"} <= seen
    assert np.all(want[a == 0] == m[a == 0] + 1)
    with np.errstate(invalid="ignore"):
        den = (a.astype(np.float64) + b.astype(np.float64)) - gamma * a.astype(np.float64)
    assert np.count_nonzero((den <= 0) & (a != 0)) > 50 and np.all(want[(den <= 0)] == m[(den <= 0)] + 1)
    assert np.all(want[(gamma <= 0) & (a != 0) & (den > 0)] == 0)


def sorted_cards(seed, n=4000):
    return np.sort(np.random.default_rng(seed).integers(0, 2_000_000, size=n, dtype=np.uint64))


def test_monotone_in_the_larger_cardinality():
    """for a fixed smaller cardinality the threshold never rises with the larger one: the all-pairs coarse value (the threshold at the
    block's last candidate) is a lower bound of every pair's threshold"""
    e = sorted_cards(1)
    e_lo = e[::97]
    for m in MS:
        for gamma in GAMMAS:
            for a in e_lo[:12].tolist() + e_lo[-4:].tolist():
                b = e[e >= a]
                t = CC.threshold(m, gamma, a, b)
                assert np.all(np.diff(t) <= 0), (m, gamma, a)
    # and the library's function says the same on one of them
    b = e[e >= e_lo[5]]
    assert np.all(np.diff(pkg.containment_matches(512, G08, int(e_lo[5]), b[::7]).astype(np.int64)) <= 0)


def test_unimodal_along_a_sorted_database():
    """a fixed query cardinality against candidates of ascending cardinality (a = min, b = max): the threshold rises, then falls, so its
    minimum over any rank interval is at one of the interval's ends.  (Candidates of cardinality 0 have the threshold m + 1 by
    definition and stand outside that shape: the kernel's coarse value is 0 for a range that starts on one.)"""
    e = sorted_cards(2)
    e = e[e > 0]
    rng = np.random.default_rng(3)
    for m in MS:
        for gamma in GAMMAS:
            for q in rng.choice(e, size=6).tolist() + [1, int(e[-1]) * 2]:
                t = CC.threshold(m, gamma, np.minimum(e, np.uint64(q)), np.maximum(e, np.uint64(q)))
                d = np.diff(t)
                rises = np.nonzero(d > 0)[0]
                falls = np.nonzero(d < 0)[0]
                assert len(rises) == 0 or len(falls) == 0 or rises.max() < falls.min(), (m, gamma, q)
                for lo, hi in rng.integers(0, len(e), size=(8, 2)):
                    lo, hi = min(lo, hi), max(lo, hi)
                    assert t[lo:hi + 1].min() == min(t[lo], t[hi])


def test_wrapper_refusals(tmp_path):
    missing = str(tmp_path / "no_such_list.txt")
    for call in (lambda **kw: pkg.select_from_filelist(missing, 0.9, 512, **kw),
                 lambda **kw: pkg.query_from_filelists(missing, missing, 0.9, 512, **kw),
                 lambda **kw: pkg.select_pairs_from_filelist(missing, missing, 0.9, 512, **kw)):
        # smh_c with gamma, with or without c_min, gets as far as reading the list
        for kw in (dict(min_containment=0.8), dict(min_containment=0.8, min_matches=20)):
            with pytest.raises(RuntimeError, match="selhost error"):
                call(criterion="smh_c", **kw)
            with pytest.raises(RuntimeError, match="selhost error"):
                call(criterion="smh_c", measure="max_containment", mode=pkg.MODE_SMH, **kw)
        with pytest.raises(ValueError, match="smh_c needs min_matches"):
            call(criterion="smh_c")
        for other in ("smh_a", "hll_a", "hll_an", "none"):
            with pytest.raises(ValueError, match="min_containment is the per-pair count threshold of criterion smh_c"):
                call(criterion=other, min_containment=0.8)
            with pytest.raises(ValueError, match="min_matches is the count threshold of criterion smh_c"):
                call(criterion=other, min_matches=7, min_containment=0.8)
    with pytest.raises(ValueError, match="aux_bytes"):
        pkg.select_from_filelist(missing, 0.9, 0, criterion="smh_c", min_containment=0.8)


def run(args):
    return subprocess.run([SEL] + args, capture_output=True, text=True)


def test_cli_refusals():
    lst = ["-l", "/nonexistent/list.txt", "-h", "0.9"]
    for args, word in ((lst + ["-G", "0.8"], "-G"),
                       (lst + ["-G", "0.8", "-c", "smh_a"], "-G"),
                       (lst + ["-G", "0.8", "-c", "none"], "-G"),
                       (lst + ["-G", "0.8", "-c", "hll_a", "-a", "512"], "-G"),
                       (lst + ["-c", "smh_c", "-a", "512"], "-C c_min"),
                       (lst + ["-c", "smh_c", "-G", "0.8"], "-a"),
                       (lst + ["-c", "smh_c", "-G", "inf", "-a", "512"], "-G"),
                       (lst + ["-c", "smh_c", "-G", "nan", "-a", "512"], "-G"),
                       (lst + ["-c", "smh_c", "-G", "0.8", "-a", "512", "-g", "2"], "-g"),
                       (lst + ["-c", "smh_c", "-G", "0.8", "-a", "512", "-B", "100"], "-B"),
                       (lst + ["-c", "smh_c", "-G", "0.8", "-C", "65", "-a", "512"], "1..64"),
                       (["-q", "/nonexistent/q.txt"] + lst + ["-G", "0.8"], "-G"),
                       (lst + ["-M", "/nonexistent/out.tsv", "-G", "0.8"], "-M")):
        out = run(args)
        assert out.returncode == 2 and out.stdout == "" and word in out.stderr, (args, out)
        assert "nonexistent" not in out.stderr and "input file" not in out.stderr, (args, out.stderr)
    # accepted: the run gets as far as the list
    for extra in (["-G", "0.8"], ["-G", "0.8", "-C", "20"], ["-G", "0.8", "-n", "-S", "max_containment"], ["-G", "0.8", "-n", "-K", "3"], ["-G", "-1"]):
        out = run(lst + ["-c", "smh_c", "-a", "512"] + extra)
        assert out.returncode not in (0, 2) and "No valid input file provided" in out.stderr, (extra, out)
    usage = run(["-x"]).stdout
    assert "-G gamma" in usage and "-C c_min" in usage


def test_setter_without_a_device():
    """the setter touches no device: without a context every value, finite or not, answers SELHIP_E_BADARG"""
    lib = pkg.hip_lib()
    for g in (float("inf"), float("-inf"), float("nan"), 0.8):
        assert lib.selhip_ctx_set_min_containment(None, C.c_double(g)) == -1
