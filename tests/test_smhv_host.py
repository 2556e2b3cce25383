"""The estimator switch of the smh_c passes (selhip_ctx_set_estimator), what needs no GPU: selhip_smh_value against
the numpy model of tests/smhv_model.py, the header's contract, the symbols, the Python names and every refusal of the front ends."""
import ctypes as C
import inspect
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import smhv_model as V

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import MEASURE_JACCARD, MEASURE_MAX_CONTAINMENT, Selector

SEL = str(ROOT / "cuda_selection_criteria_amd" / "bin" / "selection")
LIB = ROOT / "cuda_selection_criteria_amd" / "lib" / "libselhip.so"


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


# ---- selhip_smh_value ----------------------------------------------------------------------------------------------------------------
def sweep():
    """(m, c, e1, e2) arrays: every m of both kernel paths, c over 0 .. m with both ends, cardinalities in both orders, equal, 1 : 100,
    huge, and with an empty smaller genome"""
    rng = np.random.default_rng(18)
    out = []
    cards = [(0, 0), (0, 5000), (5000, 0), (1, 1), (7000, 7000), (1000, 100000), (100000, 1000), (12345, 12346), (3, 2 ** 40),
             (2 ** 53 + 1, 2 ** 62), (2 ** 63 - 1, 2 ** 63 - 1)]
    cards += [tuple(int(x) for x in rng.integers(1, 10 ** 7, 2)) for _ in range(40)]
    for m in (1, 3, 64, 100, 128, 256, 512, 1024, 4096):
        cs = sorted({0, 1, m // 4, m // 2, (3 * m) // 4, m - 1, m} | {int(x) for x in rng.integers(0, m + 1, 6)})
        for c in cs:
            if c < 0:
                continue
            for e1, e2 in cards:
                out.append((m, c, e1, e2))
    a = np.array(out, dtype=np.uint64)
    return a[:, 0].astype(np.int64), a[:, 1].astype(np.int64), a[:, 2], a[:, 3]


@pytest.mark.parametrize("measure", ["jaccard", "max_containment"])
def test_smh_value_against_the_model(measure):
    m, c, e1, e2 = sweep()
    got = pkg.smh_value(measure, m, c, e1, e2)
    want = V.value(measure, m, c, e1, e2)
    same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), [(int(m[j]), int(c[j]), int(e1[j]), int(e2[j]), got[j], want[j]) for j in np.nonzero(~same)[0][:5]]
    if measure == "jaccard":
        assert not np.isnan(got).any() and got[c == 0].max() == 0.0 and np.all(got[c == m] == 1.0)
    else:
        empty = np.minimum(e1, e2) == 0
        assert empty.any() and np.isnan(got[empty]).all() and not np.isnan(got[~empty]).any()
        assert np.all(got[(c == 0) & ~empty] == 0.0)
        assert np.all(got[(c == m) & (e1 == e2) & ~empty] == 1.0)                  # equal cardinalities, every bucket equal: 1
        ratio = (c == m) & (np.maximum(e1, e2) == 100 * np.minimum(e1, e2)) & ~empty
        assert ratio.any() and np.all(got[ratio] > 1.0)                             # 1 : 100 at c = m: 50.5, not clamped


def test_smh_value_single_values():
    assert pkg.smh_value("jaccard", 512, 410, 1, 2) == 410.0 / 512.0
    assert pkg.smh_value("max_containment", 128, 128, 1000, 100000) == (128.0 * 101000.0) / (256.0 * 1000.0)
    assert pkg.smh_value(MEASURE_MAX_CONTAINMENT, 128, 64, 7000, 7000) == (64.0 * 14000.0) / (192.0 * 7000.0)
    assert np.isnan(pkg.smh_value("max_containment", 128, 64, 0, 7000))
    assert isinstance(pkg.smh_value(MEASURE_JACCARD, 100, 50, 1, 1), float)
    # the value behind selhip_smhc_threshold: at the threshold count the estimate reaches gamma, one below it does not
    for m, g, a, b in ((512, 0.8, 6500, 90000), (128, 0.5, 13000, 13000), (100, 0.3, 40000, 41000)):
        t = pkg.containment_matches(m, g, a, b)
        assert 1 <= t <= m
        assert pkg.smh_value("max_containment", m, t, a, b) >= g - 1e-12 > pkg.smh_value("max_containment", m, t - 1, b, a) - 1e-9
    for bad in ("union", "smh_jaccard", "intersection", 16, 99):
        with pytest.raises(ValueError):
            pkg.smh_value(bad, 128, 1, 1, 1)
    # the C function itself answers NaN for a measure that no pass has
    fn = pkg.hip_lib().selhip_smh_value
    assert np.isnan(fn(1, 128, 64, 5, 5)) and np.isnan(fn(33, 128, 64, 5, 5))


# ---- the contract ----------------------------------------------------------------------------------------------------------------------
def test_header_words():
    header = (ROOT / "include" / "selection_hip.h").read_text()
    for word in ("#define SELHIP_ESTIMATOR_HLL 0", "#define SELHIP_ESTIMATOR_SMH 1",
                 "int selhip_ctx_set_estimator(selhip_ctx* ctx, int estimator);",
                 "double selhip_smh_value(int measure, int m, int c, uint64_t e1, uint64_t e2);",
                 "V = (double)c / (double)m", "V = ((double)c * (a + b)) / (((double)m + (double)c) * a)",
                 "min(e1, e2) == 0 gives NaN", "V >= (double)tau_f", "a pair with c < 1 never has a record",
                 "no HLL register or bit plane is read", "stats[1] = stats[3] = the pairs with c >= their threshold",
                 "SELHIP_E_STATE while a pass is pending",
                 # the measure's contract stays
                 "int selhip_ctx_set_measure(selhip_ctx* ctx, int measure);", "#define SELHIP_MEASURE_MAX_CONTAINMENT 34"):
        assert word in header, word
    src = (ROOT / "cuda_selection_criteria_amd" / "csrc" / "pair_value.hpp").read_text()
    assert src.count("double smh_value(") == 1


def test_symbols_and_wrappers():
    assert pkg._lib.ESTIMATOR_HLL == 0 and pkg._lib.ESTIMATOR_SMH == 1 and pkg.ESTIMATOR_SMH == 1
    for sym in ("selhip_ctx_set_estimator", "selhip_smh_value"):
        assert sym in pkg._lib.HIP_SYMBOLS
        assert getattr(pkg.hip_lib(), sym) is not None
    exported = subprocess.run(["nm", "-D", "--defined-only", str(LIB)], capture_output=True, text=True, check=True).stdout
    assert " T selhip_ctx_set_estimator" in exported and " T selhip_smh_value" in exported
    assert callable(Selector.set_estimator) and callable(pkg.smh_value)
    for helper in (pkg.select_from_filelist, pkg.query_from_filelists, pkg.select_pairs_from_filelist):
        assert inspect.signature(helper).parameters["estimator"].default == "hll"
    assert pkg.estimator_code("hll") == 0 and pkg.estimator_code("smh") == 1 and pkg.estimator_code(1) == 1
    for bad in ("HLL", "smh_c", "", 2, -1, True, 1.0, None):
        with pytest.raises(ValueError, match="estimator"):
            pkg.estimator_code(bad)


def test_setter_without_a_device():
    """the setter touches no device: without a context every code answers SELHIP_E_BADARG"""
    lib = pkg.hip_lib()
    for code in (0, 1, 2, -1):
        assert lib.selhip_ctx_set_estimator(None, C.c_int(code)) == -1


def test_wrapper_refusals(tmp_path):
    missing = str(tmp_path / "no_such_list.txt")
    for call in (lambda **kw: pkg.select_from_filelist(missing, 0.9, 512, **kw),
                 lambda **kw: pkg.query_from_filelists(missing, missing, 0.9, 512, **kw),
                 lambda **kw: pkg.select_pairs_from_filelist(missing, missing, 0.9, 512, **kw)):
        # smh_c under the estimator gets as far as reading the list
        for kw in (dict(min_matches=20), dict(min_containment=0.8), dict(min_matches=20, measure="max_containment", mode=pkg.MODE_SMH)):
            with pytest.raises(RuntimeError, match="selhost error"):
                call(criterion="smh_c", estimator="smh", **kw)
            with pytest.raises(RuntimeError, match="selhost error"):
                call(criterion="smh_c", estimator="hll", **kw)
        for other in ("smh_a", "hll_a", "hll_an", "none"):
            with pytest.raises(ValueError, match="estimator 'smh'.*takes no criterion " + other):
                call(criterion=other, estimator="smh")
        with pytest.raises(ValueError, match="estimator: 'hll' or 'smh'"):
            call(criterion="smh_c", min_matches=20, estimator="mash")
        # what the measure refuses stays refused under the estimator
        with pytest.raises(ValueError, match="max_containment"):
            call(criterion="smh_c", min_matches=20, estimator="smh", measure="max_containment", mode=pkg.MODE_CB_SMH)
        with pytest.raises(ValueError, match="smh_c needs min_matches"):
            call(criterion="smh_c", estimator="smh")


def run(args):
    return subprocess.run([SEL] + args, capture_output=True, text=True)


def test_cli_refusals():
    lst = ["-l", "/nonexistent/list.txt", "-h", "0.9"]
    smhc = lst + ["-c", "smh_c", "-C", "20", "-a", "512"]
    for args, word in ((lst + ["-V", "smh"], "-V smh needs -c smh_c"),
                       (lst + ["-V", "smh", "-c", "smh_a"], "-V smh needs -c smh_c"),
                       (lst + ["-V", "smh", "-c", "none"], "-V smh needs -c smh_c"),
                       (lst + ["-V", "smh", "-c", "hll_a", "-a", "512"], "-V smh needs -c smh_c"),
                       (["-q", "/nonexistent/q.txt"] + lst + ["-V", "smh"], "-V smh needs -c smh_c"),
                       (["-l", "/nonexistent/list.txt", "-M", "/nonexistent/out.tsv", "-V", "smh"], "-V smh"),
                       (["-l", "/nonexistent/list.txt", "-M", "/nonexistent/out.tsv", "-E", "smh", "-a", "512", "-V", "smh"], "-E"),
                       (smhc + ["-V", "smh", "-g", "2"], "-g"),
                       (smhc + ["-V", "smh", "-B", "100"], "-B"),
                       (smhc + ["-V", "mash"], "hll or smh, not 'mash'"),
                       (smhc + ["-V", ""], "hll or smh"),
                       (lst + ["-V", "SMH"], "hll or smh"),
                       # what -c smh_c and -S refuse on their own stays refused
                       (lst + ["-c", "smh_c", "-a", "512", "-V", "smh"], "-C c_min"),
                       (smhc + ["-V", "smh", "-S", "max_containment"], "needs -n")):
        out = run(args)
        assert out.returncode == 2 and out.stdout == "" and word in out.stderr, (args, out)
        assert "nonexistent" not in out.stderr and "input file" not in out.stderr, (args, out.stderr)
    # accepted: the run gets as far as the list
    for extra in (["-V", "smh"], ["-V", "hll"], ["-V", "smh", "-n"], ["-V", "smh", "-n", "-S", "max_containment"], ["-V", "smh", "-n", "-K", "3"],
                  ["-V", "smh", "-G", "0.8"], ["-V", "smh", "-o", "/nonexistent/out.selr"], ["-V", "smh", "-p", "/nonexistent/pairs.txt"]):
        out = run(smhc + extra)
        assert out.returncode not in (0, 2) and "No valid input file provided" in out.stderr, (extra, out)
    out = run(["-q", "/nonexistent/q.txt"] + smhc + ["-V", "smh", "-k", "3"])
    assert out.returncode not in (0, 2) and "-V" not in out.stderr, out
    # -V hll is the default under every criterion
    out = run(lst + ["-V", "hll"])
    assert out.returncode not in (0, 2) and "No valid input file provided" in out.stderr, out
    usage = run(["-x"]).stdout
    assert "-V smh|hll" in usage and "-G gamma" in usage and "-E smh|smh_matches" in usage
    # -E stays an option of -M
    out = run(lst + ["-E", "smh"])
    assert out.returncode == 2 and "-E (hll, smh, smh_matches) is an option of -M" in out.stderr
