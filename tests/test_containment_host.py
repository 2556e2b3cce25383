"""The containment measures (selhip_ctx_set_measure, SELHIP_MEASURE_INTERSECTION / _CONTAINMENT / _MAX_CONTAINMENT), the parts that need
no GPU: the model of containment_model.py tied to the oracle, the figures it gives on the influenza fixtures and on the nested set, the
constants and the exported symbol, the Python wrappers' names and refusals, and every refusal of the CLI's -S."""
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

import containment_model as cm
from test_exhaustive_host import flat_oracle_select
import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import FP_FMA, FP_STRICT, MODE_CB_SMH, MODE_SMH, _lib

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
SEL = str(BIN / "selection")
FLAVOURS = [FP_FMA, FP_STRICT]
# pairs of the 45 with J >= tau / with I / min(e) >= tau, both FP flavours
INFLUENZA = {0.5: (7, 7), 0.8: (7, 7), 0.9: (7, 7), 0.95: (5, 7), 0.99: (0, 1), 1.0: (0, 0)}
INFLUENZA_MAX = 0.9902720569357296


def influenza(fp):
    ds = pkg.load_dataset("influenza_filelist.txt", 0, 0, fp)
    assert ds.hll.shape == (10, 16384)
    return ds


# ---- 1. the model's numerator is the oracle's --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp", FLAVOURS)
def test_model_jaccard_has_the_oracle_bits(oracle, monkeypatch, fp):
    monkeypatch.chdir(GOLDEN)
    ds = influenza(fp)
    # the oracle's exhaustive loop (orc_select knows no criterion 4: smh_a on all-equal SuperMinHash sketches passes every pair, the
    # form every test of criterion none takes its J from), tau = -inf, no CB
    pairs, st = flat_oracle_select(oracle, ds.hll, ds.cards, -np.inf, False, fp)
    assert len(pairs) == 45 and st["evaluated"] == 45
    J = cm.values(cm.union_matrix(oracle, ds.hll, ds.hll, fp, symmetric=True), ds.cards, ds.cards)["jaccard"]
    assert np.array_equal(J[pairs["i"], pairs["k"]].view(np.uint64), pairs["jaccard"].view(np.uint64))


# ---- 2. the influenza figures ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp", FLAVOURS)
def test_influenza_counts(oracle, monkeypatch, fp):
    monkeypatch.chdir(GOLDEN)
    ds = influenza(fp)
    e = cm.trunc(ds.cards)
    assert (int(e.min()), int(e.max())) == (12892, 13323)
    val = cm.values(cm.union_matrix(oracle, ds.hll, ds.hll, fp, symmetric=True), ds.cards, ds.cards)
    E = cm.pair_space(ds.cards)
    assert int(E.sum()) == 45
    for tau, (n_j, n_v) in INFLUENZA.items():
        assert (len(cm.select(val["jaccard"], E, tau)), len(cm.select(val["max_containment"], E, tau))) == (n_j, n_v), tau
    assert float(val["max_containment"][E].max()) == INFLUENZA_MAX


# ---- 3. the nested set -------------------------------------------------------------------------------------------------------------
def test_nested_set_counts(oracle):
    hll, aux, cards, perm, members = cm.nested_set(oracle)
    n = len(cards)
    assert n == 15 and sorted(perm.tolist()) == list(range(n)) and np.all(np.diff(cards) >= 0)
    val = cm.values(cm.union_matrix(oracle, hll, hll, symmetric=True), cards, cards)
    E = cm.pair_space(cards)
    e = cm.trunc(cards)
    for tau, (n_j, n_v, n_cut) in {0.9: (55, 79, 10), 0.95: (45, 77, 32)}.items():
        rec_j, rec_v = cm.select(val["jaccard"], E, tau), cm.select(val["max_containment"], E, tau)
        cut = int((e[rec_v["i"]] / e[rec_v["k"]] < np.float64(np.float32(tau))).sum())         # pairs the CB bound would have dropped
        assert (len(rec_j), len(rec_v), cut) == (n_j, n_v, n_cut), tau
        assert set(zip(rec_j["i"].tolist(), rec_j["k"].tolist())) <= set(zip(rec_v["i"].tolist(), rec_v["k"].tolist()))
    assert np.nanmax(val["max_containment"][E]) <= 1.0
    # a nested row contains every genome under it: the smaller one is found whole, up to estimator noise
    for top, below in members:
        for g in below:
            assert val["max_containment"][min(top, g), max(top, g)] > 0.97, (top, g)
    # containment is the directed value: I / e_row, and the max containment is the larger of the two directions
    C = val["containment"]
    assert not np.array_equal(C.view(np.uint64), C.T.view(np.uint64))
    pos = E & (val["intersection"] > 0)
    assert np.array_equal(np.fmax(C, C.T)[pos].view(np.uint64), val["max_containment"][pos].view(np.uint64))


def test_model_empty_sketch():
    U = np.array([[0.0, 100.5], [100.5, 100.5]])
    val = cm.values(U, np.array([0.0, 100.9]), np.array([0.0, 100.9]))
    assert np.isnan(val["containment"][0]).all() and not np.isnan(val["containment"][1]).any()
    assert np.isnan(val["max_containment"][0, 1]) and np.isnan(val["max_containment"][1, 0]) and val["max_containment"][1, 1] == (200.0 - 100.5) / 100.0
    assert len(cm.select(val["max_containment"], cm.pair_space(np.array([0.0, 100.9])), -1.0)) == 0
    M = cm.matrix_model(U, np.array([0.0, 100.9]), np.array([0.0, 100.9]), "max_containment", True)
    assert M[0, 0] == 1.0 and M[1, 1] == 1.0 and np.isnan(M[0, 1])
    assert cm.matrix_model(U, np.array([0.0, 100.9]), np.array([0.0, 100.9]), "intersection", True)[1, 1] == 200.0 - 100.5


# ---- 4. constants, symbol, header --------------------------------------------------------------------------------------------------
def test_constants_and_header():
    assert (pkg.MEASURE_INTERSECTION, pkg.MEASURE_CONTAINMENT, pkg.MEASURE_MAX_CONTAINMENT) == (32, 33, 34)
    assert (pkg.MEASURE_JACCARD, pkg.MEASURE_UNION, pkg.MEASURE_SMH_MATCHES, pkg.MEASURE_SMH_JACCARD) == (0, 1, 16, 17)
    header = (ROOT / "include" / "selection_hip.h").read_text()
    for name, code in (("INTERSECTION", 32), ("CONTAINMENT", 33), ("MAX_CONTAINMENT", 34)):
        line = [l for l in header.splitlines() if l.startswith(f"#define SELHIP_MEASURE_{name} ")]
        assert len(line) == 1 and int(line[0].split()[2]) == code == getattr(_lib, f"MEASURE_{name}"), name
    assert "int selhip_ctx_set_measure(selhip_ctx* ctx, int measure);" in header
    for word in ("SELHIP_MODE_CB_SMH", "carries the measure", "small_pass_used", "NOT symmetric"):
        assert word in header, word


def test_symbol_is_declared_and_exported():
    assert "selhip_ctx_set_measure" in _lib.HIP_SYMBOLS
    lib = pkg.hip_lib()
    assert lib.selhip_ctx_set_measure is not None
    assert lib.selhip_ctx_set_measure(None, pkg.MEASURE_MAX_CONTAINMENT) == -1      # SELHIP_E_BADARG: no context
    assert hasattr(pkg.Selector, "set_measure")
    # the raw matrix entries still refuse a null context for the new codes
    for code in (32, 33, 34):
        assert lib.selhip_ctx_matrix(None, code, 0, 0, 0, None, 0, 0, 0, None, None) == -1


def test_measure_code():
    for name, code in (("intersection", 32), ("containment", 33), ("max_containment", 34), ("jaccard", 0), ("union", 1),
                       ("smh_matches", 16), ("smh_jaccard", 17)):
        assert pkg.measure_code(name) == code and pkg.measure_code(code) == code
    for bad in ("max-containment", "contain", 2, 15, 18, 35, -1, True, None, 33.0):
        with pytest.raises(ValueError, match="smh_matches"):
            pkg.measure_code(bad)


# ---- 5. the helpers' refusals come before any file is read -------------------------------------------------------------------------
def test_wrapper_refusals(tmp_path):
    missing = str(tmp_path / "no_such_list.txt")
    for call in (lambda **kw: pkg.select_from_filelist(missing, 0.9, 512, **kw),
                 lambda **kw: pkg.query_from_filelists(missing, missing, 0.9, 512, **kw),
                 lambda **kw: pkg.select_pairs_from_filelist(missing, missing, 0.9, 512, **kw)):
        with pytest.raises(ValueError, match="max_containment.*MODE_CB_SMH"):
            call(measure="max_containment")                                           # (the default mode is MODE_CB_SMH)
        with pytest.raises(ValueError, match="max_containment.*MODE_CB_SMH"):
            call(measure=pkg.MEASURE_MAX_CONTAINMENT, mode=MODE_CB_SMH, criterion="none")
        for crit in ("hll_a", "hll_an"):
            with pytest.raises(ValueError, match="max_containment.*" + crit):
                call(measure="max_containment", mode=MODE_SMH, criterion=crit)
        for matrix_only in ("intersection", "containment", "union", "smh_matches"):
            with pytest.raises(ValueError, match="measure of a pass"):
                call(measure=matrix_only, mode=MODE_SMH)
        with pytest.raises(ValueError, match="smh_matches"):
            call(measure="cosine", mode=MODE_SMH)
        # accepted: the call gets as far as reading the list
        for kw in ({"measure": "max_containment", "mode": MODE_SMH}, {"measure": "max_containment", "mode": MODE_SMH, "criterion": "none"},
                   {"measure": "max_containment", "mode": MODE_SMH, "criterion": "smh_c", "min_matches": 3}, {"measure": "jaccard"},
                   {"measure": "jaccard", "criterion": "hll_a"}):
            with pytest.raises(RuntimeError, match="selhost error"):
                call(**kw)
    for name in ("intersection", "containment", "max_containment"):
        with pytest.raises(RuntimeError, match="selhost error"):
            pkg.matrix_from_filelist(missing, measure=name)
        with pytest.raises(RuntimeError, match="selhost error"):
            pkg.query_matrix_from_filelists(missing, missing, measure=name)


# ---- 6. the CLI's -S ---------------------------------------------------------------------------------------------------------------
def run(args):
    return subprocess.run([SEL] + args, capture_output=True, text=True)


def test_cli_refusals():
    lst = ["-l", "/nonexistent/list.txt", "-h", "0.9"]
    mc = ["-S", "max_containment"]
    mat = ["-l", "/nonexistent/list.txt", "-M", "/nonexistent/out.tsv"]
    # every refusal comes before any file is read: exit 2, nothing on stdout, a message that names -S, no word about the (missing) list
    for args in (lst + mc,                                                            # without -n
                 lst + mc + ["-c", "none"],
                 ["-q", "/nonexistent/q.txt"] + lst + mc,
                 ["-p", "/nonexistent/p.txt"] + lst + mc,
                 lst + mc + ["-K", "3"],
                 lst + mc + ["-n", "-c", "hll_a"],
                 lst + mc + ["-n", "-c", "hll_an"],
                 ["-q", "/nonexistent/q.txt"] + lst + mc + ["-n", "-c", "hll_a"],
                 lst + mc + ["-n", "-g", "1"],
                 lst + mc + ["-n", "-g", "2"],
                 lst + mc + ["-n", "-B", "100"],
                 lst + mc + ["-n", "-o", "/nonexistent/out.selr"],
                 ["-p", "/nonexistent/p.txt"] + lst + mc + ["-n", "-o", "/nonexistent/out.selr"],
                 lst + ["-n", "-S", "intersection"],                                  # matrix names without -M
                 lst + ["-n", "-S", "containment"],
                 ["-q", "/nonexistent/q.txt"] + lst + ["-n", "-S", "containment"],
                 mat + ["-U", "-S", "intersection"],                                  # -S with -U
                 mat + ["-U", "-S", "max_containment"],
                 lst + ["-n", "-U"] + mc,
                 mat + ["-E", "smh", "-a", "512", "-S", "containment"],               # -S with -E smh*
                 mat + ["-E", "smh_matches", "-a", "512", "-S", "max_containment"],
                 lst + ["-n", "-S", "cosine"],                                        # an unknown name
                 mat + ["-S", "union"],
                 mat + ["-S", ""]):
        out = run(args)
        assert out.returncode == 2 and out.stdout == "" and "-S" in out.stderr, (args, out)
        assert "nonexistent" not in out.stderr and "input file" not in out.stderr, (args, out.stderr)
    # accepted: the run gets as far as the list
    for args in (lst + mc + ["-n"], lst + mc + ["-n", "-c", "none"], lst + mc + ["-n", "-c", "smh_c", "-C", "5", "-a", "512"],
                 lst + mc + ["-n", "-K", "3"], lst + ["-S", "jaccard"], lst + ["-S", "jaccard", "-c", "hll_a"],
                 lst + ["-S", "jaccard", "-o", "/nonexistent/out.selr"]):
        out = run(args)
        assert out.returncode not in (0, 2) and "No valid input file provided" in out.stderr, (args, out)
    for name in ("intersection", "containment", "max_containment", "jaccard"):
        out = run(mat + ["-S", name])
        assert out.returncode == 1 and "-M" in out.stderr and "-S" not in out.stderr, (name, out)
        out = run(mat + ["-E", "hll", "-S", name])
        assert out.returncode == 1, (name, out)
    out = run(["-q", "/nonexistent/q.txt", "-n"] + mc)
    assert out.returncode == 2 and "-q needs the database list" in out.stderr
    usage = run(["-x"]).stdout
    assert usage.startswith("Usage: -l -h -a -b") and "-S max_containment" in usage and "-S intersection|containment|max_containment" in usage
