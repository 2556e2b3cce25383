"""The winner-takes-all screen without a device (include/selection_hip.h section 2m): the model tests/gather_model.py against
decompositions worked out by hand, the declarations, the argument checks of the context-free entry and the command line's refusals."""
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import gather_model as GM

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import _lib

BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
E = int(GM.EMPTY)


def rows(*lists):
    return np.array(lists, dtype=np.uint64)


# (query, database, c_min, max_picks) -> (picks (d, unique, matches), unexplained), each worked out by hand from section 2m
HAND = {
    # rank 1 and rank 2 both share 3 buckets: the tie goes to rank 1; rank 2 then keeps buckets 4 and 5 (unique 2 of its 3 matches);
    # rank 0 shares 2, both explained by rank 1; buckets 6, 7, 8 stay
    "tie": ((rows([1, 2, 3, 4, 5, 6, 7, 8]), rows([1, 2, 0, 0, 0, 0, 0, 0], [1, 2, 3, 0, 0, 0, 0, 0], [0, 0, 3, 4, 5, 0, 0, 0]), 1, 8),
            ([(1, 3, 3), (2, 2, 3)], 3)),
    # ranks 0 and 2 are the same row: rank 0 is picked, its duplicate is left with nothing and never appears
    "duplicate": ((rows([1, 2, 3, 4]), rows([1, 2, 3, 9], [9, 9, 9, 4], [1, 2, 3, 9]), 1, 8), ([(0, 3, 3), (1, 1, 1)], 0)),
    # an unfilled query bucket matches nothing, not even an unfilled database bucket; c_min = 2 ends the query before rank 1's single bucket
    "empty buckets": ((rows([1, E, 3, 4, E, 6]), rows([1, E, 3, 0, E, 0], [0, E, 0, 4, 0, 0], [E, E, E, E, E, E]), 2, 8), ([(0, 2, 2)], 2)),
    # max_picks = 1 cuts the query short: bucket 4 stays unexplained though rank 1 would take it
    "cut short": ((rows([1, 2, 3, 4]), rows([1, 2, 3, 9], [9, 9, 9, 4]), 1, 1), ([(0, 3, 3)], 1)),
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_model_against_hand_worked_decompositions(name):
    (Q, D, c_min, max_picks), (want, left) = HAND[name]
    picks, n_picks, unexplained = GM.gather(Q, D, c_min, max_picks)
    assert [(int(p["q"]), int(p["d"]), int(p["unique"]), int(p["matches"])) for p in picks] == [(0,) + w for w in want]
    assert n_picks.tolist() == [len(want)] and unexplained.tolist() == [left]


def test_model_empty_sides():
    picks, n_picks, left = GM.gather(rows([E, E, E]), rows([E, E, E], [1, 2, 3]))
    assert len(picks) == 0 and n_picks.tolist() == [0] and left.tolist() == [0]
    picks, n_picks, left = GM.gather(rows([1, E, 3]), np.zeros((0, 3), dtype=np.uint64))
    assert len(picks) == 0 and n_picks.tolist() == [0] and left.tolist() == [2]
    assert [len(x) for x in GM.gather(np.zeros((0, 3), dtype=np.uint64), rows([1, 2, 3]))] == [0, 0, 0]


def test_declarations_and_dtype():
    header = (ROOT / "include" / "selection_hip.h").read_text()
    for name in ("selhip_gather", "selhip_ctx_gather"):
        assert name in _lib.HIP_SYMBOLS and f"int {name}(" in header
        assert hasattr(pkg.hip_lib(), name)
    assert "selhip_gather_pick_t" in header and " 2m. " in header and "#define SELHIP_GATHER_MAX_PICKS 4096" in header
    assert pkg.GATHER_DTYPE == GM.GATHER_DTYPE and pkg.GATHER_DTYPE.itemsize == 16
    for name in ("gather", "gather_table", "gather_from_filelists", "GATHER_DTYPE"):
        assert name in pkg.__all__
    assert hasattr(pkg.Selector, "gather")


@pytest.mark.parametrize("args, text", [
    ((16, 4, 16, 4, 128, 0, 8, None, None, None), "c_min = 0"), ((16, 4, 16, 4, 128, 129, 8, None, None, None), "c_min = 129"),
    ((16, 4, 16, 4, 128, 1, 0, None, None, None), "max_picks = 0"), ((16, 4, 16, 4, 128, 1, 4097, None, None, None), "max_picks = 4097"),
    ((16, 4, 16, 4, 0, 1, 8, None, None, None), "m = 0"), ((16, 4, 16, 4, 4097, 1, 8, None, None, None), "m = 4097"),
    ((16, 4, 16, 4, 128, 1, 8, 8, None, None), "16-byte aligned"), ((16, 4, 16, 4, 128, 1, 8, None, 2, None), "4-byte aligned"),
    ((16, 4, 16, 4, 128, 1, 8, None, None, 6), "4-byte aligned"), ((12, 4, 16, 4, 128, 1, 8, None, None, None), "8-byte aligned"),
    ((16, 4, 20, 4, 128, 1, 8, None, None, None), "8-byte aligned"), ((None, 4, 16, 4, 128, 1, 8, None, None, None), "non-null"),
    ((16, -1, 16, 4, 128, 1, 8, None, None, None), "0 <= n_q"),
])
def test_refusals_that_need_no_device(args, text):
    lib = pkg.hip_lib()
    assert lib.selhip_gather(*args, None) == -1 and text in lib.selhip_last_error(None).decode()


def test_nothing_to_do_and_null_context():
    lib = pkg.hip_lib()
    assert lib.selhip_gather(None, 0, None, 0, 128, 1, 8, None, None, None, None) == 0
    assert lib.selhip_ctx_gather(None, 1, 8, None, None, None) == -1


def test_table():
    picks = np.array([(1, 0, 3, 4), (0, 2, 2, 2), (1, 1, 1, 4)], dtype=pkg.GATHER_DTYPE)
    text = pkg.gather_table(["qa", "qb"], [1, 0], ["d0", "d1", "d2"], picks, 8)      # rank 1 is the list's first line
    assert text == "qb\td0\t3\t4\t0.375000\t0.500000\nqb\td1\t1\t4\t0.125000\t0.500000\nqa\td2\t2\t2\t0.250000\t0.250000\n"


@pytest.mark.parametrize("extra, word", [
    ([], "-w needs the query list (-q)"), (["-q", "/nonexistent/q.txt", "-p", "x"], "-p"), (["-q", "/nonexistent/q.txt", "-M", "x"], "-M"),
    (["-q", "/nonexistent/q.txt", "-g", "2"], "-g"), (["-q", "/nonexistent/q.txt", "-B", "2"], "-B"), (["-q", "/nonexistent/q.txt", "-r", "x"], "-r"),
    (["-q", "/nonexistent/q.txt", "-L", "x"], "-L"), (["-q", "/nonexistent/q.txt", "-H", "x"], "-H"), (["-q", "/nonexistent/q.txt", "-N", "x"], "-N"),
])
def test_cli_usage_errors(extra, word):
    out = subprocess.run([str(BIN / "selection"), "-l", "/nonexistent/list.txt", "-a", "512", "-w", "/nonexistent/dir/out.tsv"] + extra,
                         capture_output=True, text=True)
    assert out.returncode == 2 and out.stdout == "" and "-w" in out.stderr and word in out.stderr, out
