"""selhost_read_pair_list (libselhost, no GPU): the text the selection prints -- lines 'name1 name2 J' -- read back as a list of rank
pairs, the input of a pair-list pass (selection -p, select_pairs_from_filelist)."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN

import cuda_selection_criteria_amd as pkg

EXP = GOLDEN / "expected"
NAMES = [l.strip() for l in (GOLDEN / "influenza_filelist.txt").read_text().splitlines() if l.strip()]


def read_raw(path, names, cap):
    """the C entry itself: (rc, count, stored pairs, message)"""
    h = pkg.host_lib()
    enc = [n.encode() for n in names]
    arr = (C.c_char_p * len(enc))(*enc)
    out = np.full((max(cap, 1), 2), -7, dtype=np.int32)
    cnt = C.c_int64(-1)
    rc = h.selhost_read_pair_list(str(path).encode(), arr, len(enc), out.ctypes.data if cap else None, cap, C.byref(cnt))
    return rc, cnt.value, out, h.selhost_last_error().decode()


def test_golden_stdout_round_trips_to_ranks():
    text = (EXP / "influenza_smh_a_a512_h0.01.fma.txt").read_text()
    lines = text.splitlines()
    assert len(lines) == 27
    want = np.array([[NAMES.index(l.split()[0]), NAMES.index(l.split()[1])] for l in lines], dtype=np.int32)
    got = pkg.read_pair_list(EXP / "influenza_smh_a_a512_h0.01.fma.txt", NAMES)
    assert got.dtype == np.int32 and got.shape == (27, 2) and np.array_equal(got, want)
    # the names are looked up in names[]: another rank order gives other ranks for the same lines
    rev = NAMES[::-1]
    assert np.array_equal(pkg.read_pair_list(EXP / "influenza_smh_a_a512_h0.01.fma.txt", rev), len(NAMES) - 1 - want)


def test_count_without_buffer_and_short_buffer():
    path = EXP / "influenza_none_h0.5.fma.txt"
    rc, cnt, _, _ = read_raw(path, NAMES, 0)
    assert rc == 0 and cnt == 7
    rc, cnt, out, _ = read_raw(path, NAMES, 3)
    assert rc == 0 and cnt == 7                                               # the count of the file, three entries stored
    assert np.array_equal(out[:3], pkg.read_pair_list(path, NAMES)[:3])


def test_orientation_repeats_empty_lines_and_trailing_fields(tmp_path):
    a, b, c = NAMES[2], NAMES[5], NAMES[9]
    f = tmp_path / "pairs.txt"
    f.write_text(f"{a} {b} 0.5\n"
                 f"{b} {a}\n"                                                 # reversed: kept as written
                 "\n"
                 f"{a} {b} 0.5\n"                                             # a repeated line: a second entry
                 "   \t \n"
                 f"\t{c}\t{a}   0.25 trailing words\r\n"
                 f"{b} {c}")                                                  # no newline at the end of the file
    got = pkg.read_pair_list(f, NAMES)
    assert got.tolist() == [[2, 5], [5, 2], [2, 5], [9, 2], [5, 9]]
    empty = tmp_path / "empty.txt"
    empty.write_text("\n\n")
    assert pkg.read_pair_list(empty, NAMES).shape == (0, 2)


@pytest.mark.parametrize("bad,what", [("{a} no/such/genome 0.9", "unknown name no/such/genome"),
                                      ("no/such/genome {a} 0.9", "unknown name no/such/genome"),
                                      ("{a}", "fewer than two fields"),
                                      ("{a} {a} 1.0", "equal")])
def test_errors_name_the_line(tmp_path, bad, what):
    a, b = NAMES[0], NAMES[1]
    f = tmp_path / "pairs.txt"
    f.write_text(f"{a} {b} 0.9\n\n{b} {a} 0.9\n" + bad.format(a=a) + f"\n{a} {b} 0.9\n")
    rc, cnt, _, msg = read_raw(f, NAMES, 16)
    assert rc == -3 and cnt == 0                                              # SELHOST_E_FORMAT
    assert f"{f}:4:" in msg and what in msg, msg                              # the empty line counts as a line
    with pytest.raises(RuntimeError, match=":4:"):
        pkg.read_pair_list(f, NAMES)


def test_missing_file_and_bad_arguments(tmp_path):
    rc, _, _, msg = read_raw(tmp_path / "nothing.txt", NAMES, 4)
    assert rc == -2 and "cannot open" in msg                                  # SELHOST_E_IO
    h = pkg.host_lib()
    assert h.selhost_read_pair_list(b"x", None, 0, None, 0, None) == -1       # SELHOST_E_BADARG: no count pointer
