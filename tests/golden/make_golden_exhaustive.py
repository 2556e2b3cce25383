#!/usr/bin/env python3
"""Regenerates tests/golden/expected/influenza_none_h<tau>.{fma,nofma}.txt: what the REFERENCE prints when no criterion stands in
front of its HLL-14 Jaccard test (the ground truth of SELHIP_CRIT_NONE in mode CB).

The reference has no such option, but its `-c smh_a` loop (CB, then smh_a, then J >= tau) degenerates to it when every genome carries
the SAME SuperMinHash sketch: smh_a is then true for every pair.  So the ten influenza .hll fixtures are linked into a temporary
directory, every genome gets one identical all-zero .smh4 file (written by libselhost in the reference's format; `-a 32` = 4 buckets),
and the stdout of the reference's own programs (oracle/_ref/selection, oracle/_ref/selection_nofma, built by `make -C oracle ref` in
the authoring container) is stored as text.  Only those outputs are committed; the flat .smh4 files are not."""
import os
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
REF = ROOT / "oracle" / "_ref"

import cuda_selection_criteria_amd as pkg  # noqa: E402

TAUS = ("0.01", "0.5", "0.9")
FLAT_M = 4                                     # buckets of the flat sketch: -a 32


def flat_copy(directory: Path):
    """the fixtures' .hll files linked under directory/influenza/, one identical .smh4 next to each; returns the list file's name"""
    host = pkg.host_lib()
    names = [l.strip() for l in (HERE / "influenza_filelist.txt").read_text().splitlines() if l.strip()]
    (directory / "influenza").mkdir()
    flat = np.zeros(FLAT_M, dtype=np.uint64)
    for name in names:
        os.symlink(HERE / (name + ".hll"), directory / (name + ".hll"))
        assert host.selhost_write_smh(str(directory / name).encode() + f".smh{FLAT_M}".encode(), flat.ctypes.data, FLAT_M) == 0
    (directory / "influenza_filelist.txt").write_text("\n".join(names) + "\n")
    return "influenza_filelist.txt"


def main():
    if not (REF / "selection").exists():
        sys.exit("oracle/_ref/selection missing: run `make -C oracle ref` in the authoring container")
    exp = HERE / "expected"
    with tempfile.TemporaryDirectory() as td:
        td = Path(td)
        lst = flat_copy(td)
        for flavour, binary in (("fma", "selection"), ("nofma", "selection_nofma")):
            for h in TAUS:
                out = subprocess.run([str(REF / binary), "-l", lst, "-t", "4", "-c", "smh_a", "-a", str(8 * FLAT_M), "-h", h],
                                     cwd=td, check=True, capture_output=True, text=True).stdout
                (exp / f"influenza_none_h{h}.{flavour}.txt").write_text(out)
                print(f"influenza_none_h{h}.{flavour}.txt: {len(out.splitlines())} lines")


if __name__ == "__main__":
    main()
