#!/usr/bin/env python3
"""GPU box: the sketch builder with long genomes split across workgroups (selhip_build_sketches_split) against the
old entry (selhip_build_sketches: one workgroup per genome, the parent's kernel) in ONE child process, started here under its own time
limit.  Inputs are random codes resident on the device; m = 512, k = 31, no auxiliary rows (line a also with p_aux = 12).  After three
warm calls of each, --rounds rounds alternate the split entry under SELHIP_SPLIT_AUTO, the old entry and SELHIP_SPLIT_OFF; a call is
timed on the host from the call to the end of a device synchronisation, so the split entry's own planning, copies and read-back count.
Median (min .. max) ms.  Lines:
  a  1 x 5 Mbase                      b  8 x 5 Mbase              c  1 x 256 Mbase
  d  2 000 x 50 kbase + 1 x 20 Mbase (the long one in the middle)
  e  256 x 1 Mbase                    f  4 096 x 250 kbase        (controls: the shapes on record)
On a .. d the speed-up old / auto is recorded as measured.  On e and f the condition is auto's median <= the old entry's median + the old
entry's spread (max - min), reported as "within"; the figures are written as they are either way.  The rows of the split entry are
compared with the old entry's before the timing and behind the last round; the script exits 1 only if they differ.
--sweep: lines a, c and e under explicit chunks of 65 536 x {1, 2, 4, 8, 16} end positions as well (the record behind kSplitRounds in
csrc/host_plan.hpp), written as text to --sweep-out.
Not measured: more than one device, p_aux other than 0 and 12, the build_sketch program end to end (FASTA parsing and gunzip on the
host dominate it and are not touched).
usage: bench_build_split.py [--out profiles/build_split_bench.json] [--rounds 20] [--limit 900] [--sweep] [--sweep-out profiles/build_split_chunk_sweep.txt]"""
import argparse
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import cuda_selection_criteria_amd as pkg  # noqa: E402
from cuda_selection_criteria_amd._lib import SPLIT_AUTO, SPLIT_OFF, BuildInfo, check  # noqa: E402

K, M = 31, 512
SHAPES = {
    "a": ("1 x 5 Mbase", [5_000_000], 0),
    "a_aux12": ("1 x 5 Mbase, p_aux = 12", [5_000_000], 12),
    "b": ("8 x 5 Mbase", [5_000_000] * 8, 0),
    "c": ("1 x 256 Mbase", [256_000_000], 0),
    "d": ("2 000 x 50 kbase + 1 x 20 Mbase", [50_000] * 1000 + [20_000_000] + [50_000] * 1000, 0),
    "e": ("256 x 1 Mbase", [1_000_000] * 256, 0),
    "f": ("4 096 x 250 kbase", [250_000] * 4096, 0),
}
CONTROLS = ("e", "f")
SWEEP_LINES = ("a", "c", "e")
SWEEP_CHUNKS = [65536 * f for f in (1, 2, 4, 8, 16)]


def spread(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x)), "rounds": len(x)}


def fmt(s):
    return f"{s['median']:.3f} ({s['min']:.3f} .. {s['max']:.3f})"


class Line:
    def __init__(self, lengths, p_aux):
        import torch
        self.torch = torch
        self.lib = pkg.hip_lib()
        dev = torch.device("cuda", 0)
        self.n, self.p_aux = len(lengths), p_aux
        self.offsets = np.zeros(self.n + 1, dtype=np.int64)
        self.offsets[1:] = np.cumsum(np.asarray(lengths, dtype=np.int64))
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x5B17 + self.n)
        self.codes = torch.randint(0, 4, (int(self.offsets[-1]),), dtype=torch.uint8, device=dev, generator=gen)
        self.d_off = torch.from_numpy(self.offsets).to(dev)
        self.out = [self.rows(dev) for _ in range(2)]                     # [0]: the old entry's rows, [1]: the split entry's
        torch.cuda.synchronize()

    def rows(self, dev):
        t = self.torch
        return (t.zeros((self.n, 16384), dtype=t.uint8, device=dev), t.zeros((self.n, M), dtype=t.int64, device=dev),
                t.zeros((self.n, 1 << self.p_aux), dtype=t.uint8, device=dev) if self.p_aux else None)

    def old(self):
        hll, smh, aux = self.out[0]
        check(self.lib.selhip_build_sketches(self.codes.data_ptr(), self.d_off.data_ptr(), self.n, K, M, self.p_aux, hll.data_ptr(), smh.data_ptr(),
                                             aux.data_ptr() if aux is not None else None, None))

    def split(self, chunk):
        hll, smh, aux = self.out[1]
        info = BuildInfo()
        check(self.lib.selhip_build_sketches_split(self.codes.data_ptr(), self.d_off.data_ptr(), self.offsets.ctypes.data, self.n, K, M, self.p_aux, chunk,
                                                   hll.data_ptr(), smh.data_ptr(), aux.data_ptr() if aux is not None else None, C.byref(info), None))
        return {name: int(getattr(info, name)) for name, _ in BuildInfo._fields_}

    def wall_ms(self, fn):
        self.torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        self.torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def identical(self):
        return all(a is None or bool(self.torch.equal(a, b)) for a, b in zip(self.out[0], self.out[1]))

    def clear_split_rows(self):
        for t in self.out[1]:
            if t is not None:
                t.zero_()


def measure(line, rounds, chunks):
    """{label: spread} for the old entry and the split entry under every chunk setting of `chunks` ({label: chunk}), alternated"""
    for _ in range(3):
        line.old()
        for chunk in chunks.values():
            line.split(chunk)
    line.torch.cuda.synchronize()
    infos, same = {}, True
    for label, chunk in chunks.items():
        line.clear_split_rows()
        infos[label] = line.split(chunk)
        same = same and line.identical()
    t = {label: [] for label in ["old", *chunks]}
    for _ in range(rounds):
        for label, chunk in chunks.items():
            t[label].append(line.wall_ms(lambda: line.split(chunk)))
            if label == "auto":
                t["old"].append(line.wall_ms(line.old))
    same = same and line.identical()
    return {label: spread(v) for label, v in t.items()}, infos, same


def bench(rounds, sweep):
    out = {"k": K, "m": M, "rounds": rounds, "timing": "host wall time of the call and a device synchronisation, ms", "lines": {}}
    text, ok = [], True
    for name, (shape, lengths, p_aux) in SHAPES.items():
        if sweep and name not in SWEEP_LINES:
            continue
        line = Line(lengths, p_aux)
        chunks = {"auto": SPLIT_AUTO, "off": SPLIT_OFF}
        if sweep and name in SWEEP_LINES:
            chunks.update({str(c): c for c in SWEEP_CHUNKS})
        ms, infos, same = measure(line, rounds, chunks)
        kmers = int(sum(max(0, L - K + 1) for L in lengths))
        rec = {"shape": shape, "genomes": len(lengths), "bases": int(sum(lengths)), "p_aux": p_aux, "identical": same, "auto_plan": infos["auto"],
               "old_ms": ms["old"], "auto_ms": ms["auto"], "off_ms": ms["off"], "speedup_old_over_auto": ms["old"]["median"] / ms["auto"]["median"],
               "old_kmers_per_s": kmers / ms["old"]["median"] * 1e3, "auto_kmers_per_s": kmers / ms["auto"]["median"] * 1e3}
        if name in CONTROLS:
            rec["aim_ms"] = ms["old"]["median"] + (ms["old"]["max"] - ms["old"]["min"])
            rec["within"] = bool(ms["auto"]["median"] <= rec["aim_ms"])
        out["lines"][name] = rec
        ok = ok and same
        if sweep and name in SWEEP_LINES:
            text.append(f"line {name}  {shape}   old {fmt(ms['old'])}   auto {fmt(ms['auto'])} [C = {infos['auto']['chunk']}, {infos['auto']['chunks']} chunks]"
                        f"   off {fmt(ms['off'])}")
            for c in SWEEP_CHUNKS:
                i = infos[str(c)]
                text.append(f"    C = {c:8d}   {fmt(ms[str(c)])}   {i['chunks']} chunks of {i['split_genomes']} genomes, {i['items']} items, {i['threads']} threads, "
                            f"{i['levels']} levels")
        del line
    return out, text, ok


def child(a):
    if pkg.hip_lib().selhip_device_count() <= 0:
        sys.exit("bench_build_split.py: no MI355X (gfx950) device: nothing is measured without one")
    r, text, good = bench(a.rounds, a.sweep)
    if text:
        print("\n".join("#sweep " + ln for ln in text), flush=True)
    print(json.dumps(r), flush=True)
    sys.exit(0 if good else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "build_split_bench.json"))
    ap.add_argument("--sweep-out", default=str(ROOT / "profiles" / "build_split_chunk_sweep.txt"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--limit", type=int, default=900, help="seconds the measuring child process may take")
    ap.add_argument("--sweep", action="store_true", help="lines a, c and e under explicit chunk lengths as well")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
    cmd = [sys.executable, __file__, "--child", "--rounds", str(a.rounds)] + (["--sweep"] if a.sweep else [])
    run = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
    sys.stderr.write(run.stderr[-4000:])
    res = [json.loads(ln) for ln in run.stdout.splitlines() if ln.startswith("{")]
    sweep = [ln[len("#sweep "):] for ln in run.stdout.splitlines() if ln.startswith("#sweep ")]
    for r in res:
        print(json.dumps(r), flush=True)
    if res and not a.sweep:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    if sweep:
        print("\n".join(sweep), flush=True)
        Path(a.sweep_out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.sweep_out).write_text("\n".join(sweep) + "\n")
    sys.exit(run.returncode)


if __name__ == "__main__":
    main()
