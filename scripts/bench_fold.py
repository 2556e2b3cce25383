#!/usr/bin/env python3
"""GPU box: the fold of the auxiliary HLL sketches from the main registers (selhip_ctx_fold_aux_hll) against two
yardsticks, alternated round by round in ONE child process (started here under its own time limit) after warm calls:
  fold      device time of Selector.fold_aux_hll(p_aux) on a context that holds the set (events around the call)
  bitslice  device time of selhip_hll_bitslice over the same rows: an existing kernel of this library that reads exactly the same
            bytes and writes 0.75 of them back, where the fold writes at most a quarter -- the fold should not take longer
  upload    wall time of Selector.upload_aux_hll from a host array of the same shape: the route the fold replaces, WITHOUT the
            file reads that come before it
on the synthetic sets of cfg3 (10 000 genomes) and of 100 000 genomes, p = 14, p_aux in 4, 8, 12; median (min .. max) of --rounds rounds.
Every round's folded sketches are compared with the first round's, and the first round's with the host twin (selhost_hll_fold) on a
sample of genomes.  The condition -- fold median <= bitslice median + (bitslice max - bitslice min) of the same run -- is reported per
case as "within_yardstick"; the figures are written as they are either way and the script exits 0 unless a result differs.
usage: bench_fold.py [--out profiles/fold_bench.json] [--rounds 20] [--sets cfg3,100k] [--limit 900]"""
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
from cuda_selection_criteria_amd import SynthConfig  # noqa: E402

G = pkg.SYNTH_CONFIGS
SETS = {"cfg3": (G["cfg3"], 10_000), "100k": (G["cfg5"], 100_000)}
P_AUX = (4, 8, 12)


def spread(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x)), "rounds": len(x)}


def bench(name, rounds):
    import torch
    gen, n = SETS[name]
    cfg = SynthConfig(f"fold:{name}", n, 64, gen.tau, gen.seed ^ 0x00F0, cluster_size=gen.cluster_size, mode=gen.mode, n_sh_lo=gen.n_sh_lo,
                      n_sh_hi=gen.n_sh_hi)
    hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg)
    lib = pkg.hip_lib()
    planes = torch.empty((n, 6, 512), dtype=torch.int32, device=hll_t.device)
    gmax = torch.empty(n, dtype=torch.uint8, device=hll_t.device)
    khi = C.c_int()
    out = {"set": name, "n_genomes": n, "p": 14, "main_bytes": n << 14, "rounds": rounds, "per_p_aux": {}}
    ok = True

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def bitslice():
        pkg._lib.check(lib.selhip_hll_bitslice(hll_t.data_ptr(), n, planes.data_ptr(), gmax.data_ptr(), C.byref(khi), None))

    sample = np.unique(np.linspace(0, n - 1, 64).astype(np.int64))
    hll_sample = hll_t[torch.from_numpy(sample).to(hll_t.device)].cpu().numpy()
    with pkg.Selector(0) as sel, pkg.Selector(0) as up:
        sel.attach(hll_t, aux_t, cards_t)
        up.attach(hll_t, aux_t, cards_t)
        for p_aux in P_AUX:
            folded = torch.empty((n, 1 << p_aux), dtype=torch.uint8, device=hll_t.device)

            def snapshot():
                # the context's buffer is its own: the same fold through the building block, for the comparison alone
                pkg._lib.check(lib.selhip_hll_fold(hll_t.data_ptr(), n, 14, p_aux, folded.data_ptr(), None))
                pkg._lib.check(lib.selhip_device_synchronize())
                return folded.cpu().numpy()

            first = snapshot()
            identical = bool(np.array_equal(first[sample], pkg.hll_fold(hll_sample, p_aux)))
            for _ in range(3):                                           # warm: buffers allocated, code loaded
                sel.fold_aux_hll(p_aux)
                bitslice()
                up.upload_aux_hll(first, p_aux)
            t = {"fold": [], "bitslice": [], "upload": []}
            for _ in range(rounds):
                t["fold"].append(event_ms(lambda: sel.fold_aux_hll(p_aux)))
                t["bitslice"].append(event_ms(bitslice))
                t0 = time.perf_counter()
                up.upload_aux_hll(first, p_aux)
                t["upload"].append((time.perf_counter() - t0) * 1e3)
            identical = identical and bool(np.array_equal(snapshot(), first))
            f, b = spread(t["fold"]), spread(t["bitslice"])
            out["per_p_aux"][str(p_aux)] = {
                "d": 14 - p_aux, "aux_bytes": n << p_aux, "identical": identical, "fold_ms": f, "bitslice_ms": b,
                "upload_wall_ms": spread(t["upload"]), "fold_gb_per_s": float(((n << 14) + (n << p_aux)) / f["median"] / 1e6),
                "within_yardstick": bool(f["median"] <= b["median"] + (b["max"] - b["min"]))}
            ok = ok and identical
    return out, ok


def child(a):
    if pkg.hip_lib().selhip_device_count() <= 0:
        sys.exit("bench_fold.py: no MI355X (gfx950) device: nothing is measured without one")
    ok = True
    for name in a.sets.split(","):
        r, good = bench(name, a.rounds)
        print(json.dumps(r), flush=True)
        ok = ok and good
    sys.exit(0 if ok else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fold_bench.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--sets", default="cfg3,100k")
    ap.add_argument("--limit", type=int, default=900, help="seconds the measuring child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
    run = subprocess.run([sys.executable, __file__, "--child", "--rounds", str(a.rounds), "--sets", a.sets], capture_output=True, text=True,
                         timeout=a.limit)
    sys.stderr.write(run.stderr[-4000:])
    res = [json.loads(ln) for ln in run.stdout.splitlines() if ln.startswith("{")]
    for r in res:
        print(json.dumps(r), flush=True)
    if res:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    sys.exit(run.returncode)


if __name__ == "__main__":
    main()
