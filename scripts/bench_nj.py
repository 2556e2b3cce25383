#!/usr/bin/env python3
"""GPU box: the neighbour-joining tree of the dense matrix on the device (selhip_ctx_neighbor_joining / selhip_neighbor_joining,
DESIGN.md section 33) beside the matrix call that feeds it, the bare copy of the f64 matrix to the host -- the first step of every
host route --, selhip_linkage average on the same matrix, and the host route itself: the copy plus the vectorised numpy model
(tests/nj_model.py).

  sets      cfg3 (10 000 genomes) and its first 4 096
  measures  smh_jaccard and jaccard

Every (set, measure) runs in a child process of its own under its own time limit.  Three warm calls, then `--reps` alternating rounds
(a fresh seeded order every round) of
  nj       neighbor_joining(D, overwrite=True) on a fresh device copy of the distance matrix (the copy is not timed)
  matrix   Selector.matrix(measure) into a kept tensor
  both     Selector.neighbor_joining(measure, to_host=False): matrix + joins, scratch included
  linkage  linkage(D, "average", overwrite=True) on a fresh device copy
  copy     the f64 matrix as it lies, device -> pageable host memory, nothing else (selhip_memcpy_d2h); wall ms
median (min ... max) each, device ms between two events and wall ms around the call; whether matrix + joins (wall) beats the bare
copy -- recorded, not asserted.  The two device routes are compared byte for byte before and after the timed rounds.  The host route
runs `--host-reps` times up to `--host-max-n` genomes (its cost is cubic: "not measured" beyond), and its records are compared
with the device's byte for byte.

usage: bench_nj.py [--out profiles/nj_bench.json] [--only 10000:smh_jaccard,...] [--reps 10] [--host-reps 3] [--host-max-n 4096] [--limit seconds]
"""
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
sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(ROOT / "tests"))

from bench_cluster import med  # noqa: E402

SETS = (10000, 4096)
MEASURES = ("smh_jaccard", "jaccard")


def bench(n, measure, reps, host_reps, host_max_n):
    import torch
    import cuda_selection_criteria_amd as pkg
    import nj_model
    cfg = pkg.SYNTH_CONFIGS["cfg3"] if n == pkg.SYNTH_CONFIGS["cfg3"].n_genomes else pkg.SYNTH_CONFIGS["cfg3"].scaled(n)
    hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg, device=0)
    lib = pkg.hip_lib()
    out = {"workload": f"{n}:{measure}", "n_genomes": n, "measure": measure, "matrix_bytes": 8 * n * n}
    with pkg.Selector(0) as sel:
        sel.attach(hll_t, aux_t, cards_t)
        sim = sel.matrix(measure)
        dist = torch.where(torch.isnan(sim), torch.ones_like(sim), 1.0 - sim)
        del sim
        host = np.empty((n, n), dtype=np.float64)
        kept, work = torch.empty_like(dist), torch.empty_like(dist)

        def copy():
            pkg._lib.check(lib.selhip_memcpy_d2h(host.ctypes.data, C.c_void_p(dist.data_ptr()), host.nbytes))

        def routes_equal():
            a, b = sel.neighbor_joining(measure), pkg.neighbor_joining(dist)
            return a["joins"], bool(a["joins"].tobytes() == b["joins"].tobytes())

        calls = {"nj": lambda: pkg.neighbor_joining(work, overwrite=True, to_host=False), "matrix": lambda: sel.matrix(measure, out=kept),
                 "both": lambda: sel.neighbor_joining(measure, to_host=False), "linkage": lambda: pkg.linkage(work, "average", overwrite=True, to_host=False)}
        before, same_before = routes_equal()
        for _ in range(3):
            for call in calls.values():
                work.copy_(dist)
                call()
            copy()
        samples = {k + s: [] for k in calls for s in ("_ms", "_wall_ms")}
        samples["copy_wall_ms"] = []
        rng = np.random.default_rng(1)
        order = list(calls) + ["copy"]
        for r in range(reps):
            for which in rng.permutation(len(order)):
                what = order[which]
                work.copy_(dist)
                torch.cuda.synchronize()
                if what == "copy":
                    t0 = time.perf_counter()
                    copy()
                    samples["copy_wall_ms"].append(1e3 * (time.perf_counter() - t0))
                    continue
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record()
                calls[what]()
                b.record()
                torch.cuda.synchronize()
                samples[what + "_wall_ms"].append(1e3 * (time.perf_counter() - t0))
                samples[what + "_ms"].append(a.elapsed_time(b))
            print(f"  [{out['workload']}] round {r + 1} of {reps}", file=sys.stderr, flush=True)
        out.update({k: med(v) for k, v in samples.items()})
        after, same_after = routes_equal()
        out["routes_equal_before_and_after"] = bool(same_before and same_after and before.tobytes() == after.tobytes())
        out["both_wall_below_copy_wall"] = bool(out["both_wall_ms"]["median"] < out["copy_wall_ms"]["median"])
        out["negative_lengths"] = int(np.sum(after["len_a"] < 0) + np.sum(after["len_b"] < 0))
        out["host_copy_wall_ms"] = out["host_numpy_model_wall_ms"] = out["host_records_equal"] = "not measured"
        if n <= host_max_n and host_reps > 0:
            copy_ms, host_ms, equal = [], [], True
            for _ in range(host_reps):
                t0 = time.perf_counter()
                copy()
                copy_ms.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                joins = nj_model.neighbor_joining(host)
                host_ms.append(1e3 * (time.perf_counter() - t0))
                equal = equal and joins.tobytes() == after.tobytes()
                print(f"  [{out['workload']}] host route {len(host_ms)} of {host_reps}", file=sys.stderr, flush=True)
            out["host_copy_wall_ms"], out["host_numpy_model_wall_ms"], out["host_records_equal"] = med(copy_ms), med(host_ms), bool(equal)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/nj_bench.json")
    ap.add_argument("--only", default=",".join(f"{n}:{m}" for n in SETS for m in MEASURES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--host-max-n", type=int, default=4096)
    ap.add_argument("--limit", type=int, default=400, help="seconds a workload's child process may take")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        n, measure = args.worker.split(":")
        print("RESULT " + json.dumps(bench(int(n), measure, args.reps, args.host_reps, args.host_max_n)), flush=True)
        return 0
    results = []
    for name in args.only.split(","):
        # a fresh child process per workload, under its own time limit; nothing more is started after one that failed
        child = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, __file__, "--worker", name, "--reps", str(args.reps),
                                "--host-reps", str(args.host_reps), "--host-max-n", str(args.host_max_n)], stdout=subprocess.PIPE, text=True)
        line = next((ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if child.returncode != 0 or line is None:
            print(f"workload {name} ended with status {child.returncode}: stopping", file=sys.stderr, flush=True)
            return 1
        results.append(json.loads(line[len("RESULT "):]))
        print(json.dumps(results[-1]), flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": "MI355X", "reps": args.reps, "host_reps": args.host_reps, "workloads": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
