#!/usr/bin/env python3
"""GPU box: the hierarchy of the dense matrix on the device (selhip_ctx_linkage / selhip_linkage) beside the
matrix call that feeds it, the bare copy of the f64 matrix to the host -- the first step of every host route -- and the host route
itself, scipy.cluster.hierarchy.linkage over the copied matrix.

  sets      cfg3 (10 000 genomes) and its first 4 096
  measures  smh_jaccard and jaccard
  methods   average with max_height = inf, average with max_height = 0.1, single, complete (both whole)

Every (set, measure) runs in a child process of its own under its own time limit.  Per line: three warm calls, then `--reps`
alternating rounds (a fresh seeded order every round) of
  both     Selector.linkage(measure, method, max_height, to_host=False): matrix + linkage, scratch included; device ms between two
           events and wall ms around the call
  linkage  linkage(D, method, max_height, overwrite=True) on a fresh device copy of the distance matrix (the copy is not timed)
  matrix   Selector.matrix(measure) into a kept tensor
  copy     the f64 matrix as it lies, device -> pageable host memory, nothing else (selhip_memcpy_d2h); wall ms
median (min ... max) each; the rounds, rescan rounds and row scans of the call; whether matrix + linkage (wall) beats the bare copy
and whether the linkage alone stays within the device time of its own matrix call -- both recorded, neither asserted.  The two device
routes are compared byte for byte before and after the timed rounds.  The host route runs `--host-reps` times: the copy, then
scipy.cluster.hierarchy.linkage(squareform(D), method); its sorted heights are compared with the device's (the largest relative
difference is recorded; for a capped call over the heights up to the cap).

usage: bench_linkage.py [--out profiles/linkage_bench.json] [--only 10000:smh_jaccard,...] [--reps 20] [--host-reps 3] [--limit seconds]
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

from bench_cluster import med  # noqa: E402

SETS = (10000, 4096)
MEASURES = ("smh_jaccard", "jaccard")
LINES = (("average", None), ("average", 0.1), ("single", None), ("complete", None))


def timed(sel, pkg, lib, dist, host, measure, method, cap, reps, name):
    import torch
    kept = torch.empty_like(dist)
    work = torch.empty_like(dist)
    calls = {"both": lambda: sel.linkage(measure, method, cap, to_host=False),
             "linkage": lambda: pkg.linkage(work, method, cap, overwrite=True, to_host=False),
             "matrix": lambda: sel.matrix(measure, out=kept)}

    def copy():
        pkg._lib.check(lib.selhip_memcpy_d2h(host.ctypes.data, C.c_void_p(dist.data_ptr()), host.nbytes))

    for _ in range(3):
        work.copy_(dist)
        calls["both"](), calls["linkage"](), calls["matrix"](), copy()
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
        if (r + 1) % 5 == 0:
            print(f"  [{name}] round {r + 1} of {reps}", file=sys.stderr, flush=True)
    return {k: med(v) for k, v in samples.items()}


def bench(n, measure, reps, host_reps):
    import torch
    import cuda_selection_criteria_amd as pkg
    from scipy.cluster.hierarchy import linkage as scipy_linkage
    from scipy.spatial.distance import squareform
    cfg = pkg.SYNTH_CONFIGS["cfg3"] if n == pkg.SYNTH_CONFIGS["cfg3"].n_genomes else pkg.SYNTH_CONFIGS["cfg3"].scaled(n)
    hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg, device=0)
    lib = pkg.hip_lib()
    results = []
    with pkg.Selector(0) as sel:
        sel.attach(hll_t, aux_t, cards_t)
        sim = sel.matrix(measure)
        dist = torch.where(torch.isnan(sim), torch.ones_like(sim), 1.0 - sim)
        del sim
        host = np.empty((n, n), dtype=np.float64)
        for method, cap in LINES:
            label = f"{n}:{measure}:{method}:{'inf' if cap is None else cap}"
            out = {"workload": label, "n_genomes": n, "measure": measure, "method": method, "max_height": cap, "matrix_bytes": 8 * n * n}

            def both_routes():
                a = sel.linkage(measure, method, cap)
                counts = {k: sel.get_param(f"linkage_{k}_last") for k in ("rounds", "rescans", "rowscans", "merges")}
                b = pkg.linkage(dist, method, cap)
                same = a["merges"].tobytes() == b["merges"].tobytes() and a["sizes"].tobytes() == b["sizes"].tobytes() and a["rounds"] == b["rounds"]
                return a, counts, bool(same)

            before, counts, same_before = both_routes()
            out.update(timed(sel, pkg, lib, dist, host, measure, method, cap, reps, label))
            after, _, same_after = both_routes()
            out["routes_equal_before_and_after"] = bool(same_before and same_after and before["merges"].tobytes() == after["merges"].tobytes())
            out.update(n_merges=after["n_merges"], rounds=counts["rounds"], rescan_rounds=counts["rescans"], row_scans=counts["rowscans"],
                       row_scans_per_genome=round(counts["rowscans"] / n, 2))
            out["both_wall_below_copy_wall"] = bool(out["both_wall_ms"]["median"] < out["copy_wall_ms"]["median"])
            out["linkage_within_its_matrix_call"] = bool(out["linkage_ms"]["median"] <= out["matrix_ms"]["median"])
            sel.timing(1)
            for _ in range(3):
                sel.linkage(measure, method, cap, to_host=False)
            out["linkage_timer_ms"] = round(sel.kernel_ms("linkage"), 4)
            sel.timing(0)
            copy_ms, host_ms, diff = [], [], None
            for _ in range(host_reps):
                t0 = time.perf_counter()
                pkg._lib.check(lib.selhip_memcpy_d2h(host.ctypes.data, C.c_void_p(dist.data_ptr()), host.nbytes))
                copy_ms.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                Z = scipy_linkage(squareform(host, checks=False), method)
                host_ms.append(1e3 * (time.perf_counter() - t0))
                zh = Z[:, 2] if cap is None else Z[Z[:, 2] <= cap, 2]
                h = np.sort(after["merges"]["jaccard"])
                if len(zh) == len(h):
                    with np.errstate(divide="ignore", invalid="ignore"):
                        diff = float(np.nanmax(np.where(zh > 0, np.abs(h - zh) / zh, np.abs(h - zh)))) if len(h) else 0.0
            out["host_copy_wall_ms"], out["host_scipy_linkage_wall_ms"] = med(copy_ms), med(host_ms)
            out["host_heights_max_relative_difference"] = diff
            results.append(out)
    return results


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/linkage_bench.json")
    ap.add_argument("--only", default=",".join(f"{n}:{m}" for n in SETS for m in MEASURES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=400, help="seconds a workload's child process may take")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        n, measure = args.worker.split(":")
        print("RESULT " + json.dumps(bench(int(n), measure, args.reps, args.host_reps)), flush=True)
        return 0
    results = []
    for name in args.only.split(","):
        # a fresh child process per workload, under its own time limit; nothing more is started after one that failed
        child = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, __file__, "--worker", name, "--reps", str(args.reps),
                                "--host-reps", str(args.host_reps)], stdout=subprocess.PIPE, text=True)
        line = next((ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if child.returncode != 0 or line is None:
            print(f"workload {name} ended with status {child.returncode}: stopping", file=sys.stderr, flush=True)
            return 1
        for r in json.loads(line[len("RESULT "):]):
            results.append(r)
            print(json.dumps(r), flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": "MI355X", "reps": args.reps, "host_reps": args.host_reps, "workloads": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
