#!/usr/bin/env python3
"""GPU box: greedy representative clusters of a pass's result list on the device (selhip_ctx_cluster_greedy)
against the single-linkage call on the same list and against the route that exists without either: copy the list to the host.

The four workloads of scripts/bench_cluster.py (cfg3, none4k, D4, D16: see there), each in a child process of its own under its own
time limit.  The pass runs once; then `--reps` alternating rounds (a fresh seeded order every round) of
  greedy   Selector.cluster_greedy(to_host=False), order max_degree, every record an edge: device ms between two events, wall ms
  single   Selector.cluster(to_host=False) on the same list: device ms
  copy     the records as they lie, device -> pageable host memory, nothing else: wall ms
median (min ... max) each, with the rounds the selection took and the clusters found.  Once each: selhip_ctx_fetch (skipped beyond 5e7
records) and the model's greedy (tests/greedy_model.py, plain Python) on the fetched records where the list has at most
--model-max records (it is a Python loop over the edges: beyond that it takes more than a minute), compared with the device's answer.
Then the same list cut at its 50 %, 90 % and 99 % value quantiles under max_degree and max_rank: records kept, rounds, clusters, device
ms of the greedy and of the single-linkage call.

usage: bench_greedy.py [--out profiles/greedy_bench.json] [--only cfg3,none4k,D4,D16] [--reps 20] [--limit seconds] [--model-max records]
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
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_cluster import SORTED_FETCH_MAX, WORKLOADS, med, open_pass  # noqa: E402


def timed(call):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    res = call()
    b.record()
    torch.cuda.synchronize()
    return res, a.elapsed_time(b), 1e3 * (time.perf_counter() - t0)


def bench(name, reps, model_max):
    import torch
    import cuda_selection_criteria_amd as pkg
    import greedy_model as GM
    sel, n, what, keep = open_pass(name)
    lib = pkg.hip_lib()
    ptr, cnt = sel.result_device()
    out = {"workload": name, "n_genomes": n, "pass": what, "records": cnt, "list_bytes": 16 * cnt}
    raw = np.empty(cnt, dtype=pkg.PAIR_DTYPE)

    def greedy():
        return sel.cluster_greedy(to_host=False)

    def single():
        return sel.cluster(to_host=False)

    def copy():
        if cnt:
            pkg._lib.check(lib.selhip_memcpy_d2h(raw.ctypes.data, C.c_void_p(ptr), raw.nbytes))

    greedy(), single(), copy()
    samples = {"greedy_ms": [], "greedy_wall_ms": [], "single_ms": [], "copy_wall_ms": []}
    rng = np.random.default_rng(1)
    for r in range(reps):
        for which in rng.permutation(3):
            torch.cuda.synchronize()
            if which == 0:
                _, ms, wall = timed(greedy)
                samples["greedy_ms"].append(ms)
                samples["greedy_wall_ms"].append(wall)
            elif which == 1:
                samples["single_ms"].append(timed(single)[1])
            else:
                t0 = time.perf_counter()
                copy()
                samples["copy_wall_ms"].append(1e3 * (time.perf_counter() - t0))
        if (r + 1) % 5 == 0:
            print(f"  [{name}] round {r + 1} of {reps}", file=sys.stderr, flush=True)
    for k, v in samples.items():
        out[k] = med(v)
    got = greedy()
    out["rounds"], out["n_clusters"] = got["rounds"], got["n_clusters"]
    out["largest_cluster"] = int(got["sizes"].max().item()) if got["n_clusters"] else 0
    out["single_n_clusters"] = single()["n_clusters"]
    out["list_streams_per_ms"] = round(16 * cnt / (1e6 * max(out["greedy_ms"]["median"], 1e-9)), 1)          # GB/s of ONE stream of the list
    out["greedy_wall_below_copy_wall"] = bool(out["greedy_wall_ms"]["median"] < out["copy_wall_ms"]["median"])
    out["rounds_x_list_exceeds_copy"] = bool(out["greedy_ms"]["median"] > out["copy_wall_ms"]["median"])
    if cnt <= SORTED_FETCH_MAX:
        t0 = time.perf_counter()
        sel.fetch()
        out["fetch_sorted_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
    else:
        out["fetch_sorted_wall_ms"] = None
    if cnt <= model_max:
        t0 = time.perf_counter()
        want = GM.clusters(raw, n, -np.inf, "max_degree")
        out["model_wall_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
        out["equal_model"] = bool(all(np.array_equal(got[k].cpu().numpy(), want[k]) for k in ("rep_of", "clusters", "degrees", "sizes", "representatives"))
                                  and np.array_equal(got["values"].cpu().numpy().view(np.uint64), want["values"].view(np.uint64)))
        out["rounds_bound"] = want["rounds_bound"]
    else:
        out["model_wall_ms"] = out["equal_model"] = out["rounds_bound"] = None
    sel.timing(1)
    for _ in range(3):
        greedy()
    out["greedy_timer_ms"] = round(sel.kernel_ms("greedy"), 4)
    sel.timing(0)
    out["cuts"] = []
    if cnt:
        for q in (0.5, 0.9, 0.99):
            level = float(np.quantile(raw["jaccard"], q))
            kept = int((raw["jaccard"] >= level).sum())
            for order in ("max_degree", "max_rank"):
                ms, one = [], []
                for _ in range(5):
                    res, t, _ = timed(lambda: sel.cluster_greedy(level, order=order, to_host=False))
                    ms.append(t)
                    one.append(timed(lambda: sel.cluster(level, to_host=False))[1])
                out["cuts"].append({"quantile": q, "min_value": level, "order": order, "records_kept": kept, "rounds": res["rounds"],
                                    "n_clusters": res["n_clusters"], "largest_cluster": int(res["sizes"].max().item()), "greedy_ms": med(ms),
                                    "single_ms": med(one)})
    sel.close()
    del keep
    return out


def report(r):
    print(json.dumps({k: v for k, v in r.items() if k != "cuts"}), flush=True)
    for c in r["cuts"]:
        print(f"  cut {json.dumps(c)}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/greedy_bench.json")
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--limit", type=int, default=300, help="seconds a workload's child process may take")
    ap.add_argument("--model-max", type=int, default=3_000_000, help="records up to which the Python model runs")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        print("RESULT " + json.dumps(bench(args.worker, args.reps, args.model_max)), flush=True)
        return 0
    results = []
    for name in args.only.split(","):
        # a fresh child process per workload, under its own time limit; nothing more is started after one that failed
        child = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, __file__, "--worker", name, "--reps", str(args.reps),
                                "--model-max", str(args.model_max)], stdout=subprocess.PIPE, text=True)
        line = next((ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if child.returncode != 0 or line is None:
            print(f"workload {name} ended with status {child.returncode}: stopping", file=sys.stderr, flush=True)
            return 1
        r = json.loads(line[len("RESULT "):])
        results.append(r)
        report(r)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": "MI355X", "reps": args.reps, "workloads": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
