#!/usr/bin/env python3
"""GPU box: the maximum spanning forest of a pass's result list on the device (selhip_ctx_spanning_forest) beside
one stream of the same list (selhip_ctx_cluster) and the bare copy of the list to the host, the first step of every host route.

  cfg3   the smh_a pass of cfg3 (10 000 genomes, m = 512, tau = 0.8): about 45 000 records -- latency-bound
  none4k criterion none at tau = 0.5 on the first 4 096 genomes of cfg3
  D4     the dense-sharing set of scripts/bench_topk_rounds.py, 4 096 genomes, behind `-c smh_c -C 1 -n -h -1 -V smh`: every pair a record
  D16    the same at 16 384 genomes: 1.3e8 records (2.1 GB) and one giant component
  D16q99 the list of D16 cut at its 99 % value quantile (same child process as D16)

Every workload runs in a child process of its own under its own time limit.  The pass runs once; three warm calls; then `--reps`
alternating rounds (a fresh seeded order every round) of
  forest   Selector.spanning_forest(min_value, to_host=False): device ms between two events and wall ms around the call
  cluster  Selector.cluster(min_value, to_host=False): the same two figures -- one stream of the list
  copy     the records as they lie, device -> pageable host memory, nothing else (selhip_memcpy_d2h of result_device); wall ms
median (min ... max) each.  The forest is checked before and after the timed rounds: byte-equal, in BEFORE order, labels equal to the
cluster call's, F = n - C.  With R picking rounds ("forest_rounds_last" - 1) the code predicts about 2 (R + 1) times the cluster call's
device time: the measured ratio is recorded beside it, and whether the forest's wall time is below the bare copy's.
On the two small lists the host route is timed `--host-reps` times and recorded only: selhip_ctx_fetch, then
scipy.sparse.csgraph.minimum_spanning_tree on the negated values (its edge count is compared with F where the values are all positive).

usage: bench_forest.py [--out profiles/forest_bench.json] [--only cfg3,none4k,D4,D16] [--reps 20] [--host-reps 3] [--limit seconds]
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

from bench_cluster import med, open_pass  # noqa: E402

WORKLOADS = ("cfg3", "none4k", "D4", "D16")
HOST_ROUTE = ("cfg3", "none4k")


def host_forest(rec, n):
    """edges of scipy's minimum spanning forest of the negated values (duplicate records of a pair: the greatest value)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    a, b = np.minimum(rec["i"], rec["k"]).astype(np.int64), np.maximum(rec["i"], rec["k"]).astype(np.int64)
    key = a * n + b
    order = np.lexsort((-rec["jaccard"], key))
    first = np.ones(len(order), dtype=bool)
    first[1:] = key[order][1:] != key[order][:-1]
    pick = order[first]
    pick = pick[a[pick] != b[pick]]
    g = coo_matrix((-rec["jaccard"][pick], (a[pick], b[pick])), shape=(n, n)).tocsr()
    return int(minimum_spanning_tree(g).nnz)


def check(sel, min_value, n):
    """the forest on the host, after the checks that need no model: order, F = n - C, labels"""
    res = sel.spanning_forest(min_value)
    clu = sel.cluster(min_value)
    e = res["edges"]
    assert res["n_edges"] == n - clu["n_clusters"] and np.array_equal(res["labels"], clu["labels"])
    assert np.all(e["i"] < e["k"])
    v, key = e["jaccard"], e["i"].astype(np.int64) * n + e["k"]
    assert np.all((v[:-1] > v[1:]) | ((v[:-1] == v[1:]) & (key[:-1] < key[1:])))
    return res


def timed(sel, lib, pkg, ptr, raw, min_value, reps, name):
    import torch
    calls = {"forest": lambda: sel.spanning_forest(min_value, to_host=False), "cluster": lambda: sel.cluster(min_value, to_host=False)}

    def copy():
        if len(raw):
            pkg._lib.check(lib.selhip_memcpy_d2h(raw.ctypes.data, C.c_void_p(ptr), raw.nbytes))

    for _ in range(3):
        calls["forest"](), calls["cluster"](), copy()
    samples = {"forest_ms": [], "forest_wall_ms": [], "cluster_ms": [], "cluster_wall_ms": [], "copy_wall_ms": []}
    rng = np.random.default_rng(1)
    for r in range(reps):
        for which in rng.permutation(3):
            torch.cuda.synchronize()
            if which == 2:
                t0 = time.perf_counter()
                copy()
                samples["copy_wall_ms"].append(1e3 * (time.perf_counter() - t0))
                continue
            what = ("forest", "cluster")[which]
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


def bench(name, reps, host_reps):
    import cuda_selection_criteria_amd as pkg
    sel, n, what, keep = open_pass(name)
    lib = pkg.hip_lib()
    ptr, cnt = sel.result_device()
    raw = np.empty(cnt, dtype=pkg.PAIR_DTYPE)
    if cnt:
        pkg._lib.check(lib.selhip_memcpy_d2h(raw.ctypes.data, C.c_void_p(ptr), raw.nbytes))
    levels = [(name, None)] + ([(name + "q99", float(np.quantile(raw["jaccard"], 0.99)))] if name == "D16" and cnt else [])
    results = []
    for label, level in levels:
        out = {"workload": label, "n_genomes": n, "pass": what, "records": cnt, "list_bytes": 16 * cnt, "min_value": level,
               "records_kept": cnt if level is None else int((raw["jaccard"] >= level).sum())}
        before = check(sel, level, n)
        out.update(timed(sel, lib, pkg, ptr, raw, level, reps, label))
        after = check(sel, level, n)
        out["checked_before_and_after"] = bool(before["edges"].tobytes() == after["edges"].tobytes() and np.array_equal(before["labels"], after["labels"]))
        out["n_edges"], out["n_clusters"], out["rounds"] = after["n_edges"], after["n_clusters"], after["rounds"]
        picking = after["rounds"] - 1
        out["picking_rounds"] = picking
        out["predicted_ratio_to_cluster"] = 2 * (picking + 1)
        out["measured_ratio_to_cluster"] = round(out["forest_ms"]["median"] / max(out["cluster_ms"]["median"], 1e-9), 2)
        out["forest_wall_below_copy_wall"] = bool(out["forest_wall_ms"]["median"] < out["copy_wall_ms"]["median"])
        out["cluster_wall_below_copy_wall"] = bool(out["cluster_wall_ms"]["median"] < out["copy_wall_ms"]["median"])
        sel.timing(1)
        for _ in range(3):
            sel.spanning_forest(level, to_host=False)
        out["forest_timer_ms"] = round(sel.kernel_ms("forest"), 4)
        sel.timing(0)
        if label in HOST_ROUTE:
            fetch_ms, host_ms, f_host = [], [], None
            for _ in range(host_reps):
                t0 = time.perf_counter()
                rec = sel.fetch()
                fetch_ms.append(1e3 * (time.perf_counter() - t0))
                t0 = time.perf_counter()
                f_host = host_forest(rec, n)
                host_ms.append(1e3 * (time.perf_counter() - t0))
            out["host_fetch_wall_ms"], out["host_scipy_mst_wall_ms"] = med(fetch_ms), med(host_ms)
            out["host_scipy_edges"] = f_host
            out["host_scipy_edges_equal"] = bool(f_host == after["n_edges"]) if cnt and raw["jaccard"].min() > 0 else None
        results.append(out)
    sel.close()
    del keep
    return results


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/forest_bench.json")
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds a workload's child process may take")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        print("RESULT " + json.dumps(bench(args.worker, args.reps, args.host_reps)), flush=True)
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
