#!/usr/bin/env python3
"""GPU box: single-linkage clusters of a pass's result list on the device (selhip_ctx_cluster) against the route
that exists without it: copy the list to the host (16 B per record over PCIe), build the graph there, find its components there.

  cfg3   the smh_a pass of cfg3 (10 000 genomes, m = 512, tau = 0.8): about 45 000 records -- latency-bound
  none4k criterion none at tau = 0.5 on the first 4 096 genomes of cfg3
  D4     the dense-sharing set of scripts/bench_topk_rounds.py, 4 096 genomes, behind `-c smh_c -C 1 -n -h -1 -V smh`: every pair a record
  D16    the same at 16 384 genomes: 1.3e8 records and one giant component -- every hook lands on one root, the contention case

Every workload runs in a child process of its own under its own time limit.  The pass runs once; then `--reps` alternating rounds
(a fresh seeded order every round) of
  device   Selector.cluster(to_host=False): device ms between two events and wall ms around the call
  copy     the records as they lie, device -> pageable host memory, nothing else (selhip_memcpy_d2h of result_device): the cheapest
           form of the fetch the feature exists to avoid; wall ms
median (min ... max) each.  The rest of the host route is timed `--host-reps` times, it being seconds on the large lists:
  fetch    selhip_ctx_fetch (the copy plus its sort by (i, k)); skipped beyond 5e7 records
  host     the components of the fetched records on the host: scipy.sparse.csgraph.connected_components where scipy imports, else a
           numpy label propagation; the report says which
The labels of the device are compared with the host's in every workload (same partition, and the device's label is the smallest
member).  Also: the context's own "cluster" timer (mean of 3), the effective GB/s over the list, and -- what root contention costs --
the same list cut at its 50 %, 90 % and 99 % value quantiles, where the giant component falls apart: records kept, clusters, device ms.

usage: bench_cluster.py [--out profiles/cluster_bench.json] [--only cfg3,none4k,D4,D16] [--reps 20] [--host-reps 3] [--limit seconds]
"""
import argparse
import ctypes as C
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

WORKLOADS = ("cfg3", "none4k", "D4", "D16")
SORTED_FETCH_MAX = 50_000_000


def med(samples):
    return {"median": round(statistics.median(samples), 4), "min": round(min(samples), 4), "max": round(max(samples), 4)}


def open_pass(name):
    """(selector with the pass's list on the device, n, what ran, the tensors it reads)"""
    import cuda_selection_criteria_amd as pkg
    sel = pkg.Selector(0)
    if name in ("cfg3", "none4k"):
        cfg = pkg.SYNTH_CONFIGS["cfg3"] if name == "cfg3" else pkg.SYNTH_CONFIGS["cfg3"].scaled(4096)
        hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg, device=0)
        sel.attach(hll_t, aux_t, cards_t)
        if name == "cfg3":
            r, b = pkg.banding(cfg.m, cfg.tau)
            sel.run(cfg.tau, pkg.MODE_CB_SMH, r, b, fetch=False)
            what = f"smh_a, tau {cfg.tau}, CB mode, {r} x {b} bands"
        else:
            sel.set_criterion(pkg.CRIT_NONE)
            sel.run(0.5, pkg.MODE_CB_SMH, 1, 1, fetch=False)
            what = "criterion none, tau 0.5, CB mode"
        return sel, cfg.n_genomes, what, (hll_t, aux_t, cards_t)
    from bench_topk_rounds import dense_set
    n = 4096 if name == "D4" else 16384
    keep = dense_set(n, 512, 19)
    sel.attach(*keep)
    sel.set_criterion(pkg.CRIT_SMH_C)
    sel.set_min_matches(1)
    sel.set_estimator("smh")
    sel.run(-1.0, pkg.MODE_SMH, 1, 1, fetch=False)
    return sel, n, "dense-sharing set, -c smh_c -C 1 -n -h -1 -V smh", keep


def host_components(rec, n):
    """(labels [n] = smallest member of the component, which implementation)"""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        g = coo_matrix((np.ones(len(rec), dtype=np.int8), (rec["i"], rec["k"])), shape=(n, n))
        _, comp = connected_components(g, directed=False)
        first = np.full(comp.max() + 1 if n else 0, n, dtype=np.int64)
        np.minimum.at(first, comp, np.arange(n))
        return first[comp].astype(np.int32), "scipy.sparse.csgraph.connected_components"
    except ImportError:
        lab = np.arange(n, dtype=np.int64)
        i, k = rec["i"].astype(np.int64), rec["k"].astype(np.int64)
        while True:
            lo = np.minimum(lab[i], lab[k])
            new = lab.copy()
            np.minimum.at(new, i, lo)
            np.minimum.at(new, k, lo)
            new = new[new]
            if np.array_equal(new, lab):
                return lab.astype(np.int32), "numpy label propagation"
            lab = new


def bench(name, reps, host_reps):
    import torch
    import cuda_selection_criteria_amd as pkg
    sel, n, what, keep = open_pass(name)
    lib = pkg.hip_lib()
    ptr, cnt = sel.result_device()
    out = {"workload": name, "n_genomes": n, "pass": what, "records": cnt, "list_bytes": 16 * cnt, "last_attempts": sel.last_attempts()}
    raw = np.empty(cnt, dtype=pkg.PAIR_DTYPE)

    def device():
        return sel.cluster(to_host=False)

    def copy():
        if cnt:
            pkg._lib.check(lib.selhip_memcpy_d2h(raw.ctypes.data, C.c_void_p(ptr), raw.nbytes))

    device(), copy()
    samples = {"device_ms": [], "device_wall_ms": [], "copy_wall_ms": []}
    rng = np.random.default_rng(1)
    for r in range(reps):
        for which in rng.permutation(2):
            torch.cuda.synchronize()
            if which == 0:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                a.record()
                device()
                b.record()
                torch.cuda.synchronize()
                samples["device_wall_ms"].append(1e3 * (time.perf_counter() - t0))
                samples["device_ms"].append(a.elapsed_time(b))
            else:
                t0 = time.perf_counter()
                copy()
                samples["copy_wall_ms"].append(1e3 * (time.perf_counter() - t0))
        if (r + 1) % 5 == 0:
            print(f"  [{name}] round {r + 1} of {reps}", file=sys.stderr, flush=True)
    for k, v in samples.items():
        out[k] = med(v)
    out["effective_gb_per_s"] = round(16 * cnt / (1e6 * max(out["device_ms"]["median"], 1e-9)), 1)
    out["copy_gb_per_s"] = round(16 * cnt / (1e6 * max(out["copy_wall_ms"]["median"], 1e-9)), 1)
    out["device_wall_below_copy_wall"] = bool(out["device_wall_ms"]["median"] < out["copy_wall_ms"]["median"])
    # the rest of the host route, a few times
    fetch_ms, host_ms, impl, host_lab = [], [], None, None
    for _ in range(host_reps):
        if cnt <= SORTED_FETCH_MAX:
            t0 = time.perf_counter()
            sel.fetch()
            fetch_ms.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        host_lab, impl = host_components(raw, n)
        host_ms.append(1e3 * (time.perf_counter() - t0))
        print(f"  [{name}] host route {len(host_ms)} of {host_reps}", file=sys.stderr, flush=True)
    out["fetch_sorted_wall_ms"] = med(fetch_ms) if fetch_ms else None
    out["host_components_wall_ms"] = med(host_ms)
    out["host_components_by"] = impl
    got = device()
    out["n_clusters"] = got["n_clusters"]
    out["labels_equal_host"] = bool(np.array_equal(got["labels"].cpu().numpy(), host_lab))
    out["largest_cluster"] = int(got["sizes"].max().item()) if got["n_clusters"] else 0
    # the context's own timer
    sel.timing(1)
    for _ in range(3):
        device()
    out["cluster_timer_ms"] = round(sel.kernel_ms("cluster"), 4)
    sel.timing(0)
    # the same list cut where the giant component falls apart
    out["cuts"] = []
    if cnt:
        for q in (0.5, 0.9, 0.99):
            level = float(np.quantile(raw["jaccard"], q))
            ms = []
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                res = sel.cluster(level, to_host=False)
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            out["cuts"].append({"quantile": q, "min_value": level, "records_kept": int((raw["jaccard"] >= level).sum()), "n_clusters": res["n_clusters"],
                                "largest_cluster": int(res["sizes"].max().item()), "device_ms": med(ms)})
    sel.close()
    del keep
    return out


def report(r):
    print(json.dumps({k: v for k, v in r.items() if k != "cuts"}), flush=True)
    for c in r["cuts"]:
        print(f"  cut {json.dumps(c)}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/cluster_bench.json")
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
        r = json.loads(line[len("RESULT "):])
        results.append(r)
        report(r)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": "MI355X", "reps": args.reps, "host_reps": args.host_reps, "workloads": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
