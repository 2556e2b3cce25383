#!/usr/bin/env python3
"""GPU box: the sparse adjacency of a pass's result list on the device (selhip_ctx_adjacency) against the route it
replaces: selhip_ctx_fetch, the copy of the list plus its sort by (i, k) on the host.

The lists of scripts/bench_cluster.py -- cfg3, none4k, D4, D16 -- and
  K10    the first 4 096 genomes of cfg3 under criterion none at tau = 0.5 with the all-pairs top-k at K = 10: the k-NN list, whose
         mutual neighbours are duplicates in the symmetric form

One process per list.  The pass runs once; 3 warm calls; then `--reps` alternating rounds (a fresh seeded order every round) of
  directed / symmetric   Selector.adjacency(form, to_torch=False): device ms between two events, wall ms around the call
  directed_to_host       the directed call plus the copy of row_ptr, col and val to the host; wall ms
  fetch                  Selector.fetch() -- THE YARDSTICK; wall ms; not timed beyond 5e7 records
  copy                   the records as they lie, device -> pageable host memory; wall ms
  cluster                Selector.cluster(to_host=False), one stream over the records with atomics; device ms (not behind K10: the
                         same numbers as none4k's shorter list would say nothing new)
median (min ... max) each.  Also: the rows in each length class, nnz of both forms, and, where scipy imports, fetch +
scipy.sparse.coo_matrix(...).tocsr() as the full host route (`--host-reps` times).  "met" = directed_to_host's median is no slower than
fetch's median.

usage: bench_adjacency.py [--out profiles/adjacency_bench.json] [--only cfg3,none4k,D4,D16,K10] [--reps 20] [--host-reps 3] [--limit seconds]
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

from bench_cluster import SORTED_FETCH_MAX, med, open_pass  # noqa: E402

WORKLOADS = ("cfg3", "none4k", "D4", "D16", "K10")


def open_list(name):
    import cuda_selection_criteria_amd as pkg
    if name != "K10":
        return open_pass(name)
    cfg = pkg.SYNTH_CONFIGS["cfg3"].scaled(4096)
    keep = pkg.synth_device(cfg, device=0)[:3]
    sel = pkg.Selector(0)
    sel.attach(*keep)
    sel.set_criterion(pkg.CRIT_NONE)
    sel.run(0.5, pkg.MODE_CB_SMH, 1, 1, fetch=False, top_k=10)
    return sel, cfg.n_genomes, "criterion none, tau 0.5, CB mode, all-pairs top-k K = 10", keep


def bench(name, reps, host_reps):
    import torch
    import cuda_selection_criteria_amd as pkg
    sel, n, what, keep = open_list(name)
    lib = pkg.hip_lib()
    ptr, cnt = sel.result_device()
    out = {"workload": name, "n_genomes": n, "pass": what, "records": cnt}
    raw = np.empty(cnt, dtype=pkg.PAIR_DTYPE)
    timed_fetch = cnt <= SORTED_FETCH_MAX

    def to_host():
        got = sel.adjacency("directed", to_torch=False)
        return [got[k].cpu() for k in ("row_ptr", "col", "val")]

    def copy():
        if cnt:
            pkg._lib.check(lib.selhip_memcpy_d2h(raw.ctypes.data, C.c_void_p(ptr), raw.nbytes))

    routes = {"directed": lambda: sel.adjacency("directed", to_torch=False), "symmetric": lambda: sel.adjacency("symmetric", to_torch=False),
              "directed_to_host": to_host, "copy": copy}
    if timed_fetch:
        routes["fetch"] = sel.fetch
    if name != "K10":
        routes["cluster"] = lambda: sel.cluster(to_host=False)
    for form in ("directed", "symmetric"):
        got = routes[form]()
        out[f"nnz_{form}"] = got["nnz"]
        out[f"rows_{form}"] = {"wave": n - sel.get_param("adjacency_mid_rows_last") - sel.get_param("adjacency_long_rows_last"),
                               "block": sel.get_param("adjacency_mid_rows_last"), "long": sel.get_param("adjacency_long_rows_last")}
    for _ in range(3):
        for f in routes.values():
            f()
    wall = {k: [] for k in routes}
    dev = {k: [] for k in ("directed", "symmetric", "cluster") if k in routes}
    rng = np.random.default_rng(1)
    names = list(routes)
    for r in range(reps):
        for j in rng.permutation(len(names)):
            k = names[j]
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            routes[k]()
            b.record()
            torch.cuda.synchronize()
            wall[k].append(1e3 * (time.perf_counter() - t0))
            if k in dev:
                dev[k].append(a.elapsed_time(b))
        if (r + 1) % 5 == 0:
            print(f"  [{name}] round {r + 1} of {reps}", file=sys.stderr, flush=True)
    for k, v in wall.items():
        out[f"{k}_wall_ms"] = med(v)
    for k, v in dev.items():
        out[f"{k}_device_ms"] = med(v)
    out["aim"] = None if not timed_fetch else ("met" if out["directed_to_host_wall_ms"]["median"] <= out["fetch_wall_ms"]["median"] else "missed")
    # the full host route, a few times
    try:
        from scipy.sparse import coo_matrix
        ms = []
        for _ in range(host_reps if timed_fetch else 0):
            t0 = time.perf_counter()
            rec = sel.fetch()
            m = coo_matrix((rec["jaccard"], (rec["i"], rec["k"])), shape=(n, n)).tocsr()
            ms.append(1e3 * (time.perf_counter() - t0))
        out["fetch_scipy_tocsr_wall_ms"] = med(ms) if ms else None
        out["scipy_nnz"] = int(m.nnz) if ms else None
    except ImportError:
        out["fetch_scipy_tocsr_wall_ms"] = "scipy is not installed"
    sel.timing(1)
    for _ in range(3):
        routes["directed"]()
    out["adjacency_timer_ms"] = round(sel.kernel_ms("adjacency"), 4)
    sel.timing(0)
    sel.close()
    del keep
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/adjacency_bench.json")
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
        # a fresh child process per list, under its own time limit; nothing more is started after one that failed
        child = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, __file__, "--worker", name, "--reps", str(args.reps),
                                "--host-reps", str(args.host_reps)], stdout=subprocess.PIPE, text=True)
        line = next((ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if child.returncode != 0 or line is None:
            print(f"list {name} ended with status {child.returncode}: stopping", file=sys.stderr, flush=True)
            return 1
        results.append(json.loads(line[len("RESULT "):]))
        print(json.dumps(results[-1]), flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": "MI355X", "reps": args.reps, "host_reps": args.host_reps, "workloads": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
