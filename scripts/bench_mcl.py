#!/usr/bin/env python3
"""GPU box: Markov clustering of a pass's result list on the device (selhip_ctx_mcl) against the route it
replaces: selhip_ctx_fetch plus the same loop on the host with scipy.sparse.

The lists (scripts/bench_adjacency.py opens them):
  cfg3   the cfg3 smh_a list
  K10    the 10-nearest-neighbour graph of 4 096 genomes
  D4     the dense-sharing list of 4 096 genomes, cut at the 99 % quantile of its values (min_value)

One process per list.  The pass runs once; 3 warm calls; then `--reps` alternating rounds (a fresh seeded order every round) of
  mcl      Selector.mcl(min_value, to_host=False) with the defaults: device ms between two events, wall ms around the call
  copy     the records as they lie, device -> pageable host memory; wall ms
  host     Selector.fetch() plus section 2o's loop in scipy.sparse (`--host-reps` times; its sums are scipy's, not the ordered ones,
           so its labels are compared, not its bits) -- THE YARDSTICK; wall ms
median (min ... max) each.  "met" = mcl's wall median is below the host route's median.

usage: bench_mcl.py [--out profiles/mcl_bench.json] [--only cfg3,K10,D4] [--reps 20] [--host-reps 3] [--limit seconds]
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

from bench_adjacency import open_list  # noqa: E402
from bench_cluster import med  # noqa: E402

WORKLOADS = ("cfg3", "K10", "D4")


def host_mcl(rec, n, cut, r=2.0, K=32, prune=1e-4, max_iters=64, tol=1e-3):
    """section 2o with scipy.sparse: (labels, iterations)"""
    from scipy.sparse import coo_matrix, diags
    from scipy.sparse.csgraph import connected_components
    rec = rec[(rec["jaccard"] >= cut) & (rec["i"] != rec["k"]) & (rec["jaccard"] > 0)]
    A = coo_matrix((rec["jaccard"], (rec["i"], rec["k"])), shape=(n, n)).tocsc()
    A = A.maximum(A.T).tocsc()
    top = A.max(axis=0).toarray().ravel()

    def settle(M):                                                              # the K best of every column, normalised
        M = M.tocsc()
        M.sort_indices()
        ptr, idx, dat = M.indptr, M.indices, M.data
        for j in np.flatnonzero(np.diff(ptr) > K):
            a, b = ptr[j], ptr[j + 1]
            dat[a + np.lexsort((idx[a:b], -dat[a:b]))[K:]] = 0.0
        M.eliminate_zeros()
        return M @ diags(1.0 / np.asarray(M.sum(axis=0)).ravel())

    M = settle(A + diags(np.where(top > 0, top, 1.0)))
    it = 0
    while it < max_iters:
        M = (M @ M).tocsc()
        M.data = M.data * M.data if r == 2.0 else M.data ** r
        cutoff = prune * M.max(axis=0).toarray().ravel()
        M.data[M.data < np.repeat(cutoff, np.diff(M.indptr))] = 0.0
        M.eliminate_zeros()
        M = settle(M)
        it += 1
        chaos = (M.max(axis=0).toarray().ravel() - np.asarray(M.multiply(M).sum(axis=0)).ravel()).max()
        if chaos <= tol:
            break
    return connected_components(M, directed=False)[1], it


def bench(name, reps, host_reps):
    import torch
    import cuda_selection_criteria_amd as pkg
    sel, n, what, keep = open_list(name)
    lib = pkg.hip_lib()
    ptr, cnt = sel.result_device()
    rec = sel.fetch()
    cut = float(np.quantile(rec["jaccard"], 0.99)) if name == "D4" else None
    out = {"workload": name, "n_genomes": n, "pass": what, "records": cnt, "min_value": cut}
    raw = np.empty(cnt, dtype=pkg.PAIR_DTYPE)

    def copy():
        if cnt:
            pkg._lib.check(lib.selhip_memcpy_d2h(raw.ctypes.data, C.c_void_p(ptr), raw.nbytes))

    routes = {"mcl": lambda: sel.mcl(cut, to_host=False), "copy": copy}
    got = routes["mcl"]()
    out.update(n_clusters=got["n_clusters"], iters=got["iters"], chaos=got["chaos"], kclass=sel.get_param("mcl_kclass_last"),
               nnz=sel.adjacency("symmetric", cut, to_torch=False)["nnz"])
    for _ in range(3):
        for f in routes.values():
            f()
    wall, dev = {k: [] for k in routes}, []
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
            if k == "mcl":
                dev.append(a.elapsed_time(b))
    for k, v in wall.items():
        out[f"{k}_wall_ms"] = med(v)
    out["mcl_device_ms"] = med(dev)
    ms = []
    for _ in range(host_reps):
        t0 = time.perf_counter()
        labels, it = host_mcl(sel.fetch(), n, -np.inf if cut is None else cut)
        ms.append(1e3 * (time.perf_counter() - t0))
    out["host_wall_ms"] = med(ms)
    out["host_iters"], out["host_n_clusters"] = int(it), int(labels.max()) + 1 if n else 0
    out["aim"] = "met" if out["mcl_wall_ms"]["median"] < out["host_wall_ms"]["median"] else "missed"
    sel.close()
    del keep
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/mcl_bench.json")
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
