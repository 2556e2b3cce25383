#!/usr/bin/env python3
"""GPU box: the all-pairs top-k in row rounds (selhip_ctx_set_topk_rounds) against the one-shot route, on a
DENSE-SHARING set: every genome is a copy of one of eight ancestor rows -- themselves half-mutated copies of one root row -- with its
own mutation rate in [0.05, 0.6], so nearly every pair shares buckets and the count varies.  Generated on the device; all-zero HLL rows
(the pass `-c smh_c -C 1 -n -h -1 -K 10 -V smh` reads none).

  D4   4 096 genomes, m = 512       D16  16 384 genomes, m = 512       both routes run: one-shot, -R auto and two explicit R
  D46  46 400 genomes, m = 128      the one-shot route is refused (2 |S| > 2^31 - 1): the refusal is recorded, then -R auto and one explicit R

Every workload runs in a child process of its own under its own time limit.  Every variant has a context of its own, so what it holds on
the device after its warm-up (free device memory before the context minus after) is its own; `--reps` alternating rounds of the variants
(a fresh seeded order every round), each timed to the ranked list on the device: device ms between two events and wall ms around the
call, median (min ... max); the ranked list of every variant is compared with the one-shot's (D46: with -R auto's) in every round.
Also: |S|, the records admitted, the rounds, the records kept, and "stage1" / "topk" under the context's own timer (mean of 3).

`--shapes all`: the rounds at the narrow and the wide rows.  The same generator at n = 16 384, K = 10,
m = 32, 64, 2048, 4096 and R = n (one round: everything is admitted) and 1 024; one child process per (m, R).  One context, three routes:
the pass in rounds on the kernel of m ("new"), the same pass under "smhc_generic" = 1 (the route these m took before) and the one-shot
pass, which runs the emit form of the same kernel.  3 warm calls each, then 20 alternating rounds in a fresh seeded order, device ms as
median (min ... max); the ranked lists of the three must be the same bytes in every round.  The aim of a line at R = n is the one-shot's
median plus its spread (max - min); at R = 1 024 the line records generic / new.  Writes profiles/topk_rounds_shapes_bench.json.

usage: bench_topk_rounds.py [--out profiles/topk_rounds_bench.json] [--only D4,D16,D46] [--reps 7] [--limit seconds per workload]
       bench_topk_rounds.py --shapes all [--out profiles/topk_rounds_shapes_bench.json] [--reps 20] [--limit seconds per line]
"""
import argparse
import hashlib
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

K = 10
WORKLOADS = {                                   # genomes, m, variants (0 = one-shot), whether the one-shot route is expected to be refused
    "D4": (4_096, 512, (0, "auto", 512, 64), False),
    "D16": (16_384, 512, (0, "auto", 1024, 256), False),
    "D46": (46_400, 128, (0, "auto", 512), True),
}


def dense_set(n, m, seed):
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    big = lambda *s: torch.randint(-(1 << 62), 1 << 62, s, generator=g, device="cuda", dtype=torch.int64)          # noqa: E731
    uni = lambda *s: torch.rand(*s, generator=g, device="cuda")                                                     # noqa: E731
    root = big(m)
    anc = torch.where(uni(8, m) < 0.5, root.expand(8, m), big(8, m))
    a = torch.randint(0, 8, (n,), generator=g, device="cuda")
    rate = 0.05 + 0.55 * uni(n)
    aux = torch.where(uni(n, m) < rate[:, None], big(n, m), anc[a]).contiguous()
    cards = torch.linspace(1e6, 5e6, n, dtype=torch.float64, device="cuda")
    hll = torch.zeros(n, 1 << 14, dtype=torch.uint8, device="cuda")
    return hll, aux, cards


def free_bytes():
    import torch
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def med(samples):
    return {"median": round(statistics.median(samples), 3), "min": round(min(samples), 3), "max": round(max(samples), 3)}


def bench(name, reps):
    import torch
    import cuda_selection_criteria_amd as pkg
    n, m, variants, refused = WORKLOADS[name]
    hll_t, aux_t, cards_t = dense_set(n, m, 19)
    out = {"workload": name, "n_genomes": n, "m": m, "top_k": K, "pairs": n * (n - 1) // 2, "variants": {}}
    ctx, run, digest = {}, {}, {}

    def open_variant(v):
        before = free_bytes()
        sel = pkg.Selector(0)
        sel.attach(hll_t, aux_t, cards_t)
        sel.set_criterion(pkg.CRIT_SMH_C)
        sel.set_min_matches(1)
        sel.set_estimator("smh")
        sel.set_allpairs_topk(K)
        sel.set_topk_rounds(v)
        go = lambda: sel.run(-1.0, pkg.MODE_SMH, 1, 1, fetch=False)                                                   # noqa: E731
        go()
        attempts = sel.last_attempts()
        go()                                                                                                          # the lists have their sizes
        held = before - free_bytes()
        st = sel.stats()
        adm = sel.get_param("topk_admitted_lo") + (sel.get_param("topk_admitted_hi") << 31)
        info = {"rows_per_round": v, "rounds": sel.get_param("topk_rounds_used"), "first_run_attempts": attempts, "selected": st["selected"],
                "admitted": adm if v else st["selected"], "kept": sel.result_count(), "device_bytes_held": int(held)}
        info["admitted_over_selected"] = round(info["admitted"] / max(1, st["selected"]), 5)
        return sel, go, info

    def ranked_digest(sel):
        return hashlib.sha256(sel.fetch_ranked().tobytes()).hexdigest()

    names = []
    for v in variants:
        vname = "one_shot" if v == 0 else f"R_{v}"
        if v == 0 and refused:
            # the one-shot route beyond 2^30 - 1 selected pairs: the refusal, and what the attempt held; its context is closed before the rounds run
            before = free_bytes()
            sel = pkg.Selector(0)
            sel.attach(hll_t, aux_t, cards_t)
            sel.set_criterion(pkg.CRIT_SMH_C)
            sel.set_min_matches(1)
            sel.set_estimator("smh")
            sel.set_allpairs_topk(K)
            t0 = time.perf_counter()
            try:
                sel.run(-1.0, pkg.MODE_SMH, 1, 1, fetch=False)
                out["variants"][vname] = {"refused": False}
            except pkg.SelhipError as e:
                out["variants"][vname] = {"refused": True, "message": str(e), "wall_ms_to_refusal": round(1e3 * (time.perf_counter() - t0), 1),
                                          "device_bytes_held": int(before - free_bytes())}
            sel.close()
            continue
        ctx[vname], run[vname], out["variants"][vname] = open_variant(v)
        names.append(vname)
    ref = names[0]
    samples = {v: {"device": [], "wall": []} for v in names}
    order_rng = np.random.default_rng(1)
    for r in range(reps):
        for vname in [names[j] for j in order_rng.permutation(len(names))]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            run[vname]()
            b.record()
            torch.cuda.synchronize()
            samples[vname]["wall"].append(1e3 * (time.perf_counter() - t0))
            samples[vname]["device"].append(a.elapsed_time(b))
            digest[vname] = ranked_digest(ctx[vname])
        assert all(digest[v] == digest[ref] for v in names), (r, digest)                    # the same ranked list, byte for byte, every round
        print(f"  [{name}] round {r + 1} of {reps}", file=sys.stderr, flush=True)
    for vname in names:
        sel = ctx[vname]
        sel.timing(1)
        for _ in range(3):
            run[vname]()
        d = out["variants"][vname]
        d["device_ms"], d["wall_ms"] = med(samples[vname]["device"]), med(samples[vname]["wall"])
        d["stage1_ms"], d["topk_ms"] = round(sel.kernel_ms("stage1"), 4), round(sel.kernel_ms("topk"), 4)
        d["list_equals"] = ref
        sel.timing(0)
        sel.close()
    return out


SHAPES_N = 16_384
SHAPES = [(m, r) for m in (32, 64, 2048, 4096) for r in (SHAPES_N, 1024)]


def bench_shape(m, rows, reps):
    """one line of `--shapes all`: the three routes on one context"""
    import torch
    import cuda_selection_criteria_amd as pkg
    n = SHAPES_N
    hll_t, aux_t, cards_t = dense_set(n, m, 19)
    sel = pkg.Selector(0)
    sel.attach(hll_t, aux_t, cards_t)
    sel.set_criterion(pkg.CRIT_SMH_C)
    sel.set_min_matches(1)
    sel.set_estimator("smh")
    sel.set_allpairs_topk(K)
    routes = {"new": (rows, 0), "generic": (rows, 1), "one_shot": (0, 0)}          # (rows per round, "smhc_generic")

    def go(route):
        per_round, generic = routes[route]
        sel.set_topk_rounds(per_round)
        sel.set_param("smhc_generic", generic)
        sel.run(-1.0, pkg.MODE_SMH, 1, 1, fetch=False)
        sel.set_param("smhc_generic", 0)

    out = {"m": m, "n_genomes": n, "top_k": K, "rows_per_round": rows, "routes": {}}
    for route in routes:
        for _ in range(3):
            go(route)
        st = sel.stats()
        adm = sel.get_param("topk_admitted_lo") + (sel.get_param("topk_admitted_hi") << 31)
        out["routes"][route] = {"kernel_used": sel.get_param("smhc_kernel_used"), "rounds": sel.get_param("topk_rounds_used"), "selected": st["selected"],
                                "admitted": adm if routes[route][0] else st["selected"], "kept": sel.result_count()}
    samples = {route: [] for route in routes}
    order_rng = np.random.default_rng(1)
    for r in range(reps):
        digest = {}
        for route in [list(routes)[j] for j in order_rng.permutation(len(routes))]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            go(route)
            b.record()
            torch.cuda.synchronize()
            samples[route].append(a.elapsed_time(b))
            digest[route] = hashlib.sha256(sel.fetch_ranked().tobytes()).hexdigest()
        assert len(set(digest.values())) == 1, (r, digest)                                  # the same ranked list, byte for byte, every round
        print(f"  [m = {m}, R = {rows}] round {r + 1} of {reps}", file=sys.stderr, flush=True)
    for route in routes:
        out["routes"][route]["device_ms"] = med(samples[route])
    ms = {route: out["routes"][route]["device_ms"] for route in routes}
    out["generic_over_new"] = round(ms["generic"]["median"] / ms["new"]["median"], 2)
    out["lists_identical"] = True
    if rows == n:
        out["aim_ms"] = round(ms["one_shot"]["median"] + ms["one_shot"]["max"] - ms["one_shot"]["min"], 3)
        out["aim_met"] = ms["new"]["median"] <= out["aim_ms"]
    sel.close()
    return out


def report(r):
    print(json.dumps({k: r[k] for k in ("workload", "n_genomes", "m", "top_k", "pairs")}), flush=True)
    for v, d in r["variants"].items():
        print(f"  {v}: {json.dumps(d)}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="profiles/topk_rounds_bench.json, with --shapes profiles/topk_rounds_shapes_bench.json")
    ap.add_argument("--only", default="D4,D16,D46")
    ap.add_argument("--shapes", choices=["all"], default=None, help="the rounds at m = 32, 64, 2048, 4096 instead of the workloads")
    ap.add_argument("--reps", type=int, default=None, help="alternating rounds: 7, with --shapes 20")
    ap.add_argument("--limit", type=int, default=None, help="seconds a workload's child process may take: 240, a line of --shapes 400")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    reps = args.reps or (20 if args.shapes else 7)
    limit = args.limit or (400 if args.shapes else 240)
    out_path = Path(args.out or ("profiles/topk_rounds_shapes_bench.json" if args.shapes else "profiles/topk_rounds_bench.json"))
    if args.worker and args.shapes:
        m, rows = (int(x) for x in args.worker.split(":"))
        print("RESULT " + json.dumps(bench_shape(m, rows, reps)), flush=True)
        return 0
    if args.worker:
        print("RESULT " + json.dumps(bench(args.worker, reps)), flush=True)
        return 0
    results = []
    if args.shapes:
        for m, rows in SHAPES:
            # a fresh child process per line, under its own time limit; nothing more is started after one that failed
            child = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, __file__, "--shapes", "all", "--worker", f"{m}:{rows}", "--reps", str(reps)],
                                   stdout=subprocess.PIPE, text=True)
            line = next((ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")), None)
            if child.returncode != 0 or line is None:
                print(f"line m = {m}, R = {rows} ended with status {child.returncode}: stopping", file=sys.stderr, flush=True)
                return 1
            results.append(json.loads(line[len("RESULT "):]))
            print(json.dumps(results[-1]), flush=True)
            out_path.parent.mkdir(parents=True, exist_ok=True)
            out_path.write_text(json.dumps({"device": "MI355X", "lines": results}, indent=1) + "\n")
        return 0
    for name in args.only.split(","):
        # a fresh child process per workload, under its own time limit; nothing more is started after one that failed
        child = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, __file__, "--worker", name, "--reps", str(reps)],
                               stdout=subprocess.PIPE, text=True)
        line = next((ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if child.returncode != 0 or line is None:
            print(f"workload {name} ended with status {child.returncode}: stopping", file=sys.stderr, flush=True)
            return 1
        r = json.loads(line[len("RESULT "):])
        results.append(r)
        report(r)
        out_path.parent.mkdir(parents=True, exist_ok=True)
        out_path.write_text(json.dumps({"device": "MI355X", "workloads": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
