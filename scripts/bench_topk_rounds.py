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

usage: bench_topk_rounds.py [--out profiles/topk_rounds_bench.json] [--only D4,D16,D46] [--reps 7] [--limit seconds per workload]
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


def report(r):
    print(json.dumps({k: r[k] for k in ("workload", "n_genomes", "m", "top_k", "pairs")}), flush=True)
    for v, d in r["variants"].items():
        print(f"  {v}: {json.dumps(d)}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/topk_rounds_bench.json")
    ap.add_argument("--only", default="D4,D16,D46")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=240, help="seconds a workload's child process may take")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        print("RESULT " + json.dumps(bench(args.worker, args.reps)), flush=True)
        return 0
    results = []
    for name in args.only.split(","):
        # a fresh child process per workload, under its own time limit; nothing more is started after one that failed
        child = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, __file__, "--worker", name, "--reps", str(args.reps)],
                               stdout=subprocess.PIPE, text=True)
        line = next((ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if child.returncode != 0 or line is None:
            print(f"workload {name} ended with status {child.returncode}: stopping", file=sys.stderr, flush=True)
            return 1
        r = json.loads(line[len("RESULT "):])
        results.append(r)
        report(r)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": "MI355X", "workloads": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
