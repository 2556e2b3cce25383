#!/usr/bin/env python3
"""GPU box: the smh_c passes under the SuperMinHash estimator (selhip_ctx_set_estimator) against the same passes
under the HLL estimator and against criterion none.  The workloads of scripts/bench_smhc.py, c_min = min_matches(m, tau):

  S1  cfg3, 10 000 genomes (5.0e7 pairs)                     S3  query pass: 1 000 queries x 50 000 database genomes (5.0e7 pairs)
  S2  the first 4 096 genomes of cfg3 (8.4e6 pairs)
  KNN the first 4 096 genomes of cfg3, every genome's 10 nearest neighbours: `-c none -n -h -1 -K 10` (the route there was) against
      `-c smh_c -C 1 -n -h -1 -K 10 -V smh`; the cut is part of what is timed

Every workload runs in a child process of its own under its own time limit.  Per workload and mode (CB bound on / off; KNN: off), `--reps`
alternating rounds of the variants (a fresh seeded order every round), each timed with device events around the call; median (min ... max):
  smh_v      the smh_c pass under SELHIP_ESTIMATOR_SMH (records left on the device)
  smh_c_hll  the same pass under SELHIP_ESTIMATOR_HLL, at the same c_min
  none       the pass under criterion none with the same mode and tau
The condition recorded: smh_v's median <= smh_c_hll's median + smh_c_hll's own (max - min) of the same run -- it runs the same count and
strictly fewer launches behind it.  Record counts of all three, and the count kernel alone under selhip_ctx_timing(2) (mean of 10).

usage: bench_smhv.py [--out profiles/smhv_bench.json] [--only S1,S2,S3,KNN] [--reps 20] [--limit seconds per workload]
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

WORKLOADS = {                                   # set, generator, genomes of the (database) set, queries, top-k
    "S1": ("cfg3", "cfg3", 10_000, 0, 0),
    "S2": ("cfg3[:4096]", "cfg3", 4_096, 0, 0),
    "S3": ("1000 x 50000", "cfg4", 50_000, 1_000, 0),
    "KNN": ("cfg3[:4096], 10 nearest neighbours", "cfg3", 4_096, 0, 10),
}


def timed(run):
    """device ms between two events around the call"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def summary(samples):
    return {"reps": len(samples), "device_ms": {"median": round(statistics.median(samples), 3), "min": round(min(samples), 3), "max": round(max(samples), 3)}}


def bench(name, reps):
    import torch
    import cuda_selection_criteria_amd as pkg
    from cuda_selection_criteria_amd import SynthConfig
    label, gen_name, n_d, n_q, top_k = WORKLOADS[name]
    gen = pkg.SYNTH_CONFIGS[gen_name]
    n = n_d + n_q
    cfg = SynthConfig(f"{name}:{gen.name}", n, gen.m, gen.tau, gen.seed ^ (0x0051 if n_q else 0), p_aux=0, cluster_size=gen.cluster_size,
                      mode=gen.mode, n_sh_lo=gen.n_sh_lo, n_sh_hi=gen.n_sh_hi)
    hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg)
    m = gen.m
    tau, c_min = (-1.0, 1) if top_k else (gen.tau, pkg.min_matches(m, gen.tau))
    out = {"workload": name, "set": label, "n_genomes": n_d, "n_queries": n_q, "m": m, "tau": tau, "c_min": c_min, "top_k": top_k, "modes": {}}
    with pkg.Selector(0) as sel:
        if n_q:
            is_q = np.zeros(n, dtype=bool)
            is_q[np.random.default_rng(cfg.seed).choice(n, n_q, replace=False)] = True
            mq = torch.from_numpy(is_q).to(hll_t.device)
            sel.attach(hll_t[~mq].contiguous(), aux_t[~mq].contiguous(), cards_t[~mq].contiguous())
            sel.attach_queries(hll_t[mq].contiguous(), aux_t[mq].contiguous(), cards_t[mq].contiguous())
            run_pass = lambda mode: sel.run_queries(tau, mode, 1, 1, fetch=False)                     # noqa: E731
        else:
            sel.attach(hll_t, aux_t, cards_t)
            if top_k:
                sel.set_allpairs_topk(top_k)
            run_pass = lambda mode: sel.run(tau, mode, 1, 1, fetch=False)                             # noqa: E731
        sel.set_min_matches(c_min)

        def variant(criterion, estimator):
            def run(mode):
                sel.set_estimator("hll")
                sel.set_criterion(criterion)
                sel.set_estimator(estimator)
                run_pass(mode)
            return run

        runs = {"smh_v": variant(pkg.CRIT_SMH_C, "smh"), "smh_c_hll": variant(pkg.CRIT_SMH_C, "hll"), "none": variant(pkg.CRIT_NONE, "hll")}
        modes = (("nocb", pkg.MODE_SMH),) if top_k else (("cb", pkg.MODE_CB_SMH), ("nocb", pkg.MODE_SMH))
        for mode_name, mode in modes:
            counts = {}
            for vname, run in runs.items():                                                          # warm-up: the lists take their sizes
                run(mode)
                run(mode)
                counts[vname] = dict(sel.stats(), kept=sel.result_count())
            assert sel.get_param("smhc_path_used") == 1
            samples = {v: [] for v in runs}
            order_rng = np.random.default_rng(1)
            names = list(runs)
            for r in range(reps):                                                                    # alternating rounds, a fresh order each
                for vname in [names[j] for j in order_rng.permutation(len(names))]:
                    samples[vname].append(timed(lambda: runs[vname](mode)))
                print(f"  [{name} {mode_name}] round {r + 1} of {reps}", file=sys.stderr, flush=True)
            res = {v: summary(s) for v, s in samples.items()}
            for vname in ("smh_v", "smh_c_hll"):                                                     # the count kernel alone, under the context's own timer
                runs[vname](mode)
                sel.timing(2)
                for _ in range(10):
                    runs[vname](mode)
                res[vname]["stage1_kernel_ms"] = round(sel.kernel_ms("stage1"), 4)
                sel.timing(0)
            v, h = res["smh_v"]["device_ms"], res["smh_c_hll"]["device_ms"]
            bound = h["median"] + (h["max"] - h["min"])
            out["modes"][mode_name] = {"counts": counts, "variants": res, "bound_ms": round(bound, 3),
                                       "smh_v_over_smh_c_hll": round(v["median"] / h["median"], 5),
                                       "smh_v_over_none": round(v["median"] / res["none"]["device_ms"]["median"], 5),
                                       "within_bound": bool(v["median"] <= bound)}
        sel.set_estimator("hll")
    return out


def report(r):
    print(json.dumps({k: r.get(k) for k in ("workload", "set", "m", "tau", "c_min", "top_k")}), flush=True)
    for mode_name, d in r["modes"].items():
        print(f"  {mode_name}: smh_v / smh_c_hll {d['smh_v_over_smh_c_hll']}  smh_v / none {d['smh_v_over_none']}  bound {d['bound_ms']} ms  within {d['within_bound']}", flush=True)
        for v, x in d["variants"].items():
            c = d["counts"][v]
            print(f"    {v}: device {x['device_ms']} stage1 kernel {x.get('stage1_kernel_ms', '-')} ms; evaluated {c['evaluated']} survivors {c['survivors']} "
                  f"records {c['selected']} kept {c['kept']}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/smhv_bench.json")
    ap.add_argument("--only", default="S1,S2,S3,KNN")
    ap.add_argument("--reps", type=int, default=20)
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
