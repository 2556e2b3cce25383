#!/usr/bin/env python3
"""GPU box: the max-containment measure of the passes (selhip_ctx_set_measure) and the containment / intersection matrices (DESIGN.md
section 16) against their Jaccard twins.  The work of a pair is identical except for one divide and one compare, so every containment
variant is measured against the J variant of the same run: its median may exceed the J median by no more than J's own max - min.

  S1  cfg3, 10 000 genomes (5.0e7 pairs)                     S3  query pass: 1 000 queries x 50 000 database genomes (5.0e7 pairs)
  S2  the first 4 096 genomes of cfg3 (8.4e6 pairs)

Per workload, in ONE process, `--reps` alternating rounds of the variants (a fresh seeded order every round), each timed with device
events around the call; median (min ... max):
  none / jaccard, none / max_containment        the exhaustive pass in MODE_SMH at tau = 0.8 (records left on the device)
  smh_a / jaccard, smh_a / max_containment      the smh_a pass, same mode and tau, banding of (m, tau)
  matrix jaccard | intersection | containment | max_containment      the f64 matrix (a query matrix for S3) into one buffer
and the record counts of the four passes.

usage: bench_containment.py [--out profiles/containment_bench.json] [--only S1,S2,S3] [--reps 20]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import cuda_selection_criteria_amd as pkg  # noqa: E402
from cuda_selection_criteria_amd import SynthConfig  # noqa: E402

C = pkg.SYNTH_CONFIGS
WORKLOADS = {                                   # set, genomes of the (database) set, queries
    "S1": ("cfg3", C["cfg3"], 10_000, 0),
    "S2": ("cfg3[:4096]", C["cfg3"], 4_096, 0),
    "S3": ("1000 x 50000", C["cfg4"], 50_000, 1_000),
}
TAU = 0.8
PASS_MEASURES = ("jaccard", "max_containment")
MATRIX_MEASURES = ("jaccard", "intersection", "containment", "max_containment")


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
    return {"reps": len(samples), "device_ms": {"median": round(statistics.median(samples), 4), "min": round(min(samples), 4), "max": round(max(samples), 4)}}


def against(res, variant, yardstick):
    """the rule of the measurements here: the variant's median is no higher than the yardstick's plus the yardstick's own max - min"""
    v, y = res[variant]["device_ms"], res[yardstick]["device_ms"]
    return {"variant": variant, "yardstick": yardstick, "ratio_of_medians": round(v["median"] / y["median"], 5),
            "allowed_ms": round(y["median"] + (y["max"] - y["min"]), 4), "within": bool(v["median"] <= y["median"] + (y["max"] - y["min"]))}


def bench(name, reps):
    import torch
    label, gen, n_d, n_q = WORKLOADS[name]
    n = n_d + n_q
    cfg = SynthConfig(f"{name}:{gen.name}", n, gen.m, gen.tau, gen.seed ^ (0x0051 if n_q else 0), p_aux=0, cluster_size=gen.cluster_size,
                      mode=gen.mode, n_sh_lo=gen.n_sh_lo, n_sh_hi=gen.n_sh_hi)
    hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg)
    m = gen.m
    r, b = pkg.banding(m, TAU)
    out = {"workload": name, "set": label, "n_genomes": n_d, "n_queries": n_q, "m": m, "tau": TAU, "n_rows": r, "n_bands": b}
    with pkg.Selector(0) as sel:
        if n_q:
            is_q = np.zeros(n, dtype=bool)
            is_q[np.random.default_rng(cfg.seed).choice(n, n_q, replace=False)] = True
            mq = torch.from_numpy(is_q).to(hll_t.device)
            sel.attach(hll_t[~mq].contiguous(), aux_t[~mq].contiguous(), cards_t[~mq].contiguous())
            sel.attach_queries(hll_t[mq].contiguous(), aux_t[mq].contiguous(), cards_t[mq].contiguous())
            shape, matrix = (n_q, n_d), sel.query_matrix
            run_pass = lambda rr, bb: sel.run_queries(TAU, pkg.MODE_SMH, rr, bb, fetch=False)        # noqa: E731
        else:
            sel.attach(hll_t, aux_t, cards_t)
            shape, matrix = (n_d, n_d), sel.matrix
            run_pass = lambda rr, bb: sel.run(TAU, pkg.MODE_SMH, rr, bb, fetch=False)                # noqa: E731
        cells = torch.empty(shape, dtype=torch.float64, device="cuda")

        def a_pass(crit, measure):
            sel.set_criterion(crit)
            sel.set_measure(measure)
            run_pass(*((1, 1) if crit == pkg.CRIT_NONE else (r, b)))

        variants = [(f"{cname}/{meas}", (lambda c=crit, s=meas: a_pass(c, s)))
                    for cname, crit in (("none", pkg.CRIT_NONE), ("smh_a", pkg.CRIT_SMH_A)) for meas in PASS_MEASURES]
        variants += [(f"matrix/{meas}", (lambda s=meas: matrix(s, out=cells))) for meas in MATRIX_MEASURES]
        counts = {}
        for vname, run in variants:                                                              # warm-up: the lists take their sizes
            run()
            run()
            if not vname.startswith("matrix/"):
                st = sel.stats()
                counts[vname] = {"evaluated": st["evaluated"], "survivors": st["survivors"], "records": st["selected"]}
        samples = {v[0]: [] for v in variants}
        order_rng = np.random.default_rng(1)
        for rep in range(reps):                                                                  # alternating rounds, a fresh order each
            for vname, run in [variants[j] for j in order_rng.permutation(len(variants))]:
                samples[vname].append(timed(run))
            print(f"  [{name}] round {rep + 1} of {reps}", file=sys.stderr, flush=True)
        sel.set_measure("jaccard")
        res = {v: summary(s) for v, s in samples.items()}
        out["counts"] = counts
        out["variants"] = res
        out["checks"] = [against(res, "none/max_containment", "none/jaccard"), against(res, "smh_a/max_containment", "smh_a/jaccard")] + \
                        [against(res, f"matrix/{meas}", "matrix/jaccard") for meas in MATRIX_MEASURES[1:]]
    del hll_t, aux_t, cards_t, cells
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/containment_bench.json")
    ap.add_argument("--only", default="S1,S2,S3")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    results = []
    for name in args.only.split(","):
        res = bench(name, args.reps)
        results.append(res)
        print(json.dumps({k: res.get(k) for k in ("workload", "set", "tau", "n_rows", "n_bands")}), flush=True)
        for v, x in res["variants"].items():
            print(f"    {v}: device {x['device_ms']} ({x['reps']} reps) {res['counts'].get(v, '')}", flush=True)
        for chk in res["checks"]:
            print(f"    {chk['variant']} vs {chk['yardstick']}: ratio {chk['ratio_of_medians']} allowed {chk['allowed_ms']} ms within {chk['within']}", flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": "MI355X", "workloads": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
