#!/usr/bin/env python3
"""GPU box: the dense similarity matrix (Selector.matrix / query_matrix) against the route that existed before
it -- a criterion none pass without the CB bound and with tau = -1, then fetch and a host scatter into a matrix.

  M1  cfg3, 10 000 genomes (1.0e8 cells, 5.0e7 pairs)        M3  query matrix: 1 000 queries x 50 000 database genomes (5.0e7 cells;
  M2  the first 4 096 genomes of cfg3 (1.7e7 cells)              the sets of bench_exhaustive.py's E4)

Per workload, in ONE process, `--reps` alternating rounds of the variants (in a fresh seeded order every round), each timed with device events around the synchronous call
and with the wall clock; median (min ... max):
  matrix_f64, matrix_f32   the Jaccard matrix into a preallocated tensor
  matrix_f64_upper         self matrices only: the same call without the mirrored stores ("matrix_mirror" = 0) -- their cost
  pass_none                (a) the criterion none pass (MODE_SMH, tau = -1, fused kernel) alone, records left on the device
  pass_fetch_scatter       (b) the same pass, fetch (sorted on the host) and a numpy scatter into an n x n (n_Q x n_D) array
The expectation recorded: matrix_f64 (device) <= pass_none median * (1 + (max - min) / median of pass_none).  Afterwards a few calls of
each kind under selhip_ctx_timing(2): the kernels alone ("matrix", "dense"; mean of 10).  The mirrored stores' cost is matrix_f64 minus
matrix_f64_upper, under each of the two clocks separately.  The off-diagonal cells are compared with the records once.

usage: bench_matrix.py [--out profiles/matrix_bench.json] [--only M1,M2,M3] [--reps 20] [--reps-b 20]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import cuda_selection_criteria_amd as pkg  # noqa: E402
from cuda_selection_criteria_amd import SynthConfig  # noqa: E402

C = pkg.SYNTH_CONFIGS
WORKLOADS = {                                   # set, genomes of the (database) set, queries
    "M1": ("cfg3", C["cfg3"], 10_000, 0),
    "M2": ("cfg3[:4096]", C["cfg3"], 4_096, 0),
    "M3": ("W1", C["cfg4"], 50_000, 1_000),
}


def timed(run):
    """(device ms between two events around the call, wall ms)"""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3


def summary(samples):
    dev, wall = [s[0] for s in samples], [s[1] for s in samples]
    return {"reps": len(samples), "device_ms": {"median": round(statistics.median(dev), 3), "min": round(min(dev), 3), "max": round(max(dev), 3)},
            "wall_ms": {"median": round(statistics.median(wall), 3), "min": round(min(wall), 3), "max": round(max(wall), 3)}}


def bench(name, reps, reps_b):
    import torch
    label, gen, n_d, n_q = WORKLOADS[name]
    n = n_d + n_q
    cfg = SynthConfig(f"{name}:{gen.name}", n, gen.m, gen.tau, gen.seed ^ (0x0051 if n_q else 0), p_aux=0, cluster_size=gen.cluster_size,
                      mode=gen.mode, n_sh_lo=gen.n_sh_lo, n_sh_hi=gen.n_sh_hi)
    hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg)
    out = {"workload": name, "set": label, "n_genomes": n_d, "n_queries": n_q}
    with pkg.Selector(0) as sel:
        if n_q:
            is_q = np.zeros(n, dtype=bool)
            is_q[np.random.default_rng(cfg.seed).choice(n, n_q, replace=False)] = True
            mq = torch.from_numpy(is_q).to(hll_t.device)
            sel.attach(hll_t[~mq].contiguous(), aux_t[~mq].contiguous(), cards_t[~mq].contiguous())
            sel.attach_queries(hll_t[mq].contiguous(), aux_t[mq].contiguous(), cards_t[mq].contiguous())
            shape = (n_q, n_d)
            matrix = sel.query_matrix
            run_pass = lambda fetch: sel.run_queries(-1.0, pkg.MODE_SMH, 1, 1, fetch=fetch)          # noqa: E731
        else:
            sel.attach(hll_t, aux_t, cards_t)
            shape = (n_d, n_d)
            matrix = sel.matrix
            run_pass = lambda fetch: sel.run(-1.0, pkg.MODE_SMH, 1, 1, fetch=fetch)                  # noqa: E731
        sel.set_criterion(pkg.CRIT_NONE)
        out.update({"cells": shape[0] * shape[1], "hll_khi": sel.get_param("hll_khi")})
        buf64 = torch.empty(shape, dtype=torch.float64, device="cuda")
        buf32 = torch.empty(shape, dtype=torch.float32, device="cuda")

        def scatter():
            rec = run_pass(True)
            m = np.full(shape, np.nan)
            m[rec["i"], rec["k"]] = rec["jaccard"]
            if not n_q:
                m[rec["k"], rec["i"]] = rec["jaccard"]
                np.fill_diagonal(m, 1.0)
            return m

        def upper():
            sel.set_param("matrix_mirror", 0)
            try:
                matrix("jaccard", out=buf64)
            finally:
                sel.set_param("matrix_mirror", 1)

        variants = [("matrix_f64", lambda: matrix("jaccard", out=buf64), reps), ("matrix_f32", lambda: matrix("jaccard", dtype=torch.float32, out=buf32), reps),
                    ("pass_none", lambda: run_pass(False), reps), ("pass_fetch_scatter", scatter, reps_b)]
        if not n_q:
            variants.insert(2, ("matrix_f64_upper", upper, reps))
        # warm-up (the pass sizes its result list here), and the two routes' outputs compared once
        for _, run, _ in variants:
            run()
        want = scatter()
        matrix("jaccard", out=buf64)
        got = buf64.cpu().numpy()
        same = (np.isnan(got) & np.isnan(want)) | (got.view(np.uint64) == want.view(np.uint64))
        out["pairs_in_records"] = int(sel.stats()["selected"])
        out["identical_to_records"] = bool(same.all())
        del want, got, same
        samples = {v[0]: [] for v in variants}
        order_rng = np.random.default_rng(1)
        for r in range(max(reps, reps_b)):                                                           # alternating rounds
            # (a fresh seeded order every round: whichever variant runs right behind the seconds of host work of pass_fetch_scatter finds
            # the device idle and pays its ramp -- about 1 ms here -- and under a fixed or a cyclic order that is always the same one)
            for vname, run, cnt in [variants[j] for j in order_rng.permutation(len(variants))]:
                if r < cnt:
                    samples[vname].append(timed(run))
            print(f"  [{name}] round {r + 1} of {max(reps, reps_b)}", file=sys.stderr, flush=True)
        res = {v: summary(s) for v, s in samples.items()}
        # the kernels alone, under the context's own timers
        timed_alone = [("matrix_f64", variants[0][1], "matrix"), ("matrix_f32", variants[1][1], "matrix"), ("pass_none", lambda: run_pass(False), "dense")]
        if not n_q:
            timed_alone.append(("matrix_f64_upper", upper, "matrix"))
        for vname, run, timer in timed_alone:
            sel.timing(2)
            for _ in range(10):
                run()
            res[vname]["kernel_ms"] = round(sel.kernel_ms(timer), 3)
            sel.timing(0)
        a = res["pass_none"]["device_ms"]
        spread = (a["max"] - a["min"]) / a["median"]
        m64 = res["matrix_f64"]["device_ms"]["median"]
        out.update({"variants": res, "pass_none_spread": round(spread, 4), "matrix_over_pass_none": round(m64 / a["median"], 4),
                    "no_worse_than_pass_none": bool(m64 <= a["median"] * (1 + spread)),
                    "matrix_over_fetch_scatter_wall": round(res["matrix_f64"]["wall_ms"]["median"] / res["pass_fetch_scatter"]["wall_ms"]["median"], 5)})
        if not n_q:
            # the mirrored stores, each clock against itself: events around the call, and the context's kernel timer
            out["mirror_cost_ms"] = round(m64 - res["matrix_f64_upper"]["device_ms"]["median"], 3)
            out["mirror_cost_kernel_ms"] = round(res["matrix_f64"]["kernel_ms"] - res["matrix_f64_upper"]["kernel_ms"], 3)
    del hll_t, aux_t, cards_t, buf64, buf32
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/matrix_bench.json")
    ap.add_argument("--only", default="M1,M2,M3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reps-b", type=int, default=20, help="repetitions of pass_fetch_scatter (seconds each at 5e7 records)")
    args = ap.parse_args()
    results = []
    for name in args.only.split(","):
        r = bench(name, args.reps, args.reps_b)
        results.append(r)
        print(json.dumps({k: r.get(k) for k in ("workload", "cells", "identical_to_records", "matrix_over_pass_none", "no_worse_than_pass_none",
                                                "mirror_cost_ms", "matrix_over_fetch_scatter_wall")}), flush=True)
        for v, d in r["variants"].items():
            print(f"  {v}: device {d['device_ms']} wall {d['wall_ms']} kernel {d.get('kernel_ms', '-')} ms ({d['reps']} reps)", flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": "MI355X", "workloads": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
