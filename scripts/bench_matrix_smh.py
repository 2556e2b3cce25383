#!/usr/bin/env python3
"""GPU box: the SuperMinHash measures of the dense matrix (Selector.matrix / query_matrix with measure "smh_matches", DESIGN.md
section 14) against the route that existed before them -- selhip_smh_match_counts over the explicit list of ALL pairs, then a scatter
of the counts into the array.  The workloads are those of bench_matrix.py:

  M1  cfg3, 10 000 genomes (1.0e8 cells, 5.0e7 pairs)        M3  query matrix: 1 000 queries x 50 000 database genomes (5.0e7 cells)
  M2  the first 4 096 genomes of cfg3 (1.7e7 cells)

Per workload, in ONE process, `--reps` alternating rounds of the variants (a fresh seeded order every round), each timed with device
events around the call; median (min ... max):
  smh_f64, smh_f32       the bucket-match matrix into a preallocated tensor (the default form of a self matrix: every pair once, mirrored)
  smh_f64_upper          self matrices: the same without the mirrored stores ("matrix_mirror" = 0) -- their cost
  smh_f64_square         self matrices: the whole square computed, no mirror ("matrix_smh_form" = 3)
  pairlist_scatter       the yardstick: one selhip_smh_match_counts call over the prebuilt list of all pairs (i < k for a self matrix,
                         every (query, database) pair for a query matrix; building the list is NOT timed) and the scatter of its int32
                         counts into the f64 array (both triangles and the diagonal for a self matrix), as torch index operations
  hll_f64                for context only: the HLL Jaccard matrix of the same set (another estimator)
Afterwards the kernels alone under selhip_ctx_timing(2) (mean of 10): "matrix_smh" per variant, "matrix", and for the self workloads one
ALGO_STREAM stage-1 launch over the same pairs ("stage1": the same loads and compares per pair, a band fold in place of the count).
The condition recorded: smh_f64 (device) <= pairlist_scatter.  The two routes' arrays are compared once.

usage: bench_matrix_smh.py [--out profiles/matrix_smh_bench.json] [--only M1,M2,M3] [--reps 20]
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
    "M1": ("cfg3", C["cfg3"], 10_000, 0),
    "M2": ("cfg3[:4096]", C["cfg3"], 4_096, 0),
    "M3": ("W1", C["cfg4"], 50_000, 1_000),
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
    label, gen, n_d, n_q = WORKLOADS[name]
    n = n_d + n_q
    cfg = SynthConfig(f"{name}:{gen.name}", n, gen.m, gen.tau, gen.seed ^ (0x0051 if n_q else 0), p_aux=0, cluster_size=gen.cluster_size,
                      mode=gen.mode, n_sh_lo=gen.n_sh_lo, n_sh_hi=gen.n_sh_hi)
    hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg)
    m = gen.m
    out = {"workload": name, "set": label, "n_genomes": n_d, "n_queries": n_q, "m": m}
    lib = pkg.hip_lib()
    with pkg.Selector(0) as sel:
        if n_q:
            is_q = np.zeros(n, dtype=bool)
            is_q[np.random.default_rng(cfg.seed).choice(n, n_q, replace=False)] = True
            mq = torch.from_numpy(is_q).to(hll_t.device)
            sel.attach(hll_t[~mq].contiguous(), aux_t[~mq].contiguous(), cards_t[~mq].contiguous())
            sel.attach_queries(hll_t[mq].contiguous(), aux_t[mq].contiguous(), cards_t[mq].contiguous())
            shape = (n_q, n_d)
            matrix = sel.query_matrix
            # the explicit list indexes the one array the sets were cut from: (row of query a, row of database genome b)
            rows_q, rows_d = torch.nonzero(mq).flatten().to(torch.int32), torch.nonzero(~mq).flatten().to(torch.int32)
            pi, pk = torch.meshgrid(torch.arange(n_q, device="cuda"), torch.arange(n_d, device="cuda"), indexing="ij")
            pi, pk = pi.flatten(), pk.flatten()
            pairs = torch.stack([rows_q[pi], rows_d[pk]], dim=1).contiguous()
            list_aux = aux_t
        else:
            sel.attach(hll_t, aux_t, cards_t)
            shape = (n_d, n_d)
            matrix = sel.matrix
            tri = torch.triu_indices(n_d, n_d, offset=1, device="cuda")
            pi, pk = tri[0].contiguous(), tri[1].contiguous()
            pairs = torch.stack([pi, pk], dim=1).to(torch.int32).contiguous()
            list_aux = aux_t
        n_pairs = pairs.shape[0]
        out.update({"cells": shape[0] * shape[1], "pairs_in_list": int(n_pairs)})
        buf64 = torch.empty(shape, dtype=torch.float64, device="cuda")
        buf32 = torch.empty(shape, dtype=torch.float32, device="cuda")
        ref64 = torch.empty(shape, dtype=torch.float64, device="cuda")
        counts = torch.empty(n_pairs, dtype=torch.int32, device="cuda")
        diag = torch.arange(n_d, device="cuda")

        def pairlist_scatter():
            pkg._lib.check(lib.selhip_smh_match_counts(list_aux.data_ptr(), m, pairs.data_ptr(), n_pairs, counts.data_ptr(), None))
            v = counts.to(torch.float64)
            ref64[pi, pk] = v
            if not n_q:
                ref64[pk, pi] = v
                ref64[diag, diag] = float(m)

        def switched(param, value, restore):
            def run():
                sel.set_param(param, value)
                try:
                    matrix("smh_matches", out=buf64)
                finally:
                    sel.set_param(param, restore)
            return run

        variants = [("smh_f64", lambda: matrix("smh_matches", out=buf64)), ("smh_f32", lambda: matrix("smh_matches", dtype=torch.float32, out=buf32)),
                    ("pairlist_scatter", pairlist_scatter), ("hll_f64", lambda: matrix("jaccard", out=buf64))]
        if not n_q:
            variants += [("smh_f64_upper", switched("matrix_mirror", 0, 1)), ("smh_f64_square", switched("matrix_smh_form", 3, 1))]
        for _, run in variants:                                                                      # warm-up
            run()
        # the two routes' arrays, compared once (and the square form)
        pairlist_scatter()
        matrix("smh_matches", out=buf64)
        out["identical_to_pairlist"] = bool(torch.equal(buf64, ref64))
        if not n_q:
            switched("matrix_smh_form", 3, 1)()
            out["square_identical"] = bool(torch.equal(buf64, ref64))
        out["path_used"] = sel.get_param("matrix_smh_path_used")
        samples = {v[0]: [] for v in variants}
        order_rng = np.random.default_rng(1)
        for r in range(reps):                                                                        # alternating rounds, a fresh order each
            for vname, run in [variants[j] for j in order_rng.permutation(len(variants))]:
                samples[vname].append(timed(run))
            print(f"  [{name}] round {r + 1} of {reps}", file=sys.stderr, flush=True)
        res = {v: summary(s) for v, s in samples.items()}
        # the kernels alone, under the context's own timers
        for vname, run in variants:
            if vname == "pairlist_scatter":
                continue
            timer = "matrix" if vname == "hll_f64" else "matrix_smh"
            sel.timing(2)
            for _ in range(10):
                run()
            res[vname]["kernel_ms"] = round(sel.kernel_ms(timer), 3)
            sel.timing(0)
        if not n_q:
            r, b = pkg.banding(m, gen.tau)
            sel.set_criterion(pkg.CRIT_SMH_A)
            sel.run(gen.tau, pkg.MODE_SMH, r, b, algo=pkg.ALGO_STREAM, fetch=False)
            sel.timing(2)
            for _ in range(10):
                sel.run(gen.tau, pkg.MODE_SMH, r, b, algo=pkg.ALGO_STREAM, fetch=False)
            out["stream_stage1_kernel_ms"] = round(sel.kernel_ms("stage1"), 3)
            out["stream_pairs"] = int(sel.stats()["evaluated"])
            sel.timing(0)
        else:
            out["stream_stage1_kernel_ms"] = "not measured"
        y = res["pairlist_scatter"]["device_ms"]["median"]
        out["variants"] = res
        out["over_pairlist"] = {v: round(res[v]["device_ms"]["median"] / y, 4) for v in res if v.startswith("smh_")}
        out["not_slower_than_pairlist"] = bool(res["smh_f64"]["device_ms"]["median"] <= y and res["smh_f32"]["device_ms"]["median"] <= y)
        if not n_q:
            out["mirror_cost_ms"] = round(res["smh_f64"]["device_ms"]["median"] - res["smh_f64_upper"]["device_ms"]["median"], 3)
            out["lds_staged_mirror_ms"] = "not measured"                                             # form (ii) of the issue: not built
    del hll_t, aux_t, cards_t, buf64, buf32, ref64, counts, pairs, pi, pk
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/matrix_smh_bench.json")
    ap.add_argument("--only", default="M1,M2,M3")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    results = []
    for name in args.only.split(","):
        r = bench(name, args.reps)
        results.append(r)
        print(json.dumps({k: r.get(k) for k in ("workload", "cells", "path_used", "identical_to_pairlist", "square_identical", "over_pairlist",
                                                "not_slower_than_pairlist", "mirror_cost_ms", "stream_stage1_kernel_ms")}), flush=True)
        for v, d in r["variants"].items():
            print(f"  {v}: device {d['device_ms']} kernel {d.get('kernel_ms', '-')} ms ({d['reps']} reps)", flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": "MI355X", "workloads": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
