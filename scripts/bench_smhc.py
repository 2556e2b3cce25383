#!/usr/bin/env python3
"""GPU box: criterion smh_c (at least c_min equal SuperMinHash buckets) against the routes to the same records
that existed before it.  c_min = min_matches(m, tau): the count at which the SuperMinHash estimate c / m reaches the pass's tau.

  S1  cfg3, 10 000 genomes (5.0e7 pairs)                     S3  query pass: 1 000 queries x 50 000 database genomes (5.0e7 pairs)
  S2  the first 4 096 genomes of cfg3 (8.4e6 pairs)

Per workload and mode (CB bound on / off), in ONE process, `--reps` alternating rounds of the variants (a fresh seeded order every
round), each timed with device events around the call; median (min ... max):
  smh_c          the pass under the criterion (records left on the device)
  none           the pass under criterion none with the same mode and tau: the lower bound of the only earlier route to these records
  none_filter    that route in full: the none pass, the dense SuperMinHash match matrix in f32, and a device-side filter of the none
                 records by their cell (count >= c_min), as torch index operations on a copy of the records
The condition recorded: smh_c's median <= none's median.  smh_c's and none_filter's records are compared once (i, k, J bits).
Afterwards the kernels alone under selhip_ctx_timing(2) (mean of 10): smh_c's "stage1", the match matrix's "matrix_smh" without mirrored
stores ("matrix_mirror" = 0, self workloads) and, for the self workloads, one ALGO_STREAM stage 1 of smh_a over the same set.

usage: bench_smhc.py [--out profiles/smhc_bench.json] [--only S1,S2,S3] [--reps 20]
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


def sorted_records(rec):
    rec = np.ascontiguousarray(rec, dtype=pkg.PAIR_DTYPE)
    return rec[np.lexsort((rec["k"], rec["i"]))]


def bench(name, reps):
    import torch
    label, gen, n_d, n_q = WORKLOADS[name]
    n = n_d + n_q
    cfg = SynthConfig(f"{name}:{gen.name}", n, gen.m, gen.tau, gen.seed ^ (0x0051 if n_q else 0), p_aux=0, cluster_size=gen.cluster_size,
                      mode=gen.mode, n_sh_lo=gen.n_sh_lo, n_sh_hi=gen.n_sh_hi)
    hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg)
    m, tau = gen.m, gen.tau
    c_min = pkg.min_matches(m, tau)
    out = {"workload": name, "set": label, "n_genomes": n_d, "n_queries": n_q, "m": m, "tau": tau, "c_min": c_min, "modes": {}}
    with pkg.Selector(0) as sel:
        if n_q:
            is_q = np.zeros(n, dtype=bool)
            is_q[np.random.default_rng(cfg.seed).choice(n, n_q, replace=False)] = True
            mq = torch.from_numpy(is_q).to(hll_t.device)
            sel.attach(hll_t[~mq].contiguous(), aux_t[~mq].contiguous(), cards_t[~mq].contiguous())
            sel.attach_queries(hll_t[mq].contiguous(), aux_t[mq].contiguous(), cards_t[mq].contiguous())
            shape, matrix = (n_q, n_d), sel.query_matrix
            run_pass = lambda mode: sel.run_queries(tau, mode, 1, 1, fetch=False)                     # noqa: E731
        else:
            sel.attach(hll_t, aux_t, cards_t)
            shape, matrix = (n_d, n_d), sel.matrix
            run_pass = lambda mode: sel.run(tau, mode, 1, 1, fetch=False)                             # noqa: E731
        sel.set_min_matches(c_min)
        cells = torch.empty(shape, dtype=torch.float32, device="cuda")
        filtered = {}

        def smh_c(mode):
            sel.set_criterion(pkg.CRIT_SMH_C)
            run_pass(mode)

        def none(mode):
            sel.set_criterion(pkg.CRIT_NONE)
            run_pass(mode)

        def none_filter(mode):
            none(mode)
            cnt = sel.result_count()
            rec = torch.empty((max(cnt, 1), 4), dtype=torch.int32, device="cuda")                     # {i, k, jaccard (two dwords)} per record
            sel.copy_results_to(rec)
            matrix("smh_matches", dtype=torch.float32, out=cells)
            rec = rec[:cnt]
            keep = cells[rec[:, 0].long(), rec[:, 1].long()] >= float(c_min)
            filtered[mode] = rec[keep]

        for mode_name, mode in (("cb", pkg.MODE_CB_SMH), ("nocb", pkg.MODE_SMH)):
            variants = [("smh_c", lambda: smh_c(mode)), ("none", lambda: none(mode)), ("none_filter", lambda: none_filter(mode))]
            for _, run in variants:                                                                  # warm-up: the lists take their sizes
                run()
                run()
            # the records of the two routes, compared once
            smh_c(mode)
            st = sel.stats()
            direct = sorted_records(sel.fetch())
            assert sel.get_param("smhc_path_used") == 1
            none_filter(mode)
            st_none = sel.stats()
            via = sorted_records(filtered[mode].cpu().numpy().view(pkg.PAIR_DTYPE).reshape(-1))
            same = bool(len(direct) == len(via) and np.array_equal(direct["i"], via["i"]) and np.array_equal(direct["k"], via["k"])
                        and np.array_equal(direct["jaccard"].view(np.uint64), via["jaccard"].view(np.uint64)))
            samples = {v[0]: [] for v in variants}
            order_rng = np.random.default_rng(1)
            for r in range(reps):                                                                    # alternating rounds, a fresh order each
                for vname, run in [variants[j] for j in order_rng.permutation(len(variants))]:
                    samples[vname].append(timed(run))
                print(f"  [{name} {mode_name}] round {r + 1} of {reps}", file=sys.stderr, flush=True)
            res = {v: summary(s) for v, s in samples.items()}
            # the stage-1 kernel alone, under the context's own timer
            sel.set_criterion(pkg.CRIT_SMH_C)
            sel.timing(2)
            for _ in range(10):
                run_pass(mode)
            res["smh_c"]["stage1_kernel_ms"] = round(sel.kernel_ms("stage1"), 4)
            sel.timing(0)
            out["modes"][mode_name] = {"evaluated": st["evaluated"], "survivors": st["survivors"], "records": st["selected"],
                                       "none_records": st_none["selected"], "identical_to_none_filter": same, "variants": res,
                                       "smh_c_over_none": round(res["smh_c"]["device_ms"]["median"] / res["none"]["device_ms"]["median"], 5),
                                       "not_slower_than_none": bool(res["smh_c"]["device_ms"]["median"] <= res["none"]["device_ms"]["median"])}
        # the neighbours' kernels on the same set
        sel.set_param("matrix_mirror", 0)
        matrix("smh_matches", dtype=torch.float32, out=cells)
        sel.timing(2)
        for _ in range(10):
            matrix("smh_matches", dtype=torch.float32, out=cells)
        out["matrix_smh_f32_no_mirror_kernel_ms"] = round(sel.kernel_ms("matrix_smh"), 4)
        sel.timing(0)
        sel.set_param("matrix_mirror", 1)
        if not n_q:
            r, b = pkg.banding(m, tau)
            sel.set_criterion(pkg.CRIT_SMH_A)
            sel.run(tau, pkg.MODE_SMH, r, b, algo=pkg.ALGO_STREAM, fetch=False)
            sel.timing(2)
            for _ in range(10):
                sel.run(tau, pkg.MODE_SMH, r, b, algo=pkg.ALGO_STREAM, fetch=False)
            out["stream_stage1_kernel_ms"] = round(sel.kernel_ms("stage1"), 4)
            sel.timing(0)
        else:
            out["stream_stage1_kernel_ms"] = "not measured"
    del hll_t, aux_t, cards_t, cells
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/smhc_bench.json")
    ap.add_argument("--only", default="S1,S2,S3")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    results = []
    for name in args.only.split(","):
        r = bench(name, args.reps)
        results.append(r)
        print(json.dumps({k: r.get(k) for k in ("workload", "c_min", "matrix_smh_f32_no_mirror_kernel_ms", "stream_stage1_kernel_ms")}), flush=True)
        for mode_name, d in r["modes"].items():
            print(f"  {mode_name}: evaluated {d['evaluated']} survivors {d['survivors']} records {d['records']} (none: {d['none_records']}) "
                  f"identical {d['identical_to_none_filter']} smh_c / none {d['smh_c_over_none']} not slower {d['not_slower_than_none']}", flush=True)
            for v, x in d["variants"].items():
                print(f"    {v}: device {x['device_ms']} stage1 kernel {x.get('stage1_kernel_ms', '-')} ms ({x['reps']} reps)", flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": "MI355X", "workloads": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
