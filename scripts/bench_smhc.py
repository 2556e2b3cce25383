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

--shapes (a list of m out of 32,64,2048,4096, or 'all'): the narrow and the wide count kernel instead of the
workloads.  Per m and load -- 10 000 genomes all pairs, 1 000 queries x 50 000 -- on random rows that share a random part of their buckets
with one base row, under the estimator smh with c_min chosen so that about 0.1 % of the pairs survive: after 3 warm calls, `--reps`
alternating rounds of
  new            the pass on the kernel of m
  generic        the same pass under "smhc_generic" = 1 (the route every such m took before), same context and rows
  matrix         matrix("smh_matches", f32) of the same rows
The aim recorded: new's median <= matrix's median + its spread (max - min).  The records of new and generic are compared once.

usage: bench_smhc.py [--out profiles/smhc_bench.json] [--only S1,S2,S3] [--reps 20] [--shapes all]
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


SHAPES = (32, 64, 2048, 4096)
SHAPE_LOADS = {"self": (10_000, 0), "query": (50_000, 1_000)}


def shape_rows(n, m, seed):
    """n rows of m random buckets on the device, each sharing a random share of them with one base row (counts spread over 0 .. m)"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = torch.randint(0, 1 << 62, (n + 1, m), dtype=torch.int64, device="cuda", generator=g)
    keep = torch.rand((n, m), device="cuda", generator=g) < torch.rand((n, 1), device="cuda", generator=g)
    return torch.where(keep, rnd[n:], rnd[:n]).contiguous()


def bench_shapes(m, reps):
    import torch
    out = {"m": m, "workloads": {}}
    for wname, (n_d, n_q) in SHAPE_LOADS.items():
        with pkg.Selector(0) as sel:
            # (the estimator smh never reads the HLL rows; ascending cardinalities, none of them 0: every pair is in the pair space)
            hll = torch.zeros((max(n_d, n_q), 16384), dtype=torch.uint8, device="cuda")
            cards = torch.arange(1000, 1000 + n_d, dtype=torch.float64, device="cuda")
            rows = shape_rows(n_d + n_q, m, 1000 + m)
            sel.attach(hll[:n_d], rows[:n_d], cards)
            if n_q:
                sel.attach_queries(hll[:n_q], rows[n_d:], cards[:n_q].contiguous())
            cells = torch.empty((n_q or n_d, n_d), dtype=torch.float32, device="cuda")
            matrix = lambda: (sel.query_matrix if n_q else sel.matrix)("smh_matches", dtype=torch.float32, out=cells)   # noqa: E731
            matrix()
            hist = torch.bincount(cells.flatten().long(), minlength=m + 1).cpu().numpy().astype(np.int64)
            if not n_q:                                                                              # every pair twice, and the diagonal
                hist[m] -= n_d
                hist //= 2
            pairs = int(hist.sum())
            above = np.cumsum(hist[::-1])[::-1]                                                      # above[c] = pairs with count >= c
            c_min = max(1, int(np.argmin(np.abs(above[1:] - pairs / 1000.0))) + 1)
            sel.set_criterion(pkg.CRIT_SMH_C)
            sel.set_estimator("smh")
            sel.set_min_matches(c_min)

            def count_pass(generic, fetch=False):
                sel.set_param("smhc_generic", generic)
                rec = (sel.run_queries if n_q else sel.run)(0.0, pkg.MODE_SMH, 1, 1, fetch=fetch)
                sel.set_param("smhc_generic", 0)
                return rec

            variants = [("new", lambda: count_pass(0)), ("generic", lambda: count_pass(1)), ("matrix", matrix)]
            kernels = {}
            for vname, call in variants:
                for _ in range(3):
                    call()
                kernels[vname] = sel.get_param("matrix_smh_kernel_used" if vname == "matrix" else "smhc_kernel_used")
            direct, st = sorted_records(count_pass(0, fetch=True)), sel.stats()
            via = sorted_records(count_pass(1, fetch=True))
            assert st["survivors"] == int(above[c_min]) == sel.stats()["survivors"], (st, int(above[c_min]))
            samples = {v[0]: [] for v in variants}
            order_rng = np.random.default_rng(m)
            for r in range(reps):
                for vname, call in [variants[j] for j in order_rng.permutation(len(variants))]:
                    samples[vname].append(timed(call))
                print(f"  [m={m} {wname}] round {r + 1} of {reps}", file=sys.stderr, flush=True)
            res = {v: summary(s) for v, s in samples.items()}
            t, new = res["matrix"]["device_ms"], res["new"]["device_ms"]["median"]
            aim = t["median"] + (t["max"] - t["min"])
            out["workloads"][wname] = {"pairs": pairs, "c_min": c_min, "survivors": st["survivors"], "records": st["selected"], "kernel_used": kernels,
                                       "identical_to_generic": bool(direct.tobytes() == via.tobytes()), "variants": res, "aim_ms": round(aim, 3),
                                       "aim_met": bool(new <= aim), "generic_over_new": round(res["generic"]["device_ms"]["median"] / new, 2)}
        del hll, cards, rows, cells
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="default profiles/smhc_bench.json, with --shapes profiles/smhc_shapes_bench.json")
    ap.add_argument("--shapes", default=None, help="the narrow / wide count kernels instead of the workloads: a list of m out of 32,64,2048,4096, or 'all'")
    ap.add_argument("--only", default="S1,S2,S3")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    if args.shapes:
        path = Path(args.out or "profiles/smhc_shapes_bench.json")
        results = []
        for m in (SHAPES if args.shapes == "all" else [int(x) for x in args.shapes.split(",")]):
            results.append(bench_shapes(m, args.reps))
            print(json.dumps(results[-1]), flush=True)
            path.parent.mkdir(parents=True, exist_ok=True)
            path.write_text(json.dumps({"device": "MI355X", "protocol": f"3 warm calls, {args.reps} alternating rounds, device events", "shapes": results}, indent=1) + "\n")
        return 0
    args.out = args.out or "profiles/smhc_bench.json"
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
