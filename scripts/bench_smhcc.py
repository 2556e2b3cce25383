#!/usr/bin/env python3
"""GPU box: criterion smh_c with its per-pair threshold for a minimum containment gamma (selhip_ctx_set_min_containment, DESIGN.md
section 17) as the prefilter of a containment screen: m = 512, gamma = 0.8, no CB bound (-n), measure max_containment, tau = gamma.

  C1  cfg3, 10 000 genomes (5.0e7 pairs)                     C3  query pass: 1 000 queries x 50 000 database genomes (5.0e7 pairs)
  C2  cfg3-spread, 10 000 genomes of spread cardinalities (the thresholds of the pairs actually vary)

Per workload, in ONE process, `--reps` alternating rounds of the variants (a fresh seeded order every round), each timed with device
events around the call; median (min ... max):
  smh_c_gamma    the pass under smh_c with the containment rule (no c_min)
  smh_c_fixed    its fixed-rule twin at c_min = 342 = smhc_threshold(512, 0.8f, e, e): the same kernel shape with one threshold
  none           the pass under criterion none: the only route to a containment screen before the rule
Conditions recorded: smh_c_gamma's median below none's (the ratio is reported); the twin rule -- smh_c_gamma's median no higher than
the twin's median plus the twin's own max - min -- with the survivor counts of both beside it (a looser rule hands more survivors to
stage 2).  The records of smh_c_gamma are compared once with the `none` records filtered on the device by their cell of the
SuperMinHash match matrix against the threshold of the pair, restated here in numpy.  Afterwards the stage-1 kernels alone under
selhip_ctx_timing(2) (mean of 10).

usage: bench_smhcc.py [--out profiles/smhcc_bench.json] [--only C1,C2,C3] [--reps 20]
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
    "C1": ("cfg3", C["cfg3"], 10_000, 0),
    "C2": ("cfg3-spread", C["cfg3-spread"], 10_000, 0),
    "C3": ("1000 x 50000", C["cfg4"], 50_000, 1_000),
}
M_BUCKETS = 512
GAMMA = float(np.float32(0.8))                  # (double)0.8f: the pass's float threshold as a double
C_TWIN = 342


def model_threshold(m, gamma, e_lo, e_hi):
    """selhip_smhc_threshold restated in numpy float64 (every operation rounded on its own)"""
    a, b = e_lo.astype(np.float64), e_hi.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = ((gamma * m) * a) / ((a + b) - gamma * a)
        top = (a == 0) | ~(((a + b) - gamma * a) > 0) | (q > m)
        return np.where(top, m + 1, np.where(q <= 0, 0.0, np.ceil(np.where(top, 0.0, q)))).astype(np.int64)


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
    cfg = SynthConfig(f"{name}:{gen.name}", n, M_BUCKETS, 0.8, gen.seed ^ (0x0051 if n_q else 0), p_aux=0, cluster_size=gen.cluster_size,
                      mode=gen.mode, n_sh_lo=gen.n_sh_lo, n_sh_hi=gen.n_sh_hi)
    hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg)
    m, tau = M_BUCKETS, 0.8
    assert pkg.containment_matches(m, GAMMA, 13000, 13000) == C_TWIN
    out = {"workload": name, "set": label, "n_genomes": n_d, "n_queries": n_q, "m": m, "gamma": GAMMA, "tau": tau, "c_twin": C_TWIN}
    # two contexts on the same device arrays: c_min is sticky, and the gamma pass runs without a floor
    with pkg.Selector(0) as sel_g, pkg.Selector(0) as sel_f:
        sels = (sel_g, sel_f)
        if n_q:
            is_q = np.zeros(n, dtype=bool)
            is_q[np.random.default_rng(cfg.seed).choice(n, n_q, replace=False)] = True
            mq = torch.from_numpy(is_q).to(hll_t.device)
            D = (hll_t[~mq].contiguous(), aux_t[~mq].contiguous(), cards_t[~mq].contiguous())
            Q = (hll_t[mq].contiguous(), aux_t[mq].contiguous(), cards_t[mq].contiguous())
            for s in sels:
                s.attach(*D)
                s.attach_queries(*Q)
            shape = (n_q, n_d)
            run_pass = lambda s: s.run_queries(tau, pkg.MODE_SMH, 1, 1, fetch=False)                  # noqa: E731
            e_r, e_c = (x.cpu().numpy().astype(np.int64).astype(np.uint64) for x in (Q[2], D[2]))
        else:
            for s in sels:
                s.attach(hll_t, aux_t, cards_t)
            shape = (n_d, n_d)
            run_pass = lambda s: s.run(tau, pkg.MODE_SMH, 1, 1, fetch=False)                          # noqa: E731
            e_r = e_c = cards_t.cpu().numpy().astype(np.int64).astype(np.uint64)
        for s in sels:
            s.set_measure("max_containment")
        sel_g.set_criterion(pkg.CRIT_SMH_C)
        sel_g.set_min_containment(GAMMA)
        sel_f.set_min_matches(C_TWIN)

        def smh_c_gamma():
            run_pass(sel_g)

        def smh_c_fixed():
            sel_f.set_criterion(pkg.CRIT_SMH_C)
            run_pass(sel_f)

        def none():
            sel_f.set_criterion(pkg.CRIT_NONE)
            run_pass(sel_f)

        variants = [("smh_c_gamma", smh_c_gamma), ("smh_c_fixed", smh_c_fixed), ("none", none)]
        for _, run in variants:                                                                      # warm-up: the lists take their sizes
            run()
            run()
        # the records of the rule against none + match matrix + device filter by the model's threshold, compared once
        smh_c_gamma()
        st_g = sel_g.stats()
        direct = sorted_records(sel_g.fetch())
        assert sel_g.get_param("smhc_path_used") == 1 and sel_g.get_param("smhc_rule_used") == 1
        smh_c_fixed()
        st_f = sel_f.stats()
        assert sel_f.get_param("smhc_rule_used") == 0
        none()
        st_none = sel_f.stats()
        cnt = sel_f.result_count()
        rec = torch.empty((max(cnt, 1), 4), dtype=torch.int32, device="cuda")                         # {i, k, value (two dwords)} per record
        sel_f.copy_results_to(rec)
        rec = rec[:cnt]
        cells = torch.empty(shape, dtype=torch.float32, device="cuda")
        (sel_f.query_matrix if n_q else sel_f.matrix)("smh_matches", dtype=torch.float32, out=cells)
        ri, rk = rec[:, 0].cpu().numpy().astype(np.int64), rec[:, 1].cpu().numpy().astype(np.int64)
        need = model_threshold(m, GAMMA, np.minimum(e_r[ri], e_c[rk]), np.maximum(e_r[ri], e_c[rk]))
        keep = cells[rec[:, 0].long(), rec[:, 1].long()] >= torch.from_numpy(need.astype(np.float32)).to("cuda")
        via = sorted_records(rec[keep].cpu().numpy().view(pkg.PAIR_DTYPE).reshape(-1))
        same = bool(len(direct) == len(via) and np.array_equal(direct["i"], via["i"]) and np.array_equal(direct["k"], via["k"])
                    and np.array_equal(direct["jaccard"].view(np.uint64), via["jaccard"].view(np.uint64)))
        del cells
        samples = {v[0]: [] for v in variants}
        order_rng = np.random.default_rng(1)
        for r in range(reps):                                                                        # alternating rounds, a fresh order each
            for vname, run in [variants[j] for j in order_rng.permutation(len(variants))]:
                samples[vname].append(timed(run))
            print(f"  [{name}] round {r + 1} of {reps}", file=sys.stderr, flush=True)
        res = {v: summary(s) for v, s in samples.items()}
        # the stage-1 kernels alone, under the contexts' own timers
        for vname, s, run in (("smh_c_gamma", sel_g, smh_c_gamma), ("smh_c_fixed", sel_f, smh_c_fixed)):
            run()
            s.timing(2)
            for _ in range(10):
                run()
            res[vname]["stage1_kernel_ms"] = round(s.kernel_ms("stage1"), 4)
            s.timing(0)
        g, f, nn = (res[v]["device_ms"] for v in ("smh_c_gamma", "smh_c_fixed", "none"))
        out.update({"evaluated": st_g["evaluated"], "survivors_gamma": st_g["survivors"], "survivors_fixed": st_f["survivors"],
                    "records_gamma": st_g["selected"], "records_fixed": st_f["selected"], "records_none": st_none["selected"],
                    "identical_to_none_filter": same, "variants": res,
                    "gamma_over_none": round(g["median"] / nn["median"], 5), "below_none": bool(g["median"] < nn["median"]),
                    "twin_bound_ms": round(f["median"] + (f["max"] - f["min"]), 3),
                    "within_twin_rule": bool(g["median"] <= f["median"] + (f["max"] - f["min"]))})
    del hll_t, aux_t, cards_t
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/smhcc_bench.json")
    ap.add_argument("--only", default="C1,C2,C3")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    results = []
    for name in args.only.split(","):
        r = bench(name, args.reps)
        results.append(r)
        print(json.dumps({k: v for k, v in r.items() if k != "variants"}), flush=True)
        for v, x in r["variants"].items():
            print(f"    {v}: device {x['device_ms']} stage1 kernel {x.get('stage1_kernel_ms', '-')} ms ({x['reps']} reps)", flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": "MI355X", "workloads": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
