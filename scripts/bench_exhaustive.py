#!/usr/bin/env python3
"""GPU box: criterion none (SELHIP_CRIT_NONE, every pair of the pair space to the HLL-14 Jaccard test) on the workloads E1..E4 of
DESIGN.md section 9, the fused kernel against the list route -- the yardstick: the kernels the other criteria already run.

  E1  cfg3, 10 000 genomes (5.0e7 pairs), no CB        E3  cfg4, 50 000 genomes (1.25e9 pairs), no CB
  E2  cfg3-spread, 10 000 genomes, CB                  E4  query pass 50 000 x 1 000 (the sets of bench_query.py's W1), no CB

Per workload, in ONE process: `--rounds` alternating rounds of three variants -- fused ("dense_fused" = 1), list route with the
fused kernel's decode ("dense_fused" = 0, "hist_sparse" = 0: like for like) and list route with its default "hist_sparse" -- each
timed with device events around the synchronous pass (results left on the device); min / median / max, pairs per second, and the
like-for-like condition: fused median <= list median * (1 + (max - min) / median of the list route's passes).
Same outputs at the sizes timed: records (i, k, J bits) and statistics of the three variants compared in full (E3: count, evaluated
and a checksum of the sorted records).  With --recall, the recall table of the four criteria against the exhaustive pass
(scripts/experiments.py recall_rows) for E1 and E2.

usage: bench_exhaustive.py [--out profiles/exhaustive_bench.json] [--only E1,E2] [--rounds 3] [--recall]
"""
import argparse
import json
import statistics
import sys
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

import cuda_selection_criteria_amd as pkg  # noqa: E402
from cuda_selection_criteria_amd import SynthConfig  # noqa: E402

C = pkg.SYNTH_CONFIGS
WORKLOADS = {
    "E1": ("cfg3", C["cfg3"], pkg.MODE_SMH, 0),
    "E2": ("cfg3-spread", C["cfg3-spread"], pkg.MODE_CB_SMH, 0),
    "E3": ("cfg4", C["cfg4"], pkg.MODE_SMH, 0),
    "E4": ("W1", C["cfg4"], pkg.MODE_SMH, 1_000),
}
VARIANTS = (("fused", 1, 0), ("list_like_for_like", 0, 0), ("list_default", 0, -1))      # name, dense_fused, hist_sparse


def checksum(rec):
    return zlib.crc32(np.ascontiguousarray(rec).tobytes())


def timed(run):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def bench(name, rounds, with_recall):
    import torch
    label, gen, mode, n_q = WORKLOADS[name]
    p_aux = 8 if with_recall and not n_q else 0
    n = gen.n_genomes + n_q
    cfg = SynthConfig(f"{name}:{gen.name}", n, gen.m, gen.tau, gen.seed ^ (0x0051 if n_q else 0), p_aux=p_aux, cluster_size=gen.cluster_size,
                      mode=gen.mode, n_sh_lo=gen.n_sh_lo, n_sh_hi=gen.n_sh_hi)
    hll_t, aux_t, cards_t, _, ah_t = pkg.synth_device(cfg)
    out = {"workload": name, "set": label, "n_genomes": gen.n_genomes, "n_queries": n_q, "tau": cfg.tau,
           "mode": "cb" if mode == pkg.MODE_CB_SMH else "nocb"}
    with pkg.Selector(0) as sel:
        if n_q:
            is_q = np.zeros(n, dtype=bool)
            is_q[np.random.default_rng(cfg.seed).choice(n, n_q, replace=False)] = True
            mq = torch.from_numpy(is_q).to(hll_t.device)
            q_t = (hll_t[mq].contiguous(), aux_t[mq].contiguous(), cards_t[mq].contiguous())
            d_t = (hll_t[~mq].contiguous(), aux_t[~mq].contiguous(), cards_t[~mq].contiguous())
            sel.attach(*d_t)
            sel.attach_queries(*q_t)
            run = lambda fetch: sel.run_queries(cfg.tau, mode, 1, 1, fetch=fetch)          # noqa: E731
        else:
            sel.attach(hll_t, aux_t, cards_t)
            if p_aux:
                sel.attach_aux_hll(ah_t, p_aux)
            run = lambda fetch: sel.run(cfg.tau, mode, 1, 1, fetch=fetch)                  # noqa: E731
        sel.set_criterion(pkg.CRIT_NONE)
        out["hll_khi"] = sel.get_param("hll_khi")
        res, ms = {}, {v[0]: [] for v in VARIANTS}
        for vname, fused, sparse in VARIANTS:                                              # warm-up + outputs
            sel.set_param("dense_fused", fused)
            sel.set_param("hist_sparse", sparse)
            got = run(True)
            st = sel.stats()
            res[vname] = {"selected": len(got), "stats": st, "crc32_sorted_records": checksum(got), "route_used": sel.get_param("dense_route_used"),
                          "hist_sparse_t": sel.get_param("hist_sparse_t")}
            if vname == "fused":
                first = got
            else:
                res[vname]["identical_to_fused"] = bool(len(got) == len(first) and np.array_equal(got["i"], first["i"]) and np.array_equal(got["k"], first["k"])
                                                        and np.array_equal(got["jaccard"].view(np.uint64), first["jaccard"].view(np.uint64)) and st == res["fused"]["stats"])
        for _ in range(rounds):                                                            # alternating rounds
            for vname, fused, sparse in VARIANTS:
                sel.set_param("dense_fused", fused)
                sel.set_param("hist_sparse", sparse)
                ms[vname].append(timed(lambda: run(False)))
        pairs = res["fused"]["stats"]["evaluated"]
        for vname, _, _ in VARIANTS:
            t = ms[vname]
            res[vname].update({"ms": [round(x, 3) for x in t], "min_ms": round(min(t), 3), "median_ms": round(statistics.median(t), 3), "max_ms": round(max(t), 3),
                               "pairs_per_s": pairs / (statistics.median(t) * 1e-3), "ns_per_pair": statistics.median(t) * 1e6 / max(pairs, 1)})
        lst = res["list_like_for_like"]
        spread = (lst["max_ms"] - lst["min_ms"]) / lst["median_ms"]
        out.update({"pairs": pairs, "variants": res, "list_route_spread": spread,
                    "like_for_like_holds": bool(res["fused"]["median_ms"] <= lst["median_ms"] * (1 + spread)),
                    "fused_over_list_like_for_like": res["fused"]["median_ms"] / lst["median_ms"],
                    "fused_over_list_default": res["fused"]["median_ms"] / res["list_default"]["median_ms"]})
        sel.set_param("dense_fused", 1)
        sel.set_param("hist_sparse", -1)
        if with_recall and not n_q:
            from experiments import RECALL_CRITERIA, RECALL_HEADER, recall_rows
            rows = recall_rows(sel, label, n, cfg.m, p_aux, [cfg.tau, 0.9], list(RECALL_CRITERIA), ["cb" if mode == pkg.MODE_CB_SMH else "nocb"])
            out["recall"] = [dict(zip(RECALL_HEADER, r)) for r in rows]
    del hll_t, aux_t, cards_t, ah_t
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/exhaustive_bench.json")
    ap.add_argument("--only", default="E1,E2")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--recall", action="store_true")
    args = ap.parse_args()
    results = []
    for name in args.only.split(","):
        r = bench(name, args.rounds, args.recall)
        results.append(r)
        print(json.dumps({k: r[k] for k in ("workload", "pairs", "like_for_like_holds", "fused_over_list_like_for_like", "fused_over_list_default")}), flush=True)
        for v, d in r["variants"].items():
            print(f"  {v}: {d['ms']} ms, selected {d['selected']}, identical {d.get('identical_to_fused', '-')}", flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": "MI355X", "workloads": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
