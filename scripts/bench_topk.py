#!/usr/bin/env python3
"""GPU box: top-k of the query passes (selhip_ctx_set_query_topk) against what a caller had to do without it, DESIGN.md section 10.
Two routes to "every query's K best records in ranked order", alternated round by round in one process after warm passes:
  device  query pass with top-k on + fetch_ranked (the cut and the ordering run on the device behind the pass)
  host    query pass with top-k off + fetch (the whole list over the link, the library's host sort) + the numpy ranking below
Wall time from before the pass to the ranked list in host memory, median (min .. max) of --rounds rounds, the two results compared
record for record (i, k, J bits) in every round; a difference, or a device route that is not faster in every round of T2 / T3, makes the
script exit non-zero.  Also per workload: device time of the pass alone and of pass + top-k (events around the call, median of the
rounds), the "topk" timer, and for criterion none the fused kernel's own time ("dense").
  T1  W1 of bench_query.py (50 000 x 1 000, m 512, tau 0.8, smh_a), K = 10: what the cut adds to a sparse result
  T2  criterion none, MODE_SMH, tau = -1: 10 000 x 1 000 = 1e7 records (160 MB), K in 1, 10, 100, 1024
  T3  1 query x 100 000, criterion none, K = 10: one hot segment
The host route ranks once per round and cuts for every K (its time for a K = pass + fetch + ranking + that cut).
usage: bench_topk.py [--out profiles/topk_bench.json] [--rounds 20] [--only T1,T2,T3]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import cuda_selection_criteria_amd as pkg  # noqa: E402
from cuda_selection_criteria_amd import SynthConfig  # noqa: E402

C = pkg.SYNTH_CONFIGS
SIGN = np.uint64(1 << 63)
WORKLOADS = {
    #       database  queries  generator  m     criterion        mode             tau    K
    "T1": (50_000, 1_000, C["cfg4"], 512, pkg.CRIT_SMH_A, pkg.MODE_CB_SMH, 0.8, (10,)),
    "T2": (10_000, 1_000, C["cfg3"], 64, pkg.CRIT_NONE, pkg.MODE_SMH, -1.0, (1, 10, 100, 1024)),
    "T3": (100_000, 1, C["cfg4"], 64, pkg.CRIT_NONE, pkg.MODE_SMH, -1.0, (10,)),
}


def ranking(S):
    """S in ranked order and every record's position inside its query: i ascending, key(J) descending, k ascending"""
    b = S["jaccard"].view(np.uint64)
    key = np.where((b & SIGN) != 0, ~b, b ^ SIGN)
    R = S[np.lexsort((S["k"], ~key, S["i"]))]
    at = np.arange(len(R))
    first = np.ones(len(R), dtype=bool)
    first[1:] = R["i"][1:] != R["i"][:-1]
    return R, at - np.maximum.accumulate(np.where(first, at, 0))


def same_records(a, b):
    return len(a) == len(b) and np.array_equal(a["i"], b["i"]) and np.array_equal(a["k"], b["k"]) and \
        np.array_equal(a["jaccard"].view(np.uint64), b["jaccard"].view(np.uint64))


def spread(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x)), "rounds": len(x)}


def bench(name, rounds):
    import torch
    n_d, n_q, gen, m, crit, mode, tau, Ks = WORKLOADS[name]
    cfg = SynthConfig(f"{name}:{gen.name}", n_d + n_q, m, tau, gen.seed ^ 0x0051, cluster_size=gen.cluster_size, mode=gen.mode,
                      n_sh_lo=gen.n_sh_lo, n_sh_hi=gen.n_sh_hi)
    hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg)                  # ascending cardinality
    n = n_d + n_q
    is_q = np.zeros(n, dtype=bool)
    is_q[np.random.default_rng(cfg.seed).choice(n, n_q, replace=False)] = True
    mq = torch.from_numpy(is_q).to(hll_t.device)
    q_t = (hll_t[mq].contiguous(), aux_t[mq].contiguous(), cards_t[mq].contiguous())
    d_t = (hll_t[~mq].contiguous(), aux_t[~mq].contiguous(), cards_t[~mq].contiguous())
    del hll_t, aux_t, cards_t
    r, b = pkg.banding(m, tau) if crit == pkg.CRIT_SMH_A else (1, 1)
    out = {"workload": name, "n_database": n_d, "n_queries": n_q, "m": m, "tau": tau, "criterion": crit, "mode": mode, "rounds": rounds}
    ok = True
    with pkg.Selector(0) as sel:
        sel.set_criterion(crit)
        sel.attach(*d_t)
        sel.attach_queries(*q_t)

        def run(k):
            sel.set_query_topk(k)
            sel.run_queries(tau, mode, r, b, fetch=False)

        def device_ms(k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(k)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        for k in (0,) + Ks:                                              # warm: every shape the timed rounds use
            for _ in range(3):
                run(k)
        out["selected"] = sel.stats()["selected"]
        out["record_bytes"] = 16 * out["selected"]
        out["query_topk_lds_cap"] = sel.get_param("query_topk_lds_cap")
        wall = {"host_common": [], "host_cut": {k: [] for k in Ks}, "device": {k: [] for k in Ks}}
        dev = {"pass": [], "pass_topk": {k: [] for k in Ks}}
        identical = {k: True for k in Ks}
        reduced = {}
        for _ in range(rounds):
            t0 = time.perf_counter()
            run(0)
            S = sel.fetch()
            R, pos = ranking(S)
            wall["host_common"].append((time.perf_counter() - t0) * 1e3)
            dev["pass"].append(device_ms(0))
            for k in Ks:
                t0 = time.perf_counter()
                want = R[pos < k]
                wall["host_cut"][k].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                run(k)
                got = sel.fetch_ranked()
                wall["device"][k].append((time.perf_counter() - t0) * 1e3)
                identical[k] = identical[k] and same_records(got, want)
                reduced[k] = len(got)
                dev["pass_topk"][k].append(device_ms(k))
        out["pass_ms"] = spread(dev["pass"])
        out["per_k"] = {}
        for k in Ks:
            host = np.array(wall["host_common"]) + np.array(wall["host_cut"][k])
            device = np.array(wall["device"][k])
            sel.timing(1)
            run(k)
            per_kernel = {t: sel.kernel_ms(t) for t in ("topk", "dense", "total") if sel.kernel_ms(t) >= 0}
            sel.timing(0)
            faster = bool(np.all(device < host))
            out["per_k"][str(k)] = {"reduced": reduced[k], "identical": bool(identical[k]), "host_wall_ms": spread(host), "device_wall_ms": spread(device),
                                    "device_faster_every_round": faster, "speedup_median": float(np.median(host) / np.median(device)),
                                    "pass_topk_ms": spread(dev["pass_topk"][k]),
                                    "added_ms_median": float(np.median(dev["pass_topk"][k]) - np.median(dev["pass"])), "kernel_ms": per_kernel}
            ok = ok and identical[k] and (faster or name == "T1")
        sel.set_query_topk(0)
    return out, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "topk_bench.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--only", default="T1,T2,T3")
    a = ap.parse_args()
    if pkg.hip_lib().selhip_device_count() <= 0:
        sys.exit("bench_topk.py: no MI355X (gfx950) device: nothing is measured without one")
    res, ok = [], True
    for name in a.only.split(","):
        r, good = bench(name, a.rounds)
        print(json.dumps(r), flush=True)
        res.append(r)
        ok = ok and good
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
