#!/usr/bin/env python3
"""GPU box: query-vs-database passes (selhip_ctx_run_queries) on the workloads W1..W8 of DESIGN.md section 8.  One seeded set of
n_D + n_Q genomes from the synthetic generator, a seeded random n_Q of them as queries (generator clusters span both sides, so real
cross pairs exist).  Per workload: device ms per query pass (events around the pass, warm, median of >= 20 passes, with min / max), n_Q * n_D per second and
the per-kernel figures; for W1, W2, W5 and W6..W8 also the union route (an all-pairs pass over Q u D under the same criterion, cut to its
cross pairs), timed in the same run and compared with the query pass (pairs and J bits) -- any difference makes the script exit non-zero.
W1..W5 run criterion smh_a, W6 the two-stage hll_a + smh_a of BASELINE configs[4], W7 hll_a and W8 hll_an (auxiliary HLL p = 8);
--criterion runs the chosen workloads under another criterion (auxiliary HLL p = 8 where the workload has none).
usage: bench_query.py [--out profiles/query_bench.json] [--passes 20] [--only W1,W3] [--criterion smh_a|hll_a|hll_an|hll_a+smh_a]"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import cuda_selection_criteria_amd as pkg  # noqa: E402
from cuda_selection_criteria_amd import PAIR_DTYPE, SynthConfig  # noqa: E402

C = pkg.SYNTH_CONFIGS
CRITERIA = {"smh_a": pkg.CRIT_SMH_A, "hll_a": pkg.CRIT_HLL_A, "hll_an": pkg.CRIT_HLL_AN, "hll_a+smh_a": pkg.CRIT_HLL_A_SMH_A}
WORKLOADS = {
    #       database  queries  generator  union route  criterion  auxiliary HLL p
    "W1": (50_000, 1_000, C["cfg4"], True, "smh_a", 0),
    "W2": (100_000, 1_000, C["cfg5"], True, "smh_a", 0),
    "W3": (50_000, 1, C["cfg4"], False, "smh_a", 0),
    "W4": (10_000, 10_000, C["cfg3"], False, "smh_a", 0),
    "W5": (50_000, 1_000, C["cfg3-spread"], True, "smh_a", 0),     # CB prunes: most join blocks meet no window and leave at once
    "W6": (100_000, 1_000, C["cfg5"], True, "hll_a+smh_a", 8),     # the configs[4] shape
    "W7": (50_000, 1_000, C["cfg3-spread"], True, "hll_a", 8),
    "W8": (50_000, 1_000, C["cfg3-spread"], True, "hll_an", 8),
}
KERNELS = ("prep", "sigbuild", "join", "verify", "stage1", "aux", "hist", "select", "total")


def timed_passes(sel, run, passes):
    """device time of whole passes (a pair of events on the stream around each one, no events inside it), then one pass with every
    kernel scope timed for the per-kernel figures"""
    import torch
    sel.timing(0)
    ms = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    sel.timing(1)
    run()
    per_kernel = {k: sel.kernel_ms(k) for k in KERNELS if sel.kernel_ms(k) >= 0}
    sel.timing(0)
    return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "passes": len(ms),
            "kernel_ms": per_kernel}


def bench(name, passes, criterion=None):
    n_d, n_q, gen, union, crit_name, p_aux = WORKLOADS[name]
    if criterion is not None:
        crit_name = criterion
        if crit_name != "smh_a" and not p_aux:
            p_aux = 8
    crit = CRITERIA[crit_name]
    cfg = SynthConfig(f"{name}:{gen.name}", n_d + n_q, gen.m, gen.tau, gen.seed ^ 0x0051, p_aux=p_aux, cluster_size=gen.cluster_size,
                      mode=gen.mode, n_sh_lo=gen.n_sh_lo, n_sh_hi=gen.n_sh_hi)
    hll_t, aux_t, cards_t, _, ah_t = pkg.synth_device(cfg)               # ascending cardinality
    n = n_d + n_q
    is_q = np.zeros(n, dtype=bool)
    is_q[np.random.default_rng(cfg.seed).choice(n, n_q, replace=False)] = True
    mq = pkg_bool(is_q, hll_t.device)
    q_t = (hll_t[mq].contiguous(), aux_t[mq].contiguous(), cards_t[mq].contiguous())
    d_t = (hll_t[~mq].contiguous(), aux_t[~mq].contiguous(), cards_t[~mq].contiguous())
    r, b = pkg.banding(cfg.m, cfg.tau)
    out = {"workload": name, "n_database": n_d, "n_queries": n_q, "m": cfg.m, "tau": cfg.tau, "n_rows": r, "n_bands": b,
           "generator": gen.name, "criterion": crit_name, "p_aux": p_aux}
    with pkg.Selector(0) as sel:
        sel.set_criterion(crit)
        sel.attach(*d_t)
        sel.attach_queries(*q_t)
        if p_aux:
            ah_q, ah_d = ah_t[mq].contiguous(), ah_t[~mq].contiguous()
            sel.attach_aux_hll(ah_d, p_aux)
            sel.attach_queries_aux_hll(ah_q, p_aux)
        for _ in range(3):
            got = sel.run_queries(cfg.tau, pkg.MODE_CB_SMH, r, b)
        st = sel.stats()
        q = timed_passes(sel, lambda: sel.run_queries(cfg.tau, pkg.MODE_CB_SMH, r, b, fetch=False), passes)
        q.update({"selected": len(got), "stats": st, "pairs_per_s": n_q * n_d / (q["median_ms"] * 1e-3),
                  "query_db_sig_builds": sel.get_param("query_db_sig_builds")})
        out["query"] = q
        if union:
            sel.attach(hll_t, aux_t, cards_t)
            if p_aux:
                sel.attach_aux_hll(ah_t, p_aux)
            allp = sel.run(cfg.tau, pkg.MODE_CB_SMH, r, b)
            u = timed_passes(sel, lambda: sel.run(cfg.tau, pkg.MODE_CB_SMH, r, b, fetch=False), max(5, passes // 4))
            q_rank, d_rank = np.cumsum(is_q) - 1, np.cumsum(~is_q) - 1
            cross = is_q[allp["i"]] != is_q[allp["k"]]
            a, c = allp["i"][cross], allp["k"][cross]
            want = np.zeros(int(cross.sum()), dtype=PAIR_DTYPE)
            want["i"] = np.where(is_q[a], q_rank[a], q_rank[c])
            want["k"] = np.where(is_q[a], d_rank[c], d_rank[a])
            want["jaccard"] = allp["jaccard"][cross]
            want = want[np.lexsort((want["k"], want["i"]))]
            same = len(want) == len(got) and np.array_equal(want["i"], got["i"]) and np.array_equal(want["k"], got["k"]) and \
                np.array_equal(want["jaccard"].view(np.uint64), got["jaccard"].view(np.uint64))
            u.update({"pairs": n * (n - 1) // 2, "cross_selected": len(want), "identical": bool(same),
                      "speedup_query_vs_union": u["median_ms"] / q["median_ms"]})
            out["union"] = u
    return out


def pkg_bool(mask, device):
    import torch
    return torch.from_numpy(mask).to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "query_bench.json"))
    ap.add_argument("--passes", type=int, default=20)
    ap.add_argument("--only", default="W1,W2,W3,W4,W5")
    ap.add_argument("--criterion", choices=sorted(CRITERIA), default=None, help="run the workloads under this criterion instead of their own")
    a = ap.parse_args()
    res = []
    ok = True
    for name in a.only.split(","):
        r = bench(name, a.passes, a.criterion)
        print(json.dumps(r), flush=True)
        res.append(r)
        if "union" in r and not r["union"]["identical"]:
            ok = False
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
