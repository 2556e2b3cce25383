#!/usr/bin/env python3
"""GPU box: query-vs-database passes (selhip_ctx_run_queries) on the workloads W1..W8 of DESIGN.md section 8.  One seeded set of
n_D + n_Q genomes from the synthetic generator, a seeded random n_Q of them as queries (generator clusters span both sides, so real
cross pairs exist).  Per workload: device ms per query pass (events around the pass, warm, median of >= 20 passes, with min / max), n_Q * n_D per second and
the per-kernel figures; for W1, W2, W5 and W6..W8 also the union route (an all-pairs pass over Q u D under the same criterion, cut to its
cross pairs), timed in the same run and compared with the query pass (pairs and J bits) -- any difference makes the script exit non-zero.
W1..W5 run criterion smh_a, W6 the two-stage hll_a + smh_a of BASELINE configs[4], W7 hll_a and W8 hll_an (auxiliary HLL p = 8);
--criterion runs the chosen workloads under another criterion (auxiliary HLL p = 8 where the workload has none).
--algo sig (default) times the query pass as the library chooses it; index times it under ALGO_INDEX (the sorted band-signature index of
the database); both times SIG and INDEX in alternation in one process (>= 3 rounds of --passes each, after warm-up passes that include
the index build), compares their results (records and J bits, statistics; exit non-zero on a difference) and reports, for INDEX, the
one-off build time, the index's resident bytes and the break-even number of passes.
usage: bench_query.py [--out profiles/query_bench.json] [--passes 20] [--only W1,W3] [--criterion smh_a|hll_a|hll_an|hll_a+smh_a]
                      [--algo sig|index|both] [--rounds 3]"""
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


def timed_passes(sel, run, passes, keep_all=False):
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
    out = {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms)), "passes": len(ms),
           "kernel_ms": per_kernel}
    if keep_all:
        out["pass_ms"] = [float(x) for x in ms]
    return out


def same_records(a, b):
    return len(a) == len(b) and np.array_equal(a["i"], b["i"]) and np.array_equal(a["k"], b["k"]) and \
        np.array_equal(a["jaccard"].view(np.uint64), b["jaccard"].view(np.uint64))


def bench_both(sel, cfg, r, b, n_q, n_d, passes, rounds):
    """SIG and INDEX on one context, timed in alternation; returns ({"sig": ..., "index": ...}, the SIG records, identical?)"""
    run = {name: (lambda fetch=True, algo=algo: sel.run_queries(cfg.tau, pkg.MODE_CB_SMH, r, b, algo=algo, fetch=fetch))
           for name, algo in (("sig", pkg.ALGO_SIG), ("index", pkg.ALGO_INDEX))}
    res = {"sig": {}, "index": {}}
    got, st = {}, {}
    run["sig"]()                                                         # the database signatures are built here, not in the index's build figure
    sel.timing(1)
    got["index"] = run["index"]()                                        # the first INDEX pass: key build + sort, timed as "sigbuild"
    res["index"]["build_ms"] = sel.kernel_ms("sigbuild")
    sel.timing(0)
    for name in ("sig", "index"):
        for _ in range(3):
            got[name] = run[name]()
        st[name] = sel.stats()
    parts = {"sig": [], "index": []}
    for _ in range(max(3, rounds)):
        for name in ("sig", "index"):
            parts[name].append(timed_passes(sel, lambda name=name: run[name](False), passes, keep_all=True))
    for name in ("sig", "index"):
        ms = [p["median_ms"] for p in parts[name]]
        res[name].update({"median_ms": float(np.median(ms)), "min_ms": float(min(p["min_ms"] for p in parts[name])),
                          "max_ms": float(max(p["max_ms"] for p in parts[name])), "round_medians_ms": ms,
                          "round_pass_ms": [p["pass_ms"] for p in parts[name]],
                          "passes": int(sum(p["passes"] for p in parts[name])), "kernel_ms": parts[name][-1]["kernel_ms"],
                          "selected": len(got[name]), "stats": st[name]})
        res[name]["pairs_per_s"] = n_q * n_d / (res[name]["median_ms"] * 1e-3)
    gain = res["sig"]["median_ms"] - res["index"]["median_ms"]
    res["index"].update({"index_bytes": 1024 * sel.get_param("query_db_index_kib"), "break_even_passes": res["index"]["build_ms"] / gain if gain > 0 else None,
                         "query_db_index_builds": sel.get_param("query_db_index_builds"),
                         "max_below_sig_min": bool(res["index"]["max_ms"] < res["sig"]["min_ms"]),
                         "speedup_vs_sig": res["sig"]["median_ms"] / res["index"]["median_ms"]})
    identical = same_records(got["sig"], got["index"]) and all(st["sig"][k] == st["index"][k] for k in st["sig"])
    return res, got["sig"], bool(identical)


def bench(name, passes, criterion=None, algo="sig", rounds=3):
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
        if algo == "both":
            both, got, same_algos = bench_both(sel, cfg, r, b, n_q, n_d, passes, rounds)
            q = both["sig"]
            out["index"] = both["index"]
            out["index_identical_to_sig"] = same_algos
        else:
            run_algo = pkg.ALGO_INDEX if algo == "index" else pkg.ALGO_AUTO
            for _ in range(3):
                got = sel.run_queries(cfg.tau, pkg.MODE_CB_SMH, r, b, algo=run_algo)
            st = sel.stats()
            q = timed_passes(sel, lambda: sel.run_queries(cfg.tau, pkg.MODE_CB_SMH, r, b, algo=run_algo, fetch=False), passes)
            q.update({"selected": len(got), "stats": st, "pairs_per_s": n_q * n_d / (q["median_ms"] * 1e-3)})
            if algo == "index":
                q.update({"algo": "index", "query_db_index_builds": sel.get_param("query_db_index_builds")})
        q["query_db_sig_builds"] = sel.get_param("query_db_sig_builds")
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
            same = same_records(want, got)
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
    ap.add_argument("--algo", choices=("sig", "index", "both"), default="sig", help="stage 1 of the query pass: as chosen by the library, ALGO_INDEX, or both compared")
    ap.add_argument("--rounds", type=int, default=3, help="--algo both: rounds of --passes per algorithm, in alternation (at least 3)")
    a = ap.parse_args()
    res = []
    ok = True
    for name in a.only.split(","):
        r = bench(name, a.passes, a.criterion, a.algo, a.rounds)
        print(json.dumps(r), flush=True)
        res.append(r)
        if "union" in r and not r["union"]["identical"]:
            ok = False
        if not r.get("index_identical_to_sig", True):
            ok = False
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
