#!/usr/bin/env python3
"""GPU box: top-k of the all-pairs passes (selhip_ctx_set_allpairs_topk) against what a caller had to do without it, DESIGN.md
section 11.  Two routes to "every genome's K best partners in ranked order", alternated round by round in one process after warm passes:
  device  all-pairs pass with the setting on + fetch_ranked (regrouping, cut and ordering run on the device behind the pass)
  host    all-pairs pass with the setting off + fetch (the whole list over the link, the library's host sort) + the numpy below:
          the list mirrored (every record once per member), ranked, cut
Wall time from before the pass to the ranked list in host memory, median (min .. max) of --rounds rounds, the two results compared
record for record (owner, partner, J bits) in every round; a difference makes the script exit non-zero.  No ratio is required of
either route.  Also per workload: device time of the pass alone and of pass + cut (events around the call), and the "topk" timer next
to the pass's own ("total").
  N1  cfg3 (10 000 genomes, m 512, tau 0.8, smh_a): a sparse result
  N2  the same sketches hardened (bench.py --hard: a quarter of the genomes with degenerate buckets, a dense survivor graph)
  N3  criterion none, MODE_SMH, tau = -1 on 4 096 genomes: the exact k-NN graph, 8.4 M records
all with K = 10.
usage: bench_allpairs_topk.py [--out profiles/allpairs_topk_bench.json] [--rounds 20] [--only N1,N2,N3] [--k 10]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import cuda_selection_criteria_amd as pkg  # noqa: E402
from cuda_selection_criteria_amd import PAIR_DTYPE, SynthConfig  # noqa: E402

C = pkg.SYNTH_CONFIGS
SIGN = np.uint64(1 << 63)
WORKLOADS = {
    #       generator                                                            hardened  criterion        mode            tau
    "N1": (C["cfg3"], False, pkg.CRIT_SMH_A, pkg.MODE_SMH, C["cfg3"].tau),
    "N2": (C["cfg3"], True, pkg.CRIT_SMH_A, pkg.MODE_SMH, C["cfg3"].tau),
    "N3": (SynthConfig("N3: cfg3's recipe, 4096 genomes, m 64", 4096, 64, -1.0, C["cfg3"].seed ^ 0x0052), False, pkg.CRIT_NONE, pkg.MODE_SMH, -1.0),
}


def host_neighbours(S, k):
    """nbr(S, k) in ranked order from the fetched list: mirrored, then owner ascending, key(J) descending, partner ascending, cut"""
    D = np.empty(2 * len(S), dtype=PAIR_DTYPE)
    D[:len(S)] = S
    D["i"][len(S):], D["k"][len(S):], D["jaccard"][len(S):] = S["k"], S["i"], S["jaccard"]
    b = D["jaccard"].view(np.uint64)
    key = np.where((b & SIGN) != 0, ~b, b ^ SIGN)
    R = D[np.lexsort((D["k"], ~key, D["i"]))]
    at = np.arange(len(R))
    first = np.ones(len(R), dtype=bool)
    first[1:] = R["i"][1:] != R["i"][:-1]
    return R[at - np.maximum.accumulate(np.where(first, at, 0)) < k]


def same_records(a, b):
    return len(a) == len(b) and np.array_equal(a["i"], b["i"]) and np.array_equal(a["k"], b["k"]) and \
        np.array_equal(a["jaccard"].view(np.uint64), b["jaccard"].view(np.uint64))


def spread(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x)), "rounds": len(x)}


def bench(name, rounds, k):
    import torch
    cfg, hard, crit, mode, tau = WORKLOADS[name]
    hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg)                  # ascending cardinality
    n_degenerate = pkg.harden(aux_t) if hard else 0
    r, b = pkg.banding(cfg.m, tau) if crit == pkg.CRIT_SMH_A else (1, 1)
    out = {"workload": name, "n_genomes": cfg.n_genomes, "m": cfg.m, "tau": tau, "criterion": crit, "mode": mode, "degenerate_genomes": n_degenerate,
           "k": k, "rounds": rounds}
    with pkg.Selector(0) as sel:
        sel.set_criterion(crit)
        sel.attach(hll_t, aux_t, cards_t)

        def run(kk):
            sel.set_allpairs_topk(kk)
            sel.run(tau, mode, r, b, fetch=False)

        def device_ms(kk):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(kk)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        for kk in (0, k):                                                # warm: both shapes the timed rounds use
            for _ in range(3):
                run(kk)
        st = sel.stats()
        out.update(selected=st["selected"], survivors=st["survivors"], record_bytes=16 * st["selected"])
        wall = {"host": [], "device": []}
        dev = {"pass": [], "pass_topk": []}
        identical, reduced = True, 0
        for _ in range(rounds):
            t0 = time.perf_counter()
            run(0)
            want = host_neighbours(sel.fetch(), k)
            wall["host"].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            run(k)
            got = sel.fetch_ranked()
            wall["device"].append((time.perf_counter() - t0) * 1e3)
            identical = identical and same_records(got, want)
            reduced = len(got)
            dev["pass"].append(device_ms(0))
            dev["pass_topk"].append(device_ms(k))
        per_kernel = {}
        for kk in (0, k):
            sel.timing(1)
            for _ in range(5):
                run(kk)
            per_kernel[str(kk)] = {t: sel.kernel_ms(t) for t in ("topk", "dense", "total") if sel.kernel_ms(t) >= 0}
            sel.timing(0)
        sel.set_allpairs_topk(0)
        host, device = np.array(wall["host"]), np.array(wall["device"])
        out.update(reduced=reduced, identical=bool(identical), host_wall_ms=spread(host), device_wall_ms=spread(device),
                   device_faster_every_round=bool(np.all(device < host)), speedup_median=float(np.median(host) / np.median(device)),
                   pass_ms=spread(dev["pass"]), pass_topk_ms=spread(dev["pass_topk"]),
                   added_ms_median=float(np.median(dev["pass_topk"]) - np.median(dev["pass"])), kernel_ms=per_kernel)
    return out, bool(identical)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "allpairs_topk_bench.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--only", default="N1,N2,N3")
    ap.add_argument("--k", type=int, default=10)
    a = ap.parse_args()
    if pkg.hip_lib().selhip_device_count() <= 0:
        sys.exit("bench_allpairs_topk.py: no MI355X (gfx950) device: nothing is measured without one")
    res, ok = [], True
    for name in a.only.split(","):
        r, good = bench(name, a.rounds, a.k)
        print(json.dumps(r), flush=True)
        res.append(r)
        ok = ok and good
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
