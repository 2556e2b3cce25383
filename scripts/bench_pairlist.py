#!/usr/bin/env python3
"""GPU box: pair-list passes (selhip_ctx_run_pairs) -- the two stage-1 routes against each other, against the
all-pairs pass and against the drop-in launchers' explicit-list path on the same list.  Nothing is gated and no ratio is required.
Workload: cfg3 (10 000 genomes, m 512, tau 0.8, smh_a, MODE_SMH).  A list of P entries is min(|S|, P / 2) pairs of the all-pairs result S
(all of S where it fits) in random orientation plus uniformly random valid pairs, shuffled; P in {n/8, n/2, 4n, 10^6, 10^7}.
Timed in alternation, round by round in one process after warm passes of every shape, --rounds passes each (median, min .. max):
  sig        run_pairs, ALGO_SIG (signature build + one check per entry; "sig_cache" off, so every pass builds)
  sig_cached the same with "sig_cache" = 1 (the build is skipped after the first pass)
  direct     run_pairs, ALGO_STREAM
  allpairs   the all-pairs pass of the same context (what a caller without a list pass runs and filters)
  launcher   launch_kernel_smh64 with the explicit list + a device synchronise
  launcher@--lib   the same call into another build of the library (--lib PATH: a build of the parent commit is the baseline)
Wall time from before the call to after its synchronise, host clock; the passes leave their records on the device (no fetch).
Every list pass is compared with the filtered all-pairs result once, before the timing.  "crossover": the smallest P at which the
signature route's median is at or below the direct route's -- ALGO_AUTO switches at n / 2 (host_pairs.hpp, kPairsSigShare).
usage: bench_pairlist.py [--out profiles/pairlist_bench.json] [--rounds 60] [--lib PATH] [--sizes 1250,5000,...]"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import cuda_selection_criteria_amd as pkg  # noqa: E402
from cuda_selection_criteria_amd import ALGO_SIG, ALGO_STREAM, MODE_SMH  # noqa: E402
from cuda_selection_criteria_amd._lib import HIP_SYMBOLS  # noqa: E402


def spread(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x)), "rounds": len(x)}


def make_list(S, n, P, rng):
    keep = min(len(S), P // 2)
    pick = rng.choice(len(S), keep, replace=False)
    base = np.stack([S["i"][pick], S["k"][pick]], axis=1).astype(np.int32)
    flip = rng.random(keep) < 0.5
    base[flip] = base[flip][:, ::-1]
    x = rng.integers(0, n, P - keep, dtype=np.int32)
    y = ((x + rng.integers(1, n, P - keep, dtype=np.int32)) % n).astype(np.int32)
    L = np.concatenate([base, np.stack([x, y], axis=1)])
    rng.shuffle(L)
    return np.ascontiguousarray(L, dtype=np.int32), keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pairlist_bench.json"))
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--lib", default=None, help="another build of libselhip.so whose explicit-list launcher is timed beside this tree's")
    ap.add_argument("--sizes", default=None, help="comma-separated list lengths (default n/8, n/2, 4n, 10^6, 10^7)")
    a = ap.parse_args()
    if pkg.hip_lib().selhip_device_count() <= 0:
        sys.exit("bench_pairlist.py: no MI355X (gfx950) device: nothing is measured without one")
    import torch
    cfg = pkg.SYNTH_CONFIGS["cfg3"]
    n, tau = cfg.n_genomes, cfg.tau
    r, b = pkg.banding(cfg.m, tau)
    hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg)
    sizes = [int(s) for s in a.sizes.split(",")] if a.sizes else [n // 8, n // 2, 4 * n, 10 ** 6, 10 ** 7]
    launchers = {"launcher": pkg.hip_lib().launch_kernel_smh64}
    if a.lib:
        other = C.CDLL(a.lib)                                                # local scope: only its launcher is called
        other.launch_kernel_smh64.restype, other.launch_kernel_smh64.argtypes = HIP_SYMBOLS["launch_kernel_smh64"]
        launchers["launcher@--lib"] = other.launch_kernel_smh64
    rng = np.random.default_rng(0x9A125)
    res = {"workload": "cfg3", "n_genomes": n, "m": cfg.m, "tau": tau, "n_rows": r, "n_bands": b, "rounds": a.rounds, "lib": a.lib, "lists": []}
    ok = True
    with pkg.Selector(0) as sel, pkg.Selector(0) as cached:
        cached.set_param("sig_cache", 1)
        for s in (sel, cached):
            s.attach(hll_t, aux_t, cards_t)
        S = sel.run(tau, MODE_SMH, r, b)
        res["selected_all_pairs"] = len(S)
        s_key = S["i"].astype(np.int64) * n + S["k"]                         # ascending: the fetch sorts by (i, k)
        s_bits = S["jaccard"].view(np.uint64)
        for P in sizes:
            L, kept = make_list(S, n, P, rng)
            L_t = torch.from_numpy(L).to("cuda")
            out_t = torch.zeros(12 * (P + 1), dtype=torch.uint8, device="cuda")
            cnt_t = torch.zeros(1, dtype=torch.int64, device="cuda")

            def launcher(fn):
                rc = fn(hll_t.data_ptr(), aux_t.data_ptr(), cards_t.data_ptr(), L_t.data_ptr(), P, float(np.float32(tau)), cfg.m, 1 << 14, r, b,
                        out_t.data_ptr(), cnt_t.data_ptr(), 256)
                torch.cuda.synchronize()
                return rc

            variants = {"sig": lambda: sel.run_pairs(L_t, tau, MODE_SMH, r, b, algo=ALGO_SIG, fetch=False),
                        "sig_cached": lambda: cached.run_pairs(L_t, tau, MODE_SMH, r, b, algo=ALGO_SIG, fetch=False),
                        "direct": lambda: sel.run_pairs(L_t, tau, MODE_SMH, r, b, algo=ALGO_STREAM, fetch=False),
                        "allpairs": lambda: sel.run(tau, MODE_SMH, r, b, fetch=False)}
            for name, fn in launchers.items():
                variants[name] = (lambda f: lambda: launcher(f))(fn)
            # every route once against the filtered all-pairs result (and the warm passes of every shape)
            l_key = np.sort(L.min(axis=1).astype(np.int64) * n + L.max(axis=1))
            at = np.minimum(np.searchsorted(s_key, l_key), max(len(s_key) - 1, 0))
            hit = s_key[at] == l_key if len(s_key) else np.zeros(len(l_key), dtype=bool)
            want_key, want_bits = l_key[hit], s_bits[at[hit]]
            same = {}
            for name in ("sig", "sig_cached", "direct"):
                variants[name]()
                got = (sel if name != "sig_cached" else cached).fetch()
                same[name] = bool(np.array_equal(got["i"].astype(np.int64) * n + got["k"], want_key) and
                                  np.array_equal(got["jaccard"].view(np.uint64), want_bits))
            for name in launchers:
                assert variants[name]() == 0
                same[name] = int(cnt_t.cpu()[0]) == len(want_key)
            ok = ok and all(same.values())
            for _ in range(3):
                for fn in variants.values():
                    fn()
            wall = {name: [] for name in variants}
            for _ in range(a.rounds):
                for name, fn in variants.items():
                    t0 = time.perf_counter()
                    fn()
                    wall[name].append((time.perf_counter() - t0) * 1e3)
            row = {"P": P, "entries_from_S": kept, "records": len(want_key), "identical": same, "wall_ms": {k: spread(v) for k, v in wall.items()}}
            print(json.dumps(row), flush=True)
            res["lists"].append(row)
            del L_t, out_t
    at = [row["P"] for row in res["lists"] if row["wall_ms"]["sig"]["median"] <= row["wall_ms"]["direct"]["median"]]
    res["crossover"] = {"smallest_P_with_sig_at_or_below_direct": min(at) if at else None, "auto_switches_at": n // 2}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
