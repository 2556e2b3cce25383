#!/usr/bin/env python3
"""GPU box: the winner-takes-all screen (selhip_ctx_gather) stage by stage, beside the dense matrix over the
same rectangle and the host route.

  workloads  screen    1 000 queries (every 50th row of the set) x cfg4's 50 000 rows, m = 512
             mixture   10 queries, each the bucket-wise minimum of 20 rows of 20 different clusters, against the same 50 000
             dense     64 queries against the 50 000 rows with 8 buckets forged equal on every row and every query: each row a candidate
  c_min      1, 3, 16 (screen); 1, 3 (mixture, dense)

Every workload runs in a child process of its own under its own time limit.  Three warm calls, then `--reps` alternating rounds of
  gather   Selector.gather(c_min, 64, to_host=False) under the context's timers: "gather_mask" and "gather_pick", device ms per call
  matrix   Selector.query_matrix("smh_matches", f32) over the same rectangle into a kept tensor, device ms between two events
median (min ... max) each; picks and candidates per query; the pick stage per pick (us).  The aim for the mask stage follows from the
code: it streams the rows twice (count, then fill), so twice the yardstick's median plus the yardstick's own spread (max - min).  The
host route runs `--host-reps` times over the first 16 queries: both bucket arrays copied to the host plus tests/gather_model.py; its picks
are compared with the device's byte for byte.

`--shapes` measures the mask stage's narrow (m = 32, 64) and wide (m = 2048, 4096) kernels instead: the screen and
the mixture workload rebuilt at that m (cfg4's generator with m replaced), c_min = 3.  Three warm calls, then `--reps` rounds that
alternate the kernel of m, the same context under "gather_generic" = 1 (the route those m took before) and the matrix call; the aim is
the same rule, and the picks of the two routes are compared byte for byte.

usage: bench_gather.py [--out profiles/gather_bench.json] [--only screen:1,...] [--reps 20] [--host-reps 3] [--limit seconds]
       bench_gather.py --shapes all|32,64,2048,4096 [--out profiles/gather_shapes_bench.json] [--reps 20] [--limit seconds]
"""
import argparse
import dataclasses
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(ROOT / "tests"))

from bench_cluster import med  # noqa: E402

WORKLOADS = ("screen:1", "screen:3", "screen:16", "mixture:1", "mixture:3", "dense:1", "dense:3")
MAX_PICKS = 64
HOST_QUERIES = 16


SHAPES = (32, 64, 2048, 4096)
SHAPE_C_MIN = 3


def sets(kind, m=None):
    """(hll, aux, cards) of the database and the queries' bucket rows, device tensors; m: cfg4's generator at another row width"""
    import torch
    import cuda_selection_criteria_amd as pkg
    cfg = pkg.SYNTH_CONFIGS["cfg4"]
    hll, aux, cards, _, _ = pkg.synth_device(cfg if m is None else dataclasses.replace(cfg, m=m), device=0)
    if kind == "screen":
        return hll, aux, cards, aux[::50].contiguous()
    if kind == "mixture":
        flip = torch.tensor(-2 ** 63, dtype=torch.int64, device=aux.device)                     # unsigned order through the signed minimum
        rows = (torch.arange(10, device=aux.device)[:, None] * 5000 + torch.arange(20, device=aux.device)[None, :] * 250)
        return hll, aux, cards, ((aux[rows] ^ flip).min(dim=1).values ^ flip).contiguous()
    shared = torch.arange(1, 9, dtype=torch.int64, device=aux.device) * 1000003 + 17
    aux = aux.clone()
    aux[:, :8] = shared
    return hll, aux, cards, aux[::782][:64].contiguous()


def bench(kind, c_min, reps, host_reps):
    import torch
    import cuda_selection_criteria_amd as pkg
    import gather_model
    hll, aux, cards, q_aux = sets(kind)
    n_q, n_d, m = q_aux.shape[0], aux.shape[0], aux.shape[1]
    out = {"workload": f"{kind}:{c_min}", "n_q": n_q, "n_d": n_d, "m": m, "c_min": c_min, "max_picks": MAX_PICKS}
    with pkg.Selector(0) as sel:
        sel.attach(hll, aux, cards)
        sel.attach_queries(torch.zeros((n_q, 1 << 14), dtype=torch.uint8, device=aux.device), q_aux, torch.zeros(n_q, dtype=torch.float64, device=aux.device))
        kept = sel.query_matrix("smh_matches", torch.float32)
        valid = (q_aux != -1)
        out["candidates_per_query"] = float((kept >= c_min).sum().item()) / n_q       # (exact where no query bucket is unfilled: these sets)
        assert bool(valid.all())
        first = sel.gather(c_min, MAX_PICKS)
        out["picks_per_query"] = float(first["n_picks"].mean())
        out["lds_cap_bytes"] = sel.get_param("gather_lds_cap")

        def gather_ms():
            sel.timing(1)
            sel.gather(c_min, MAX_PICKS, to_host=False)
            t = sel.kernel_ms("gather_mask"), sel.kernel_ms("gather_pick")
            sel.timing(0)
            return t

        def matrix_ms():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            sel.query_matrix("smh_matches", torch.float32, out=kept)
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b)

        for _ in range(3):
            gather_ms()
            matrix_ms()
        mask, pick, matrix = [], [], []
        for r in range(reps):
            for what in ((0, 1) if r % 2 == 0 else (1, 0)):
                if what == 0:
                    a, b = gather_ms()
                    mask.append(a)
                    pick.append(b)
                else:
                    matrix.append(matrix_ms())
        out.update(mask_ms=med(mask), pick_ms=med(pick), matrix_ms=med(matrix))
        total_picks = max(int(first["n_picks"].sum()), 1)
        out["pick_us_per_pick_of_the_longest_query"] = round(1e3 * out["pick_ms"]["median"] / max(int(first["n_picks"].max()), 1), 3)
        out["pick_us_per_pick_overall"] = round(1e3 * out["pick_ms"]["median"] / total_picks, 4)
        out["mask_aim_ms"] = round(2 * out["matrix_ms"]["median"] + (out["matrix_ms"]["max"] - out["matrix_ms"]["min"]), 4)
        out["mask_within_the_aim"] = bool(out["mask_ms"]["median"] <= out["mask_aim_ms"])
        again = sel.gather(c_min, MAX_PICKS)
        out["same_picks_before_and_after"] = bool(again["picks"].tobytes() == first["picks"].tobytes())
        host_ms, equal = [], True
        hn = min(n_q, HOST_QUERIES)                                  # (the model takes ~50 ms per query and round at this width: a prefix of the queries)
        out["host_route_queries"] = hn
        for _ in range(host_reps):
            t0 = time.perf_counter()
            hq, hd = q_aux[:hn].cpu().numpy().view(np.uint64), aux.cpu().numpy().view(np.uint64)
            picks, _, _ = gather_model.gather(hq, hd, c_min, MAX_PICKS)
            host_ms.append(1e3 * (time.perf_counter() - t0))
            equal = equal and picks.tobytes() == first["picks"][first["picks"]["q"] < hn].tobytes()
        out["host_route_wall_ms"] = med(host_ms) if host_ms else "not measured"
        out["host_picks_equal"] = bool(equal) if host_ms else "not measured"
    return out


def bench_shape(kind, m, reps):
    """one workload at one m: the mask and pick timers under the kernel of m and under "gather_generic" = 1, and the matrix call"""
    import torch
    import cuda_selection_criteria_amd as pkg
    hll, aux, cards, q_aux = sets(kind, m)
    n_q, n_d, c_min = q_aux.shape[0], aux.shape[0], SHAPE_C_MIN
    out = {"workload": f"{kind}:{c_min}", "n_q": n_q, "n_d": n_d, "m": m, "c_min": c_min, "max_picks": MAX_PICKS}
    with pkg.Selector(0) as sel:
        sel.attach(hll, aux, cards)
        sel.attach_queries(torch.zeros((n_q, 1 << 14), dtype=torch.uint8, device=aux.device), q_aux, torch.zeros(n_q, dtype=torch.float64, device=aux.device))
        kept = sel.query_matrix("smh_matches", torch.float32)
        out["candidates_per_query"] = float((kept >= c_min).sum().item()) / n_q
        picks, used = {}, {}
        for generic in (0, 1):
            sel.set_param("gather_generic", generic)
            picks[generic] = sel.gather(c_min, MAX_PICKS)
            used[generic] = sel.get_param("gather_mask_kernel_used")
        out["mask_kernel_used"] = {"new": used[0], "generic": used[1]}
        out["picks_per_query"] = float(picks[0]["n_picks"].mean())
        out["picks_identical_to_generic"] = bool(all(picks[0][k].tobytes() == picks[1][k].tobytes() for k in ("picks", "n_picks", "unexplained")))

        def gather_ms(generic):
            sel.set_param("gather_generic", generic)
            sel.timing(1)
            sel.gather(c_min, MAX_PICKS, to_host=False)
            t = sel.kernel_ms("gather_mask"), sel.kernel_ms("gather_pick")
            sel.timing(0)
            return t

        def matrix_ms():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            sel.query_matrix("smh_matches", torch.float32, out=kept)
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b)

        calls = {"new": lambda: gather_ms(0), "generic": lambda: gather_ms(1), "matrix": matrix_ms}
        for _ in range(3):
            for call in calls.values():
                call()
        samples = {"new_mask": [], "new_pick": [], "generic_mask": [], "generic_pick": [], "matrix": []}
        names = list(calls)
        for r in range(reps):
            for name in names[r % 3:] + names[:r % 3]:
                t = calls[name]()
                if name == "matrix":
                    samples["matrix"].append(t)
                else:
                    samples[name + "_mask"].append(t[0])
                    samples[name + "_pick"].append(t[1])
        sel.set_param("gather_generic", 0)
        out.update({k + "_ms": med(v) for k, v in samples.items()})
        out["mask_aim_ms"] = round(2 * out["matrix_ms"]["median"] + (out["matrix_ms"]["max"] - out["matrix_ms"]["min"]), 4)
        out["mask_within_the_aim"] = bool(out["new_mask_ms"]["median"] <= out["mask_aim_ms"])
        out["generic_over_new"] = round(out["generic_mask_ms"]["median"] / out["new_mask_ms"]["median"], 2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="default profiles/gather_bench.json, with --shapes profiles/gather_shapes_bench.json")
    ap.add_argument("--shapes", default=None, help="the narrow / wide mask kernels instead of the workloads: a list of m out of 32,64,2048,4096, or 'all'")
    ap.add_argument("--only", default=",".join(WORKLOADS))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=300, help="seconds a workload's child process may take")
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        kind, c_min = args.worker.split(":")
        res = bench_shape(kind, int(c_min), args.reps) if args.shapes else bench(kind, int(c_min), args.reps, args.host_reps)
        print("RESULT " + json.dumps(res), flush=True)
        return 0
    results = []
    if args.shapes:
        shapes = SHAPES if args.shapes == "all" else tuple(int(x) for x in args.shapes.split(","))
        out_path = Path(args.out or "profiles/gather_shapes_bench.json")
        for m in shapes:
            for kind in ("screen", "mixture"):
                # (the worker's second field is m here) a fresh child process per line, under its own time limit; nothing more after a failure
                child = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, __file__, "--shapes", "1", "--worker", f"{kind}:{m}", "--reps",
                                        str(args.reps)], stdout=subprocess.PIPE, text=True)
                line = next((ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")), None)
                if child.returncode != 0 or line is None:
                    print(f"m = {m} {kind} ended with status {child.returncode}: stopping", file=sys.stderr, flush=True)
                    return 1
                r = json.loads(line[len("RESULT "):])
                results.append(r)
                print(f"m={m} {r['workload']}: mask {r['new_mask_ms']['median']} ms, generic {r['generic_mask_ms']['median']} ms ({r['generic_over_new']}x), aim "
                      f"{r['mask_aim_ms']}, within the aim: {'yes' if r['mask_within_the_aim'] else '**no**'}; pick {r['new_pick_ms']['median']} ms; matrix "
                      f"{r['matrix_ms']['median']} ms; picks identical: {r['picks_identical_to_generic']}", flush=True)
                out_path.parent.mkdir(parents=True, exist_ok=True)
                out_path.write_text(json.dumps({"device": "MI355X", "protocol": f"3 warm calls, {args.reps} alternating rounds", "lines": results}, indent=1) + "\n")
        return 0
    args.out = args.out or "profiles/gather_bench.json"
    for name in args.only.split(","):
        # a fresh child process per workload, under its own time limit; nothing more is started after one that failed
        child = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, __file__, "--worker", name, "--reps", str(args.reps),
                                "--host-reps", str(args.host_reps)], stdout=subprocess.PIPE, text=True)
        line = next((ln for ln in child.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if child.returncode != 0 or line is None:
            print(f"workload {name} ended with status {child.returncode}: stopping", file=sys.stderr, flush=True)
            return 1
        results.append(json.loads(line[len("RESULT "):]))
        r = results[-1]
        print(f"{r['workload']}: mask {r['mask_ms']['median']} ms (aim {r['mask_aim_ms']}), within the aim: {'yes' if r['mask_within_the_aim'] else '**no**'}; "
              f"pick {r['pick_ms']['median']} ms; matrix {r['matrix_ms']['median']} ms", flush=True)
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps({"device": "MI355X", "reps": args.reps, "host_reps": args.host_reps, "workloads": results}, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
