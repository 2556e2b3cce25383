#!/usr/bin/env python3
"""GPU box: sketches merged by group on the device (selhip_ctx_merge_groups) against its yardsticks, alternated
round by round in ONE child process (started here under its own time limit) after warm calls, on the cfg3 set of 10 000 genomes with
m = 512, main and SuperMinHash rows (16 KiB + 4 KiB per genome, 205 MB):
  merge     device time of selhip_ctx_merge_groups writing the merged registers, buckets and sizes (no cardinalities), for three groupings:
              balanced    the 1 000 clusters of 10 the generator planted
              singletons  G = n: every row a group of its own
              giant       one group of n: SELHIP_MERGE_SEGMENT-row segments, then the partial rows again
  gather    device time of selhip_permute_rows over the same main and SuperMinHash rows under a random permutation: it reads the bytes
            the merge reads and writes all of them, where the balanced merge writes a tenth
  grouping  device time of the same entry with no sketch output: the counting sort alone (count, scan, scatter and its read-back)
  host      (3 times, recorded only) wall time of the route the call replaces: the rows copied to pageable host memory, then numpy
            maximum.at / minimum.at over the balanced grouping
Each grouping's result is compared with numpy before it is timed, and again behind the last round.  The aims -- balanced: merge median
<= gather median + grouping median + (gather max - gather median); giant: merge median <= balanced median + one launch (taken as the
grouping's fastest call / its launches) + (balanced max - balanced median) -- are reported as "within_aim"; the figures are written as
they are either way and the script exits 0 unless a result differs.  Median (min .. max) of --rounds rounds on one device; nothing
beyond one device and this set is measured.
usage: bench_merge.py [--out profiles/merge_bench.json] [--rounds 20] [--limit 900] [--segment S]"""
import argparse
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import cuda_selection_criteria_amd as pkg  # noqa: E402
from cuda_selection_criteria_amd import SynthConfig  # noqa: E402
from cuda_selection_criteria_amd._lib import Merged, check  # noqa: E402

M_BUCKETS = 512
GROUPING_LAUNCHES = 5            # memsets aside: count, pack, scan (two kernels of the library call), scatter


def spread(x):
    return {"median": float(np.median(x)), "min": float(np.min(x)), "max": float(np.max(x)), "rounds": len(x)}


def model(rows, groups, n_groups, op):
    out = np.full((n_groups, rows.shape[1]), 0 if op == "max" else np.iinfo(rows.dtype).max, dtype=rows.dtype)
    (np.maximum if op == "max" else np.minimum).at(out, groups, rows)
    return out


def bench(rounds, segment):
    import torch
    gen = pkg.SYNTH_CONFIGS["cfg3"]
    n = gen.n_genomes
    cfg = SynthConfig("merge:cfg3", n, M_BUCKETS, gen.tau, gen.seed ^ 0x4D52, cluster_size=gen.cluster_size, mode=gen.mode, n_sh_lo=gen.n_sh_lo,
                      n_sh_hi=gen.n_sh_hi)
    hll_t, aux_t, cards_t, perm, _ = pkg.synth_device(cfg)
    dev = hll_t.device
    lib = pkg.hip_lib()
    hll, aux = hll_t.cpu().numpy(), aux_t.cpu().numpy().view(np.uint64)
    groupings = {"balanced": (np.asarray(perm) // gen.cluster_size).astype(np.int32), "singletons": np.arange(n, dtype=np.int32),
                 "giant": np.zeros(n, dtype=np.int32)}
    row_bytes = (1 << 14) + 8 * M_BUCKETS
    out = {"set": "cfg3", "n_genomes": n, "m": M_BUCKETS, "p": 14, "row_bytes": row_bytes, "input_bytes": n * row_bytes, "rounds": rounds,
           "segment": segment, "lines": {}}
    ok = True

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    shuffle = torch.from_numpy(np.random.default_rng(7).permutation(n).astype(np.int32)).to(dev)
    g_hll, g_aux = torch.empty_like(hll_t), torch.empty_like(aux_t)

    def gather():
        check(lib.selhip_permute_rows(hll_t.data_ptr(), g_hll.data_ptr(), shuffle.data_ptr(), n, 1 << 14, None))
        check(lib.selhip_permute_rows(aux_t.data_ptr(), g_aux.data_ptr(), shuffle.data_ptr(), n, 8 * M_BUCKETS, None))

    with pkg.Selector(0) as sel:
        sel.attach(hll_t, aux_t, cards_t)
        state = {}
        for name, groups in groupings.items():
            G = int(groups.max()) + 1
            d_groups = torch.from_numpy(groups).to(dev)
            o_hll = torch.empty((G, 1 << 14), dtype=torch.uint8, device=dev)
            o_aux = torch.empty((G, M_BUCKETS), dtype=torch.int64, device=dev)
            o_size = torch.empty(G, dtype=torch.int32, device=dev)
            full = Merged(o_hll.data_ptr(), o_aux.data_ptr(), None, None, o_size.data_ptr())
            sizes_only = Merged(None, None, None, None, o_size.data_ptr())

            def merge(out_struct=full, d_groups=d_groups, G=G):
                check(lib.selhip_ctx_merge_groups(sel._ctx, d_groups.data_ptr(), G, C.byref(out_struct)), sel._ctx)

            def identical(o_hll=o_hll, o_aux=o_aux, o_size=o_size, groups=groups, G=G):
                if G == n:
                    want_hll, want_aux = hll, aux
                elif G == 1:
                    want_hll, want_aux = hll.max(axis=0, keepdims=True), aux.min(axis=0, keepdims=True)
                else:
                    want_hll, want_aux = state["model"]
                return bool(np.array_equal(o_hll.cpu().numpy(), want_hll) and np.array_equal(o_aux.cpu().numpy().view(np.uint64), want_aux)
                            and np.array_equal(o_size.cpu().numpy(), np.bincount(groups, minlength=G)))

            if name == "balanced":
                # the host route, timed: rows to pageable host memory, then numpy per group
                host = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    h_hll, h_aux = hll_t.cpu().numpy(), aux_t.cpu().numpy().view(np.uint64)
                    state["model"] = (model(h_hll, groups, G, "max"), model(h_aux, groups, G, "min"))
                    host.append((time.perf_counter() - t0) * 1e3)
                out["host_route_wall_ms"] = spread(host)
            for _ in range(3):                                           # warm: scratch allocated, code loaded
                merge()
                merge(sizes_only)
                gather()
            same = identical()
            t = {"merge": [], "gather": [], "grouping": []}
            for _ in range(rounds):
                t["merge"].append(event_ms(merge))
                t["gather"].append(event_ms(gather))
                t["grouping"].append(event_ms(lambda: merge(sizes_only)))
            same = same and identical()
            mg, ga, gr = spread(t["merge"]), spread(t["gather"]), spread(t["grouping"])
            line = {"n_groups": G, "largest_group": int(np.bincount(groups).max()), "identical": same, "merge_ms": mg, "gather_ms": ga, "grouping_ms": gr,
                    "output_bytes": G * row_bytes, "merge_gb_per_s": float((n + G) * row_bytes / mg["median"] / 1e6),
                    "gather_gb_per_s": float(2 * n * row_bytes / ga["median"] / 1e6)}
            if name == "giant":
                bal = out["lines"]["balanced"]["merge_ms"]
                line["aim_ms"] = bal["median"] + gr["min"] / GROUPING_LAUNCHES + (bal["max"] - bal["median"])
            else:
                line["aim_ms"] = ga["median"] + gr["median"] + (ga["max"] - ga["median"])
            line["within_aim"] = bool(mg["median"] <= line["aim_ms"])
            out["lines"][name] = line
            ok = ok and same
    fold = ROOT / "profiles" / "fold_bench.json"
    if fold.exists():
        # a second yardstick for bytes per second: the fold kernel over the same set's main rows (scripts/bench_fold.py)
        rec = next((r for r in json.loads(fold.read_text()) if r.get("set") == "cfg3"), None)
        if rec:
            out["fold_gb_per_s_cfg3"] = {k: v["fold_gb_per_s"] for k, v in rec["per_p_aux"].items()}
    return out, ok


def child(a):
    if pkg.hip_lib().selhip_device_count() <= 0:
        sys.exit("bench_merge.py: no MI355X (gfx950) device: nothing is measured without one")
    r, good = bench(a.rounds, a.segment)
    print(json.dumps(r), flush=True)
    sys.exit(0 if good else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "profiles" / "merge_bench.json"))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--limit", type=int, default=900, help="seconds the measuring child process may take")
    ap.add_argument("--segment", type=int, default=pkg.MERGE_SEGMENT,
                    help="label of the record: the SELHIP_MERGE_SEGMENT the library under test was built with (a development build through SELHIP_LIB)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a)
    run = subprocess.run([sys.executable, __file__, "--child", "--rounds", str(a.rounds), "--segment", str(a.segment)], capture_output=True, text=True, timeout=a.limit)
    sys.stderr.write(run.stderr[-4000:])
    res = [json.loads(ln) for ln in run.stdout.splitlines() if ln.startswith("{")]
    for r in res:
        print(json.dumps(r), flush=True)
    if res:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(res, indent=1) + "\n")
    sys.exit(run.returncode)


if __name__ == "__main__":
    main()
