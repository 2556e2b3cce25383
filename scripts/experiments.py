#!/usr/bin/env python3
"""The reference's two experiment methods as runnable artefacts (run_comparison_experiment.sh:57-112, run_time_experiment.sh).

  experiments.py compare -l LIST [-a AUX_BYTES ...] [-h TAU] [-o comparison_cpu_gpu.csv] [--cpu oracle|reference]
      runs a CPU program (the oracle CLI, or the reference's own `selection` where oracle/_ref exists) and the MI355X
      `bin/selection` on the same file list, keys every output line by "name1_name2" and writes
          cfg,card1,card2,sim_cpu,sim_gpu,diff          (diff < eps printed as 0, eps = 1e-6: the reference's columns)
      Unlike the reference's `join`, pairs present on one side only are NOT dropped: they are written with an empty
      similarity on the other side, and the exit code is 1 if there is any such pair or any diff >= eps.
  experiments.py time -l LIST | -N GENOMES [-m BUCKETS ...] [-h TAU] [-R REPS] [-t THREADS] [-o experiment_smh.csv]
      impl,threads,mh_size,rep,criterio,tiempo    rows for cpu (oracle library: the OpenMP loop of selection.cpp:270-291,
      modes smh_a and CB+smh_a of time_smh.cpp) and gpu (bin/time_smh_hip records `list;label;tau;seconds`)
  experiments.py recall -l LIST [-a AUX_BYTES] | --cfg NAME [-N GENOMES]  [-h TAU ...] [-c CRITERION ...] [--modes cb nocb] [--min-matches C ...] [--min-containment G ...] [-p P_AUX] [--fold -p P_AUX ...] [-o recall.csv]
      what every criterion loses against the pass without one (criterion none: every pair inside the CB bound, or every pair, to the
      HLL-14 Jaccard test), on the MI355X, for a file list or a synthetic configuration of synth.py:
          cfg,criterion,aux,tau,mode,selected,exhaustive,missed,recall,ms_criterion,ms_exhaustive
      "missed" comes from a keyed join of the two record sets; a pair of a criterion that the exhaustive pass does not hold (or
      holds with another Jaccard value) is an error, not a row.  Criteria: smh_a, hll_a, hll_an, hll_a+smh_a, smh_c.  smh_c (at least c of
      the m buckets equal) gives one row per count threshold of --min-matches, "aux" = m<m>c<c>; without the option the threshold is
      min_matches(m, tau), the count at which the SuperMinHash estimate c / m reaches tau.  --min-containment G ...: smh_c with its
      per-pair threshold for a minimum containment G (Selector.set_min_containment), one row per G, "aux" = m<m>g<G>; with
      --min-matches as well, one row per (C, G), C the floor under the per-pair threshold, "aux" = m<m>c<C>g<G>.
      --fold: the auxiliary HLL sketches of hll_a, hll_an and hll_a+smh_a are folded on the device from the main registers
      (Selector.fold_aux_hll) instead of read from .hll_<p> files or generated: their rows are produced for EVERY precision given
      with -p (4 .. 14), from the .hll files alone; the rows of the other criteria come once.
"""
import argparse
import csv
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
BIN = ROOT / "cuda_selection_criteria_amd" / "bin"
EPS = 1e-6


def lines_to_map(text):
    out = {}
    for ln in text.splitlines():
        f = ln.split()
        if len(f) == 3:
            out[f"{f[0]}_{f[1]}"] = (f[0], f[1], float(f[2]))
    return out


def compare(args):
    cpu_bin = ROOT / "oracle" / ("_ref/selection" if args.cpu == "reference" else "selection_oracle_cli")
    if not cpu_bin.exists():
        sys.exit(f"{cpu_bin} missing")
    rows, bad = [], 0
    for a in args.a:
        cfg = f"t{args.t}_m{a}"
        cpu = subprocess.run([str(cpu_bin), "-l", args.l, "-t", str(args.t), "-h", args.tau, "-a", str(a), "-c", args.c],
                             capture_output=True, text=True, check=True).stdout
        gpu = subprocess.run([str(BIN / "selection"), "-l", args.l, "-h", args.tau, "-a", str(a), "-b", "128", "-c", args.c],
                             capture_output=True, text=True, check=True).stdout
        mc, mg = lines_to_map(cpu), lines_to_map(gpu)
        for key in sorted(set(mc) | set(mg)):
            c, g = mc.get(key), mg.get(key)
            n1, n2 = (c or g)[0], (c or g)[1]
            if c is None or g is None:
                rows.append([cfg, n1, n2, "" if c is None else c[2], "" if g is None else g[2], "missing"])
                bad += 1
                continue
            d = abs(c[2] - g[2])
            if d < EPS:
                d = 0
            else:
                bad += 1
            rows.append([cfg, n1, n2, c[2], g[2], d])
    with open(args.o, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["cfg", "card1", "card2", "sim_cpu", "sim_gpu", "diff"])
        w.writerows(rows)
    print(f"comparison complete: {len(rows)} pairs in '{args.o}', {bad} mismatching")
    return 1 if bad else 0


def timing(args):
    import numpy as np
    import oracle_py
    import cuda_selection_criteria_amd as pkg
    orc = oracle_py.Oracle()
    rows = []
    for m in args.m:
        for rep in range(1, args.R + 1):
            # ---- gpu: bin/time_smh_hip prints list;label;tau;seconds
            cmd = [str(BIN / "time_smh_hip"), "-h", args.tau, "-m", str(m), "-b", "256"]
            cmd += ["-l", args.l, "-D"] if args.l else ["-N", str(args.N)]       # -D: sketch files from disk (the CPU side below loads the same files)
            out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
            for ln in out.splitlines():
                f = ln.split(";")
                if len(f) >= 4 and f[1] in ("build_smh", "smh_a", "CB+smh_a"):
                    rows.append(["gpu", 256, m, rep, f[1], f[3]])
            # ---- cpu: the oracle's OpenMP loop on the same sketches
            if args.l:
                ds = pkg.load_dataset(args.l, m, 0)
                hll, aux, cards = ds.hll, ds.aux, ds.cards
            else:
                cfg = pkg.SynthConfig("time", args.N, m, float(args.tau), 0x5EED0000)
                hll, aux, _ = pkg.synth_host(cfg)
                cards = orc.cards(hll)
                perm = pkg.sort_by_card(cards)
                hll, aux, cards = hll[perm], aux[perm], cards[perm]
            r, b = pkg.banding(m, float(args.tau))
            for label, use_cb in (("smh_a", False), ("CB+smh_a", True)):
                t0 = time.perf_counter()
                orc.select(hll, aux, cards, float(args.tau), r, b, use_cb=use_cb, threads=args.t)
                rows.append(["cpu", args.t, m, rep, label, f"{time.perf_counter() - t0:.6f}"])
    with open(args.o, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["impl", "threads", "mh_size", "rep", "criterio", "tiempo"])
        w.writerows(rows)
    print(f"done, results in {args.o}")
    return 0


RECALL_CRITERIA = {"smh_a": 0, "hll_a": 1, "hll_an": 2, "hll_a+smh_a": 3, "smh_c": 5}


def recall_rows(sel, cfg_name, n, m, p_aux, taus, criteria, modes, min_matches=(), min_containment=()):
    """rows of the recall table for the sketches loaded in `sel` (a Selector; auxiliary HLL sketches loaded if a criterion needs
    them).  Times: host clock around one synchronous pass (the second of two: the first sizes the lists), results left on the device."""
    import numpy as np
    import cuda_selection_criteria_amd as pkg

    def timed(tau, mode, r, b):
        sel.run(tau, mode, r, b, fetch=False)
        t0 = time.perf_counter()
        got = sel.run(tau, mode, r, b)
        return got, (time.perf_counter() - t0) * 1e3

    rows = []
    for tau in taus:
        for mode_name in modes:
            mode = pkg.MODE_CB_SMH if mode_name == "cb" else pkg.MODE_SMH
            sel.set_criterion(pkg.CRIT_NONE)
            full, ms_full = timed(tau, mode, 1, 1)
            key_full = full["i"].astype(np.int64) * n + full["k"]
            # (smh_c: one row per count threshold -- per minimum containment, or per pair of the two, when those are given)
            if min_containment:
                counts = [(c, g) for c in (list(min_matches) or [None]) for g in min_containment]
            else:
                counts = [(c, None) for c in (list(min_matches) or [pkg.min_matches(m, tau)])]
            for name, (c_min, gamma) in [(c, t) for c in criteria for t in (counts if c == "smh_c" else [(None, None)])]:
                smh = name in ("smh_a", "hll_a+smh_a")
                r, b = pkg.banding(m, tau) if smh else (1, 1)
                sel.set_criterion(RECALL_CRITERIA[name])
                if c_min is not None:
                    sel.set_min_matches(c_min)
                if name == "smh_c":
                    sel.set_min_containment(gamma)                       # (None clears it: the fixed rule)
                got, ms = timed(tau, mode, r, b)
                key = got["i"].astype(np.int64) * n + got["k"]
                pos = np.minimum(np.searchsorted(key_full, key), max(len(key_full) - 1, 0))
                ok = len(key) == 0 or (len(key_full) > 0 and np.array_equal(key_full[pos], key)
                                       and np.array_equal(full["jaccard"][pos].view(np.uint64), got["jaccard"].view(np.uint64)))
                if not ok:
                    raise RuntimeError(f"{cfg_name} {name} tau {tau} {mode_name}: a selected pair is not in the exhaustive result")
                aux = f"m{m}" if name == "smh_a" else f"m{m}" + (f"c{c_min}" if c_min is not None else "") + (f"g{gamma:g}" if gamma is not None else "") if name == "smh_c" else f"p{p_aux}" if not smh else f"p{p_aux}+m{m}"
                rows.append([cfg_name, name, aux, tau, mode_name, len(got), len(full), len(full) - len(got),
                             f"{len(got) / len(full):.6f}" if len(full) else "", f"{ms:.3f}", f"{ms_full:.3f}"])
    return rows


RECALL_HEADER = ["cfg", "criterion", "aux", "tau", "mode", "selected", "exhaustive", "missed", "recall", "ms_criterion", "ms_exhaustive"]


def recall(args):
    import numpy as np
    import cuda_selection_criteria_amd as pkg
    need_aux = any(c not in ("smh_a", "smh_c") for c in args.c)
    need_smh = any(c in ("smh_a", "hll_a+smh_a", "smh_c") for c in args.c)
    if len(args.p) > 1 and not args.fold:
        sys.exit("recall: several -p precisions need --fold (without it the one precision's .hll_<p> files are read)")
    fold_ps = args.p if args.fold and need_aux else []
    args.p = 0 if fold_ps else args.p[0]                                 # (folding: no auxiliary file is read, none is generated)
    with pkg.Selector(0) as sel:
        if args.l:
            m = args.a // 8 if need_smh else 0
            p_aux = args.p if need_aux else 0
            ds = pkg.load_dataset(args.l, m, p_aux)
            n, name = len(ds.names), Path(args.l).name
            sel.upload(ds.hll, ds.aux if m else np.zeros((n, 1), dtype=np.uint64), ds.cards)
            if p_aux:
                sel.upload_aux_hll(ds.aux_hll, p_aux)
            keep = ds
        else:
            base = pkg.SYNTH_CONFIGS[args.cfg]
            base = base.scaled(args.N) if args.N else base
            p_aux = (base.p_aux or args.p) if need_aux else 0
            cfg = pkg.SynthConfig(base.name, base.n_genomes, base.m, base.tau, base.seed, p_aux, base.cluster_size, base.mode, base.n_sh_lo, base.n_sh_hi)
            keep = pkg.synth_device(cfg, device=0)
            n, m, name = cfg.n_genomes, cfg.m, args.cfg + (f"@{args.N}" if args.N else "")
            sel.attach(keep[0], keep[1], keep[2])
            if p_aux:
                sel.attach_aux_hll(keep[4], p_aux)
        taus = [float(t) for t in args.tau]
        if fold_ps:
            rows = []
            for idx, p_fold in enumerate(fold_ps):
                sel.fold_aux_hll(p_fold)
                crits = [c for c in args.c if idx == 0 or c not in ("smh_a", "smh_c")]
                rows += recall_rows(sel, name, n, m, p_fold, taus, crits, args.modes, args.min_matches, args.min_containment)
        else:
            rows = recall_rows(sel, name, n, m, p_aux, taus, args.c, args.modes, args.min_matches, args.min_containment)
    with open(args.o, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(RECALL_HEADER)
        w.writerows(rows)
    print(f"recall: {len(rows)} rows in '{args.o}'")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter, add_help=False)
    ap.add_argument("--help", action="help")
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("compare", add_help=False)
    c.add_argument("-l", required=True); c.add_argument("-a", type=int, nargs="+", default=[512]); c.add_argument("-h", dest="tau", default="0.01")
    c.add_argument("-t", type=int, default=8); c.add_argument("-c", default="smh_a"); c.add_argument("-o", default="comparison_cpu_gpu.csv")
    c.add_argument("--cpu", choices=["oracle", "reference"], default="oracle")
    t = sub.add_parser("time", add_help=False)
    t.add_argument("-l", default=""); t.add_argument("-N", type=int, default=0); t.add_argument("-m", type=int, nargs="+", default=[512])
    t.add_argument("-h", dest="tau", default="0.9"); t.add_argument("-R", type=int, default=1); t.add_argument("-t", type=int, default=8)
    t.add_argument("-o", default="experiment_smh_comparative.csv")
    rc = sub.add_parser("recall", add_help=False)
    rc.add_argument("-l", default=""); rc.add_argument("--cfg", default=""); rc.add_argument("-N", type=int, default=0)
    rc.add_argument("-a", type=int, default=2048); rc.add_argument("-p", type=int, nargs="+", default=[8]); rc.add_argument("--fold", action="store_true")
    rc.add_argument("-h", dest="tau", nargs="+", default=["0.9"]); rc.add_argument("-c", nargs="+", default=list(RECALL_CRITERIA), choices=list(RECALL_CRITERIA))
    rc.add_argument("--modes", nargs="+", default=["cb"], choices=["cb", "nocb"]); rc.add_argument("-o", default="recall.csv")
    rc.add_argument("--min-matches", dest="min_matches", type=int, nargs="+", default=[])
    rc.add_argument("--min-containment", dest="min_containment", type=float, nargs="+", default=[])
    args = ap.parse_args()
    if args.cmd == "time" and not args.l and not args.N:
        sys.exit("time: give -l LIST or -N GENOMES")
    if args.cmd == "recall" and bool(args.l) == bool(args.cfg):
        sys.exit("recall: give -l LIST or --cfg NAME")
    sys.exit(compare(args) if args.cmd == "compare" else recall(args) if args.cmd == "recall" else timing(args))


if __name__ == "__main__":
    main()
