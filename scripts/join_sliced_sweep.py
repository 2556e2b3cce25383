#!/usr/bin/env python3
"""development sweep of the LDS-tile signature join (GPU box): packed minimum (join_form 0) against the bit-sliced form (join_form 2)
over candidate groups per wave (join_t), waves per block (join_wpb) and tile height (join_qt; 0 = automatic).  The variants take turns
over three rounds of 20 timed passes (HIP-event kernel averages); one line per variant with the median of the rounds.  Every variant
must report the same stats.
   usage: join_sliced_sweep.py [workload ...]"""
import statistics
import sys
from pathlib import Path
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import cuda_selection_criteria_amd as pkg

VARIANTS = {  # (form, T, wpb, qt)
    "small": [(0, 1, 4, 0), (2, 1, 4, 32), (2, 1, 8, 32), (2, 1, 4, 64), (2, 1, 8, 64), (2, 2, 4, 32), (2, 2, 4, 64), (2, 2, 8, 32)],
    "large": [(0, 1, 4, 0), (2, 1, 4, 128), (2, 1, 8, 128), (2, 1, 4, 64), (2, 1, 8, 64), (2, 2, 4, 128), (2, 2, 4, 64), (2, 2, 8, 128)],
}
KERNELS = ("sigbuild", "join", "verify", "total")
for wl in sys.argv[1:] or ("cfg3", "cfg4"):
    cfg = pkg.SYNTH_CONFIGS[wl]
    hll, aux, cards, _, _ = pkg.synth_device(cfg)
    r, b = pkg.banding(cfg.m, cfg.tau)
    sel = pkg.Selector(0); sel.attach(hll, aux, cards)
    variants = VARIANTS["small" if cfg.n_genomes < 20000 else "large"]
    ref, times = None, {v: [] for v in variants}
    for rnd in range(3):
        for form, t, wpb, qt in variants:
            sel.set_param("join_form", form); sel.set_param("join_t", t); sel.set_param("join_wpb", wpb); sel.set_param("join_qt", qt)
            for _ in range(2): sel.run(cfg.tau, pkg.MODE_SMH, r, b, algo=pkg.ALGO_SIG, fetch=False)
            st = sel.stats()
            if ref is None: ref = st
            assert st == ref, (wl, form, t, wpb, qt, st, ref)
            sel.timing(True)
            for _ in range(20): sel.run(cfg.tau, pkg.MODE_SMH, r, b, algo=pkg.ALGO_SIG, fetch=False)
            times[(form, t, wpb, qt)].append([sel.kernel_ms(k) * 1e3 for k in KERNELS])
            sel.timing(False)
    for (form, t, wpb, qt), ts in times.items():
        sel.set_param("join_qt", qt)
        med = [statistics.median(x[i] for x in ts) for i in range(len(KERNELS))]
        print(wl, "form=%d T=%d wpb=%d qt=%3d (tile %3d)" % (form, t, wpb, qt, sel.get_param("join_tile_rows")),
              " ".join("%s=%.1f" % (k, v) for k, v in zip(KERNELS, med)), "us; totals", " ".join("%.1f" % x[3] for x in ts), "OK", flush=True)
    sel.close()
    del hll, aux, cards
