"""bench.py's process handling, checked without a GPU: `python bench.py --gpus N` (N > 1, no torch.distributed environment) must start
its own ranks as a child `torch.distributed.run` and hand the child's exit status back (it used to stop with an error
before launching anything); without an MI355X the ranks refuse to run -- there is no CPU fallback -- so the status is non-zero."""
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.timeout(240)
def test_bench_starts_its_own_ranks_and_propagates_their_status():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: this is the no-GPU behaviour check")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1"],
                       capture_output=True, text=True, timeout=200)
    assert r.returncode != 0
    assert "needs an MI355X" in r.stderr and "must be launched with torch.distributed.run" not in r.stderr
    assert r.stderr.count("needs an MI355X") >= 2                       # both ranks were started
    r1 = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "1", "--warmup", "1"], capture_output=True, text=True, timeout=200)
    assert r1.returncode != 0 and "needs an MI355X" in r1.stderr       # N = 1: same refusal, no spawn


def test_write_outputs_sorts_and_bounds_the_dump(tmp_path, monkeypatch):
    """--dump-outputs: the frames' records (record 0 of a frame = its count) come out sorted by (i, k) as float64 arrays; a list longer
    than DUMP_MAX_PAIRS is cut to the same seeded sample every time"""
    import numpy as np
    import bench
    from cuda_selection_criteria_amd.selection import PAIR_DTYPE

    rng = np.random.default_rng(1)
    frames = np.zeros((2, 9, 2), dtype=np.int64)                 # two ranks, capacity 8 records each
    recs = []
    for r, cnt in enumerate((5, 3)):
        p = np.zeros(cnt, dtype=PAIR_DTYPE)
        p["i"], p["k"], p["jaccard"] = rng.integers(0, 50, cnt), rng.integers(50, 100, cnt), rng.random(cnt)
        frames[r, 0, 0] = cnt
        frames[r, 1:1 + cnt] = p.view(np.int64).reshape(cnt, 2)
        recs.append(p)
    want = np.concatenate(recs)
    want = want[np.lexsort((want["k"], want["i"]))]
    bench.write_outputs(tmp_path / "a", frames, (100, 20, 8))
    got = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("pair_i", "pair_k", "jaccard", "stats")}
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["pair_i"], want["i"]) and np.array_equal(got["pair_k"], want["k"])
    assert np.array_equal(got["jaccard"], want["jaccard"]) and list(got["stats"]) == [100, 20, 8]
    with pytest.raises(AssertionError):
        bench.write_outputs(tmp_path / "b", frames, (100, 20, 7))          # the frames must hold every selected pair

    monkeypatch.setattr(bench, "DUMP_MAX_PAIRS", 4)
    for d in ("c", "d"):
        bench.write_outputs(tmp_path / d, frames[0], (100, 20, 5))
    one, two = np.load(tmp_path / "c" / "pair_i.npy"), np.load(tmp_path / "d" / "pair_i.npy")
    assert len(one) == 4 and np.array_equal(one, two) and np.all(np.diff(one) >= 0)


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_dumps_the_pairs_of_its_last_timed_step(tmp_path):
    """`bench.py --steps 3 --warmup 1 --dump-outputs DIR` (the default workload): the headline line without the --full objects, and
    DIR/*.npy == the pairs and counters of one pass over the same seeded set, bit for bit"""
    import json

    import numpy as np

    import cuda_selection_criteria_amd as pkg
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=500)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["steps"] == 3 and d["unit"] == "pairs/s" and d["higher_is_better"] is True and d["dtype"] == "u64"
    assert d["value"] == pytest.approx(d["config"]["pairs_per_step"] / (d["ms_per_step"] * 1e-3), rel=1e-9)
    assert not {"roofline", "stream_kernel", "harder_workload", "cpu_baseline", "pcie_inclusive"} & set(d)

    cfg = pkg.SYNTH_CONFIGS["cfg3"]
    hll_t, aux_t, cards_t, _, _ = pkg.synth_device(cfg)
    nr, nb = pkg.banding(cfg.m, cfg.tau)
    with pkg.Selector(0) as sel:
        sel.attach(hll_t, aux_t, cards_t)
        want = sel.run(cfg.tau, pkg.MODE_SMH, nr, nb)
        st = sel.stats()
    want = want[np.lexsort((want["k"], want["i"]))]
    assert 0 < len(want) == d["config"]["selected_pairs"]
    assert np.array_equal(np.load(tmp_path / "pair_i.npy"), want["i"].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "pair_k.npy"), want["k"].astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "jaccard.npy").view(np.uint64), want["jaccard"].view(np.uint64))
    assert list(np.load(tmp_path / "stats.npy")) == [st["evaluated"], st["survivors"], st["selected"]]
