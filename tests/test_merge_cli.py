"""`selection -P dir` on the influenza fixtures: one merged sketch set per cluster of a -L run or per group of a -I
file, against merge_from_filelist and the numpy model; the directory as a database of a further run; every refusal."""
import gzip
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import merge_model as M

import cuda_selection_criteria_amd as pkg
from cuda_selection_criteria_amd import MODE_SMH

pytestmark = pytest.mark.gpu

SEL = str(ROOT / "cuda_selection_criteria_amd" / "bin" / "selection")
LIST = "influenza_filelist.txt"


def run(args):
    return subprocess.run([SEL] + args, cwd=GOLDEN, capture_output=True, text=True)


def registers(path):
    raw = gzip.open(path, "rb").read()
    p = int(np.frombuffer(raw[16:20], dtype=np.uint32)[0])
    assert len(raw) == 28 + (1 << p), (path, len(raw), p)
    return np.frombuffer(raw[28:], dtype=np.uint8)


def buckets(path):
    raw = gzip.open(path, "rb").read()
    assert len(raw) == 4 + 8 * int(np.frombuffer(raw[:4], dtype=np.uint32)[0])
    return np.frombuffer(raw[4:], dtype=np.uint64)


def assert_directory(d, names, res, m, p_aux):
    """the files of -P: exactly the sets of `names`, holding the rows of res (Selector.merge on the host), and the list of them"""
    want = {"filelist.txt"} | {f"{nm}.hll" for nm in names} | ({f"{nm}.smh{m}" for nm in names} if m else set()) | \
           ({f"{nm}.hll_{p_aux}" for nm in names} if p_aux else set())
    assert {f.name for f in d.iterdir()} == want
    assert (d / "filelist.txt").read_text() == "".join(f"{d}/{nm}\n" for nm in names)
    for c, nm in enumerate(names):
        assert np.array_equal(registers(d / f"{nm}.hll"), res["hll"][c]), nm
        if m:
            assert np.array_equal(buckets(d / f"{nm}.smh{m}"), res["aux"][c]), nm
        if p_aux:
            assert np.array_equal(registers(d / f"{nm}.hll_{p_aux}"), res["aux_hll"][c]), nm


# (options of the pass, the -L options, merge_from_filelist's arguments, m, p_aux)
CASES = {"smh_a": (["-h", "0.5", "-a", "4096"], [], dict(aux_bytes=4096, tau=0.5), 512, 0),
         "hll_a-greedy": (["-h", "0.5", "-a", "256", "-c", "hll_a"], ["-Z", "greedy", "-Y", "max_rank"],
                          dict(aux_bytes=256, tau=0.5, criterion="hll_a", linkage="greedy", rep="max_rank"), 0, 8),
         "hll_a-folded": (["-h", "0.5", "-a", "256", "-c", "hll_a", "-D"], [], dict(aux_bytes=256, tau=0.5, criterion="hll_a", fold_aux=True), 0, 8),
         "none-T": (["-h", "0.3", "-a", "512", "-c", "none", "-n"], ["-T", "0.9"],
                    dict(aux_bytes=512, tau=0.3, criterion="none", mode=MODE_SMH, cluster_min=0.9), 0, 0)}


@pytest.mark.parametrize("name", list(CASES))
def test_clusters_merged_into_a_directory(monkeypatch, tmp_path, name):
    args, cluster_args, kw, m, p_aux = CASES[name]
    monkeypatch.chdir(GOLDEN)
    base = ["-l", LIST] + args
    plain, table = run(base), tmp_path / "clusters.tsv"
    with_l = run(base + ["-L", str(table)] + cluster_args)
    assert plain.returncode == 0 and with_l.returncode == 0 and with_l.stdout == plain.stdout, (plain.stderr, with_l.stderr)
    d, table_p = tmp_path / "merged", tmp_path / "clusters_p.tsv"
    with_p = run(base + ["-L", str(table_p)] + cluster_args + ["-P", str(d)])
    assert with_p.returncode == 0, with_p.stderr
    assert with_p.stdout == plain.stdout and table_p.read_bytes() == table.read_bytes()      # byte for byte what they are without -P
    ids = [int(ln.split("\t")[1]) for ln in table.read_text().splitlines()]
    n_clusters = max(ids) + 1
    res = pkg.merge_from_filelist(LIST, **kw)
    assert res["names"] == pkg.cluster_names(n_clusters) and len(res["sizes"]) == n_clusters
    assert sorted(np.bincount(ids).tolist()) == sorted(res["sizes"].tolist())
    assert_directory(d, res["names"], res, m, p_aux)
    if name == "none-T":
        assert 1 < n_clusters < len(ids)
    # the Python front end writes the same files
    d2 = tmp_path / "merged_py"
    pkg.merge_from_filelist(LIST, out_dir=str(d2), **kw)
    assert {f.name for f in d2.iterdir()} == {f.name for f in d.iterdir()}
    for f in d.iterdir():
        if f.name != "filelist.txt":
            assert gzip.open(f, "rb").read() == gzip.open(d2 / f.name, "rb").read(), f.name
    # the directory is a database
    again = run(["-l", str(d / "filelist.txt"), "-c", "none", "-n", "-h", "-1"])
    assert again.returncode == 0, again.stderr
    assert len(again.stdout.splitlines()) == n_clusters * (n_clusters - 1) // 2
    assert all(ln.split(" ")[0].startswith(f"{d}/cluster_") for ln in again.stdout.splitlines())


def test_groups_file(monkeypatch, tmp_path):
    monkeypatch.chdir(GOLDEN)
    listed = (GOLDEN / LIST).read_text().split()
    groups = tmp_path / "groups.tsv"
    # two groups, numbered by first appearance; listed[4] is in none
    member = {0: "beta", 1: "alpha", 2: "beta", 3: "alpha", 5: "beta", 6: "beta", 7: "alpha", 8: "alpha", 9: "beta"}
    groups.write_text("".join(f"{listed[j]}\t{g}\n" for j, g in member.items()) + "\n")
    d = tmp_path / "merged"
    out = run(["-l", LIST, "-a", "4096", "-I", str(groups), "-P", str(d)])
    assert out.returncode == 0 and out.stdout == "", out.stderr
    ds = pkg.load_dataset(LIST, 512)
    ids = np.array([-1 if ds.names[r] == listed[4] else ("beta", "alpha").index(member[listed.index(ds.names[r])]) for r in range(len(ds.names))], dtype=np.int32)
    want = {"hll": M.merge(ds.hll, ids, 2, "max"), "aux": M.merge(ds.aux, ids, 2, "min")}
    assert list(M.sizes(ids, 2)) == [5, 4]
    assert_directory(d, ["beta", "alpha"], want, 512, 0)
    res = pkg.merge_from_filelist(LIST, 4096, groups_file=str(groups))
    assert res["names"] == ["beta", "alpha"] and list(res["sizes"]) == [5, 4] and np.array_equal(res["groups"], ids)
    assert np.array_equal(res["hll"], want["hll"]) and np.array_equal(res["aux"], want["aux"])
    # with auxiliary sketches in play, read or folded
    for extra in ([], ["-D"]):
        d8 = tmp_path / ("merged_aux" + "".join(extra))
        out = run(["-l", LIST, "-a", "256", "-c", "hll_a", "-I", str(groups), "-P", str(d8)] + extra)
        assert out.returncode == 0, out.stderr
        ds8 = pkg.load_dataset(LIST, 0, 8)
        assert ds8.names == ds.names
        assert_directory(d8, ["beta", "alpha"], {"hll": want["hll"], "aux_hll": M.merge(ds8.aux_hll, ids, 2, "max")}, 0, 8)
    # the groups as a database: two sets, one pair
    again = run(["-l", str(d / "filelist.txt"), "-c", "none", "-n", "-h", "-1"])
    assert again.returncode == 0 and len(again.stdout.splitlines()) == 1, again.stderr


def test_groups_file_refused(tmp_path):
    listed = (GOLDEN / LIST).read_text().split()
    groups, d = tmp_path / "groups.tsv", tmp_path / "merged"
    for text, line in ((f"{listed[0]}\ta\nno_such_genome\ta\n", 2), (f"{listed[0]} a\n", 1), (f"{listed[0]}\t\n", 1), (f"{listed[0]}\ta\n\n{listed[1]}\tx/y\n", 3)):
        groups.write_text(text)
        out = run(["-l", LIST, "-a", "4096", "-I", str(groups), "-P", str(d)])
        assert out.returncode == 5 and out.stdout == "" and f"selection: -I: line {line} of" in out.stderr and not d.exists(), (text, out)
    out = run(["-l", LIST, "-a", "4096", "-I", str(tmp_path / "missing.tsv"), "-P", str(d)])
    assert out.returncode == 5 and "selection: -I: cannot read" in out.stderr and not d.exists()


def test_refusals(tmp_path):
    d, t, g = str(tmp_path / "merged"), str(tmp_path / "clusters.tsv"), str(tmp_path / "groups.tsv")
    base = ["-l", "/nonexistent/list.txt", "-h", "0.9", "-a", "256"]
    for args, word in ((base + ["-P", d], "-L"),                                        # -P without -L or -I
                       (base + ["-I", g], "-P"),                                        # -I without -P
                       (base + ["-L", t, "-I", g, "-P", d], "-I"),                      # -I together with -L
                       (base + ["-L", t, "-P", d, "-q", "/nonexistent/q.txt"], "-q"),
                       (base + ["-I", g, "-P", d, "-q", "/nonexistent/q.txt"], "-q"),
                       (["-l", "/nonexistent/list.txt", "-M", "/nonexistent/m.tsv", "-I", g, "-P", d], "-M"),
                       (["-l", "/nonexistent/list.txt", "-M", "/nonexistent/m.tsv", "-L", t, "-P", d], "-M"),
                       (base + ["-L", t, "-P", d, "-g", "2"], "-g"), (base + ["-I", g, "-P", d, "-g", "2"], "-g"),
                       (base + ["-L", t, "-P", d, "-B", "4"], "-B"), (base + ["-I", g, "-P", d, "-B", "4"], "-B"),
                       (["-r", "/nonexistent/results.bin", "-L", t, "-P", d], "-r"), (["-r", "/nonexistent/results.bin", "-I", g, "-P", d], "-r"),
                       (base + ["-I", g, "-P", d, "-K", "3"], "-K"), (base + ["-I", g, "-P", d, "-p", "/nonexistent/pairs.txt"], "-p"),
                       (base + ["-I", g, "-P", d, "-o", "/nonexistent/out.bin"], "-o")):
        out = run(args)
        assert out.returncode == 2 and out.stdout == "" and ("-P" in out.stderr or "-I" in out.stderr) and word in out.stderr, (args, out)
        assert "nonexistent" not in out.stderr and not list(tmp_path.iterdir()), (args, out.stderr)
    # accepted: the runs get as far as the list
    for args in (base + ["-L", t, "-P", d], base + ["-L", t, "-Z", "greedy", "-P", d], base + ["-I", g, "-P", d]):
        out = run(args)
        assert out.returncode not in (0, 2) and "No valid input file provided" in out.stderr and not list(tmp_path.iterdir()), (args, out)
    usage = run(["-x"])
    assert usage.returncode == 0 and "-P dir" in usage.stdout and "-I groups.tsv" in usage.stdout
