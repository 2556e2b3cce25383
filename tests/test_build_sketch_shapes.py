"""sketch_build_kernel (csrc/kernel_sketch.cuh) and its launcher selhip_build_sketches (csrc/abi_blocks.inc) at the
launch shapes, window edges, small sketch sizes and k-mer lengths that the fixture genomes of test_build_sketch.py do
not reach.  Every GPU comparison is exact byte equality with the sequential oracle (oracle/build_sketch_oracle.c):
HLL p = 14 registers, auxiliary registers, SuperMinHash words.  The oracle itself is checked first, without the
kernel, against a plain window scan written here (k = 1, 16, 31, 32).

Inputs are code strings (0..3 = ACGT, 4 = window reset) handed to build_from_codes, so that a reset lands on an exact
byte; the oracle reads the same genome as a one-record, unwrapped FASTA with N for code 4."""
import ctypes as C
import random

import numpy as np
import pytest

# The kernel's shape, restated on purpose: a change there should be followed by a deliberate change here.
SEG = 64                    # kernel_sketch.cuh: constexpr int kSketchSeg = 64;  (k-mer end positions rolled by one thread)
JMAX_PARALLEL = 15          # kernel_sketch.cuh: constexpr int kSketchJmaxParallel = 15;  (a beyond it: one sequential lane)
THREADS_FEW = 1024          # abi_blocks.inc: const unsigned threads = n_genomes < 2048 ? 1024u : (unsigned)kBlock;
THREADS_MANY = 256          # common.cuh: kBlock
MANY_GENOMES = 2048         # abi_blocks.inc: the same line's threshold
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def rand_codes(rng, n, resets=()):
    c = np.array([rng.randrange(4) for _ in range(n)], dtype=np.uint8) if n < 4096 else \
        np.random.default_rng(rng.randrange(1 << 30)).integers(0, 4, n).astype(np.uint8)
    for x in resets:
        c[x] = 4
    return c


def write_fastas(directory, genomes):
    """one plain one-record FASTA per genome, no line wrapping, code 4 -> N"""
    directory.mkdir(parents=True, exist_ok=True)
    lut = np.frombuffer(b"ACGTN", dtype=np.uint8)
    paths = []
    for j, c in enumerate(genomes):
        p = directory / f"g{j}.fna"
        p.write_bytes(b">g\n" + lut[c].tobytes() + b"\n")
        paths.append(p)
    return paths


@pytest.fixture(scope="module")
def build_oracle():
    import oracle_py
    return oracle_py.BuildOracle()


def oracle_rows(build_oracle, paths, m, p_aux, k=31):
    rows = [build_oracle.sketch(p, m=m, p_aux=p_aux, k=k) for p in paths]
    hll = np.stack([r[0] for r in rows])
    aux = np.stack([r[1] for r in rows]) if p_aux else None
    smh = np.stack([r[2] for r in rows]) if m else None
    return hll, smh, aux, [r[3] for r in rows]


def assert_rows_equal(got, want, what):
    """(hll, smh, aux) triples, row by row so that a failure names the genome"""
    for name, g, w in zip(("hll", "smh", "aux"), got, want):
        assert (g is None) == (w is None), (what, name)
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape)
        bad = [j for j in range(len(g)) if not np.array_equal(g[j], w[j])]
        assert not bad, (what, name, "rows", bad[:8], "of", len(g))


def check_against_oracle(build_oracle, directory, genomes, settings, k=31):
    """settings: [(m, p_aux)]; one GPU call and one oracle sweep per setting over the same files"""
    from cuda_selection_criteria_amd.build import build_from_codes
    paths = write_fastas(directory, genomes)
    out = {}
    for m, p_aux in settings:
        got = build_from_codes(genomes, m, p_aux, k, 0)
        hll, smh, aux, n = oracle_rows(build_oracle, paths, m, p_aux, k)
        assert_rows_equal(got, (hll, smh, aux), (k, m, p_aux))
        out[(m, p_aux)] = (got, n)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# B. the oracle against a plain window scan (no kernel)
# ---------------------------------------------------------------------------------------------------------------------
def scan_kmers(codes, k):
    """every window of k consecutive valid bases, as the 2k-bit integer with the first base most significant"""
    out = []
    for e in range(k - 1, len(codes)):
        w = codes[e - k + 1:e + 1]
        if (w < 4).all():
            v = 0
            for c in w:
                v = (v << 2) | int(c)
            out.append(v)
    return out


def py_canonical(kmer, k):
    rc = 0
    for t in range(k):
        rc = (rc << 2) | (3 - ((kmer >> (2 * t)) & 3))          # complement of base t from the end, placed from the front
    return min(kmer, rc)


def py_wang(key):
    key = (~key + (key << 21)) & M64
    key ^= key >> 24
    key = (key + (key << 3) + (key << 8)) & M64
    key ^= key >> 14
    key = (key + (key << 2) + (key << 4)) & M64
    key ^= key >> 28
    return (key + (key << 31)) & M64


def py_hll14(kmers, k):
    regs = np.zeros(16384, dtype=np.uint8)
    for v in kmers:
        h = py_wang(py_canonical(v, k))
        idx = h >> 50
        rest = h & ((1 << 50) - 1)
        rank = 50 - rest.bit_length() + 1                         # leading zeros of the remaining 50 bits, plus one (51 if none set)
        regs[idx] = max(regs[idx], rank)
    return regs


@pytest.mark.parametrize("k", [1, 16, 31, 32])
def test_oracle_kmer_stream_matches_window_scan(build_oracle, tmp_path, k):
    """the checker at every k the ABI accepts at its edges: k-mer count and p = 14 registers from a scan written here"""
    rng = random.Random(1000 + k)
    genomes = [rand_codes(rng, 100),                                                  # no reset: 101 - k k-mers
               rand_codes(rng, 400, resets=(0, 57, 58, 130, 399)),
               rand_codes(rng, 300, resets=[rng.randrange(300) for _ in range(6)]),
               rand_codes(rng, k), rand_codes(rng, max(k - 1, 0)), rand_codes(rng, 2 * k + 1, resets=(k,))]
    paths = write_fastas(tmp_path, genomes)
    for c, p in zip(genomes, paths):
        kmers = scan_kmers(c, k)
        hll, _, _, n = build_oracle.sketch(p, k=k)
        assert n == len(kmers), (k, len(c))
        assert np.array_equal(hll, py_hll14(kmers, k)), (k, len(c))
    assert len(scan_kmers(genomes[0], k)) == 101 - k


# ---------------------------------------------------------------------------------------------------------------------
# D. GPU
# ---------------------------------------------------------------------------------------------------------------------
SWEEP_SETTINGS = [(16, 5), (64, 5)]          # m = 16: parallel re-run branch; m = 64: sequential lane; p_aux = 5: 8 words of aregs


@pytest.mark.gpu
def test_reset_sweep(build_oracle, tmp_path):
    """one reset on every byte of a 260-base genome (first / last warm-up base, first / last end position of segments
    0..3), and two resets with k-1, k, k+1 valid bases between them (no k-mer, one, two) at 64 consecutive offsets"""
    k, n = 31, 260
    rng = random.Random(11)
    single = [rand_codes(rng, n, resets=(x,)) for x in range(n)]
    double = []
    for gap in (k - 1, k, k + 1):
        for s in range(40, 40 + SEG):                             # the window between the resets crosses the segment edges 94 and 158
            double.append(rand_codes(rng, n, resets=(s, s + 1 + gap)))
    res = check_against_oracle(build_oracle, tmp_path / "single", single, SWEEP_SETTINGS, k)
    assert res[SWEEP_SETTINGS[0]][1] == [max(x - k + 1, 0) + max(n - 1 - x - k + 1, 0) for x in range(n)]
    check_against_oracle(build_oracle, tmp_path / "double", double, SWEEP_SETTINGS, k)


@pytest.mark.gpu
def test_length_sweep(build_oracle, tmp_path):
    """every length 0..199: zero-length rows, L = k-1 (no k-mer), L = k (one), the ends of segments 0, 1 and 2"""
    k = 31
    rng = random.Random(12)
    genomes = [rand_codes(rng, n) for n in range(200)]
    assert k - 1 + 2 * SEG + 1 < 199                              # segment 2 is entered
    res = check_against_oracle(build_oracle, tmp_path, genomes, SWEEP_SETTINGS, k)
    for (m, p_aux), ((hll, smh, aux), n_kmers) in res.items():
        assert n_kmers == [max(n - k + 1, 0) for n in range(200)]
        for n in range(k):                                        # no k-mer: what the oracle gives for an empty input
            assert not hll[n].any() and not aux[n].any() and (smh[n] == EMPTY).all(), (m, n)
        assert hll[k].any() and (smh[k] != EMPTY).any()


@pytest.mark.gpu
def test_stride_wrap_1024_threads(build_oracle, tmp_path):
    """thread 0's second segment starts at W = k-1 + 64 * 1024: genomes that end just before, on and after it, and a
    reset on the first warm-up base of the wrapped segment"""
    k = 31
    W = k - 1 + SEG * THREADS_FEW
    rng = random.Random(13)
    genomes = [rand_codes(rng, n) for n in (W - 1, W, W + 1, W + SEG)]
    genomes.append(rand_codes(rng, 70001, resets=(W - (k - 1),)))
    res = check_against_oracle(build_oracle, tmp_path, genomes, [(64, 12)], k)
    assert res[(64, 12)][1][:4] == [W - k, W - k + 1, W - k + 2, W - k + 1 + SEG]
    assert res[(64, 12)][1][4] == 70001 - k + 1 - k


def many_genomes():
    """exactly 2 048 genomes: short random ones (a quarter with resets), four that wrap the 256-thread stride, four empty"""
    k = 31
    W = k - 1 + SEG * THREADS_MANY
    rng = random.Random(14)
    genomes = []
    for j in range(MANY_GENOMES - 8):
        n = rng.randint(20, 200)
        genomes.append(rand_codes(rng, n, resets=[rng.randrange(n) for _ in range(rng.randint(1, 3))] if j % 4 == 0 else ()))
    for at, n in ((100, W - 1), (700, W), (1300, W + 1), (1900, W + SEG)):
        genomes.insert(at, rand_codes(rng, n))
    for at in (1, 513, 1024, 2046):                               # zero-length rows between others
        genomes.insert(at, np.zeros(0, dtype=np.uint8))
    assert len(genomes) == MANY_GENOMES
    return genomes


@pytest.mark.gpu
def test_256_thread_launch(build_oracle, tmp_path):
    """the launch every real collection takes (n_genomes >= 2 048): stride, init and write-out loops and the sequential
    lane under a 4-wave block; then the same genomes under the 1 024-thread launch and in another order"""
    from cuda_selection_criteria_amd.build import build_from_codes
    genomes = many_genomes()
    W = 31 - 1 + SEG * THREADS_MANY
    assert sorted(len(g) for g in genomes)[-4:] == [W - 1, W, W + 1, W + SEG] and sum(len(g) == 0 for g in genomes) == 4
    res = check_against_oracle(build_oracle, tmp_path, genomes, [(64, 5), (16, 8)])
    big = res[(64, 5)][0]

    few = build_from_codes(genomes[:MANY_GENOMES - 1], 64, 5, 31, 0)             # 2 047 genomes: 1 024 threads
    assert_rows_equal(few, tuple(x[:MANY_GENOMES - 1] for x in big), "2047 of 2048")

    order = sorted(range(MANY_GENOMES), key=lambda j: (-len(genomes[j]), j))
    assert order != list(range(MANY_GENOMES))
    perm = build_from_codes([genomes[j] for j in order], 64, 5, 31, 0)
    assert_rows_equal(perm, tuple(x[order] for x in big), "sorted by length")


@pytest.mark.gpu
def test_small_m(build_oracle, tmp_path):
    """m = 1 .. 16 take the per-thread permutation map (m = 16: J = 15 fills it to its last entry), m = 32 is the
    first size that goes to the sequential lane"""
    k = 31
    rng = random.Random(15)
    genomes = [rand_codes(rng, k - 1 + n) for n in (1, 2, 3, 10, 30, 100, 1000)]
    genomes.append(np.zeros(300, dtype=np.uint8))                 # poly-A: 270 identical k-mers
    paths = write_fastas(tmp_path / "probe", genomes)
    assert JMAX_PARALLEL == 16 - 1                                # m = 16 is the largest size whose a = m-1 stays parallel
    smh16 = oracle_rows(build_oracle, paths, 16, 0, k)[1]
    filled_hi = [int((row[row != EMPTY] >> np.uint64(32)).max()) for row in smh16]
    assert max(filled_hi) >= 8, filled_hi                         # a chain that runs deep into the map
    assert any((row == EMPTY).any() for row in smh16)             # a bucket no step reaches: a stays m-1
    res = check_against_oracle(build_oracle, tmp_path / "run", genomes, [(m, 5) for m in (1, 2, 4, 8, 16, 32)], k)
    assert res[(16, 5)][1] == [1, 2, 3, 10, 30, 100, 1000, 270]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 16, 21, 32])
def test_kmer_length(build_oracle, tmp_path, k):
    """k is an ABI parameter: lengths that straddle k and the first segment edge, with resets"""
    rng = random.Random(160 + k)
    edge = k - 1 + SEG
    genomes = [rand_codes(rng, n) for n in (max(k - 1, 0), k, k + 1, edge - 1, edge, edge + 1, edge + 2, 300)]
    genomes += [rand_codes(rng, 300, resets=(0,)), rand_codes(rng, 300, resets=(k - 1, edge)),
                rand_codes(rng, 300, resets=(edge - k, edge + 1, 299)),
                rand_codes(rng, 500, resets=[rng.randrange(500) for _ in range(5)])]
    assert len(genomes) == 12
    res = check_against_oracle(build_oracle, tmp_path, genomes, [(16, 0), (64, 0)], k)
    assert res[(16, 0)][1][:4] == [0, 1, 2, SEG - 1]


@pytest.mark.gpu
def test_hot_spot_is_deterministic(build_oracle, tmp_path):
    """every k-mer of a genome contends for one or two registers and buckets (LDS CAS max / atomic min): two runs give
    the same bytes, and they are the oracle's"""
    from cuda_selection_criteria_amd.build import build_from_codes
    genomes = [np.tile(np.array([0, 1], dtype=np.uint8), 35000), np.full(70000, 3, dtype=np.uint8)]
    first = check_against_oracle(build_oracle, tmp_path, genomes, [(16, 4)])[(16, 4)][0]
    again = build_from_codes(genomes, 16, 4, 31, 0)
    assert_rows_equal(again, first, "second run")
    assert np.count_nonzero(first[0][0]) == 2 and np.count_nonzero(first[0][1]) == 1      # two canonical k-mers, one


@pytest.mark.gpu
def test_refusals():
    """argument checks of selhip_build_sketches, pinned: SELHIP_E_BADARG before any launch (the outputs keep their fill);
    n_genomes = 0 is OK and writes nothing.  Every buffer is large enough for the refused sizes."""
    import torch
    from cuda_selection_criteria_amd._lib import hip_lib
    lib = hip_lib()
    dev = torch.device("cuda", 0)
    codes = torch.from_numpy(rand_codes(random.Random(18), 100)).to(dev)
    off = torch.tensor([0, 100], dtype=torch.int64, device=dev)
    hll = torch.full((16384,), 0xAB, dtype=torch.uint8, device=dev)
    smh = torch.full((4096,), 0x2B2B2B2B2B2B2B2B, dtype=torch.int64, device=dev)
    aux = torch.full((1 << 13,), 0xAB, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    c, o, h, s, a = (t.data_ptr() for t in (codes, off, hll, smh, aux))

    def call(codes=c, off=o, n=1, k=31, m=64, p_aux=8, hll=h, smh=s, aux=a):
        return lib.selhip_build_sketches(codes, off, n, k, m, p_aux, hll, smh, aux, None)

    def untouched():
        assert lib.selhip_device_synchronize() == 0
        return bool((hll == 0xAB).all()) and bool((smh == 0x2B2B2B2B2B2B2B2B).all()) and bool((aux == 0xAB).all())

    BADARG = -1                                                   # selection_hip.h: SELHIP_E_BADARG
    refused = [dict(k=0), dict(k=33), dict(m=48), dict(m=4096), dict(p_aux=3), dict(p_aux=13),
               dict(codes=None), dict(off=None), dict(hll=None), dict(n=-1)]
    for kw in refused:
        assert call(**kw) == BADARG, kw
        assert lib.selhip_last_error(None), kw
    assert untouched()
    assert call(n=0) == 0 and untouched()
    # without the output pointer its size is not looked at
    assert call(m=48, smh=None, p_aux=13, aux=None) == 0
    assert lib.selhip_device_synchronize() == 0
    assert bool((hll != 0xAB).any()) and bool((smh == 0x2B2B2B2B2B2B2B2B).all()) and bool((aux == 0xAB).all())
