"""The fold of a HyperLogLog sketch to a lower precision, in numpy alone -- shares nothing with the library.

A hash h lands in register h >> (64 - p) with rank clz(((h << 1) | 1) << (p - 1)) + 1 (the reference's hll.h:886-888).  With
d = p - p_aux, an old index splits into its top p_aux bits g and d dropped bits t; at precision p_aux the dropped bits are the first d
bits the rank counts.  A non-empty register with t != 0 has the rank d - floor(log2 t) there, the one with t == 0 has d + r:

    out[g] = max over t in [0, 2^d) with r = in[(g << d) | t], r != 0 of (t == 0 ? d + r : d - floor(log2 t))     (0 if every r is 0)
"""
import numpy as np


def fold(hll: np.ndarray, p_aux: int) -> np.ndarray:
    """hll: u8 [n, 1 << p] (or [1 << p]) -> u8 [n, 1 << p_aux] (or [1 << p_aux])"""
    hll = np.asarray(hll, dtype=np.uint8)
    one = hll.ndim == 1
    rows = hll.reshape(1, -1) if one else hll
    n, width = rows.shape
    p = width.bit_length() - 1
    assert width == 1 << p and 0 <= p_aux <= p
    d = p - p_aux
    t = np.arange(1 << d, dtype=np.int32)
    log2t = np.zeros(1 << d, dtype=np.int16)
    for b in range(d):                                   # floor(log2 t) for t >= 1
        log2t[(t >> b) >= 1] = b
    out = np.zeros((n, 1 << p_aux), dtype=np.uint8)
    step = max(1, (1 << 22) >> p)                        # rows per slice: a few MiB of temporaries
    for lo in range(0, n, step):
        grp = rows[lo:lo + step].reshape(-1, 1 << p_aux, 1 << d).astype(np.int16)
        contrib = np.where(t == 0, d + grp, d - log2t)   # broadcast over the last axis
        contrib = np.where(grp != 0, contrib, 0)
        out[lo:lo + step] = contrib.max(axis=2).astype(np.uint8)
    return out[0] if one else out


def random_registers(rng: np.random.Generator, n: int, p: int, fill: float = 0.5) -> np.ndarray:
    """valid registers [n, 1 << p]: values 1 .. 64 - p + 1 with a geometric-like law, a share 1 - fill of them empty"""
    cap = 64 - p + 1
    r = np.minimum(rng.geometric(0.5, size=(n, 1 << p)), cap).astype(np.uint8)
    r[rng.random((n, 1 << p)) >= fill] = 0
    return r


def slot(h: int, p: int):
    """(register, rank) of a 64-bit hash at precision p, straight from hll.h:886-888"""
    idx = h >> (64 - p)
    lzt = (((h << 1) | 1) << (p - 1)) & 0xFFFFFFFFFFFFFFFF
    return idx, (64 - lzt.bit_length()) + 1


def sketch(hashes, p: int) -> np.ndarray:
    """the sketch a list of hashes builds at precision p"""
    out = np.zeros(1 << p, dtype=np.uint8)
    for h in hashes:
        i, r = slot(int(h), p)
        out[i] = max(out[i], r)
    return out
