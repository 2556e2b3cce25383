"""The numpy model of the merge by group: np.maximum.at / np.minimum.at per group, and nothing else."""
import numpy as np


def merge(rows, groups, n_groups, op):
    """rows [n, w] reduced to [n_groups, w] by groups [n] (-1 = in no group): op "max" from 0 (HLL registers), "min" from ~0 (buckets)"""
    rows = np.asarray(rows)
    groups = np.asarray(groups, dtype=np.int64)
    out = np.full((n_groups, rows.shape[1]), 0 if op == "max" else np.iinfo(rows.dtype).max, dtype=rows.dtype)
    keep = groups >= 0
    (np.maximum if op == "max" else np.minimum).at(out, groups[keep], rows[keep])
    return out


def sizes(groups, n_groups):
    groups = np.asarray(groups, dtype=np.int64)
    return np.bincount(groups[groups >= 0], minlength=n_groups).astype(np.int32)


def merge_all(hll, smh, aux_hll, groups, n_groups):
    """the dict merge_sketches returns"""
    return {"hll": None if hll is None else merge(hll, groups, n_groups, "max"),
            "smh": None if smh is None else merge(smh, groups, n_groups, "min"),
            "aux_hll": None if aux_hll is None else merge(aux_hll, groups, n_groups, "max"),
            "sizes": sizes(groups, n_groups)}
