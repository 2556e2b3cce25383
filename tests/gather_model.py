"""The winner-takes-all screen of include/selection_hip.h section 2m in plain numpy: the definition, nothing of the library."""
import numpy as np

GATHER_DTYPE = np.dtype([("q", "<i4"), ("d", "<i4"), ("unique", "<i4"), ("matches", "<i4")])
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def gather(Q, D, c_min=1, max_picks=64):
    """(picks GATHER_DTYPE compacted: queries ascending, each in pick order; n_picks [n_q] int32; unexplained [n_q] int32)"""
    Q, D = np.asarray(Q, dtype=np.uint64), np.asarray(D, dtype=np.uint64)
    picks = []
    n_picks, left = np.zeros(len(Q), dtype=np.int32), np.zeros(len(Q), dtype=np.int32)
    for q, row in enumerate(Q):
        live = row != EMPTY                                            # L_0 = valid
        M = (D == row[None, :]) & live[None, :]                        # M(d), on all 64 bits
        while len(D) and n_picks[q] < max_picks:
            c = (M & live[None, :]).sum(axis=1)
            d = int(np.argmax(c))                                      # the first maximum: ties go to the smaller rank
            if c[d] < c_min:
                break
            picks.append((q, d, int(c[d]), int(M[d].sum())))
            live = live & ~M[d]
            n_picks[q] += 1
        left[q] = live.sum()
    return np.array(picks, dtype=GATHER_DTYPE).reshape(-1), n_picks, left
