"""The two spanning-forest entries on a caller's non-blocking stream: the inputs are written and the outputs filled on that stream right
before the call, and the outputs are the model's once the call returns.  The other checks of the entries are tests/test_forest_gpu.py;
this one creates a torch stream and sits beside the suite's other stream tests (tests/test_streams_gpu.py), so that the tests in front
of them run in a process that has created none, as before."""
import ctypes as C

import numpy as np
import pytest

import forest_model as FM
from test_cluster_gpu import sparse_random, with_noise
from test_smhv_gpu import case, configure, zeros_hll

pytestmark = pytest.mark.gpu


def test_building_block_on_a_callers_stream():
    import torch
    from cuda_selection_criteria_amd import PAIR_DTYPE
    from cuda_selection_criteria_amd._lib import hip_lib
    n = 5000
    edges = with_noise(sparse_random(n, 6000, 21), n, 22).astype(np.int32)
    values = np.random.default_rng(23).integers(0, 50, size=len(edges)) / 50.0
    k, lab = FM.kruskal(FM.records_of(edges, values), n)
    lib = hip_lib()
    dev = torch.device("cuda", 0)
    src_pairs, src_vals = torch.from_numpy(edges).to(dev), torch.from_numpy(values).to(dev)
    d_pairs, d_vals = torch.full_like(src_pairs, -1), torch.zeros_like(src_vals)            # (-1: an invalid entry until the copy lands)
    d_edges = torch.empty((n - 1, 16), dtype=torch.uint8, device=dev)
    d_label = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(device=dev)
    f, rounds = C.c_int64(-5), C.c_int64(-5)
    with torch.cuda.stream(stream):
        d_pairs.copy_(src_pairs, non_blocking=True)
        d_vals.copy_(src_vals, non_blocking=True)
        d_edges.fill_(0xAB)
        d_label.fill_(-77)
        rc = lib.selhip_spanning_forest(d_pairs.data_ptr(), d_vals.data_ptr(), len(edges), n, d_edges.data_ptr(), d_label.data_ptr(), C.byref(f),
                                        C.byref(rounds), stream.cuda_stream)
    assert rc == 0, lib.selhip_last_error(None)
    assert f.value == len(k) and rounds.value == FM.boruvka_rounds(FM.records_of(edges, values), n)[2]
    got = d_edges.cpu().numpy()
    assert got[:f.value].reshape(-1).view(PAIR_DTYPE).tobytes() == FM.as_records(k).tobytes() and np.all(got[f.value:] == 0xAB)
    assert d_label.cpu().numpy().tolist() == lab


def test_context_entry_on_a_callers_stream():
    import torch
    from cuda_selection_criteria_amd import MODE_SMH, PAIR_DTYPE, Selector
    from cuda_selection_criteria_amd._lib import Forest, check
    n, m = 300, 128
    aux, cards = case(n, m)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with Selector(0) as sel:
        sel.set_stream(stream.cuda_stream)
        sel.upload(zeros_hll(n), aux, cards)
        configure(sel, c_min=1)
        rec = sel.run(-1.0, MODE_SMH, 7, 3)
        k, lab = FM.kruskal(FM.records_of_pass(rec), n)
        d_edges = torch.empty((n - 1, 16), dtype=torch.uint8, device=dev)
        d_label = torch.empty(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        cnt = C.c_int64(-5)
        with torch.cuda.stream(stream):
            d_edges.fill_(0xAB)                                                   # the fills are the stream's work: the call runs behind them
            d_label.fill_(-77)
            out = Forest(d_edges.data_ptr(), d_label.data_ptr())
            check(sel._lib.selhip_ctx_spanning_forest(sel._ctx, float("-inf"), C.byref(out), C.byref(cnt)), sel._ctx)
        got = d_edges.cpu().numpy()
        assert cnt.value == len(k) and got[:len(k)].reshape(-1).view(PAIR_DTYPE).tobytes() == FM.as_records(k).tobytes() and np.all(got[len(k):] == 0xAB)
        assert d_label.cpu().numpy().tolist() == lab
        sel.set_stream(None)
