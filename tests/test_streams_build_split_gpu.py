"""selhip_build_sketches_split on a caller's non-blocking stream: the inputs are written and the outputs filled on that stream right
before the call, h_offsets is NULL (the entry copies the offsets back on the stream), and the rows are the oracle's once the call
returns.  The other checks of the entry are tests/test_build_split_gpu.py; this one creates a torch stream and sits beside the suite's
other stream tests (tests/test_streams_gpu.py), so that the tests in front of them run in a process that has created none, as before."""
import ctypes as C

import numpy as np
import pytest

from test_build_split_gpu import Reference, assert_rows_equal, build_oracle, stream_genomes  # noqa: F401  (build_oracle: the fixture)

pytestmark = pytest.mark.gpu


def test_on_a_callers_stream(build_oracle, tmp_path):  # noqa: F811
    import torch
    from cuda_selection_criteria_amd._lib import BuildInfo, hip_lib
    k, m, p_aux = 31, 64, 8
    genomes = stream_genomes()
    ref = Reference(build_oracle, tmp_path, genomes, m, p_aux, k)

    lib = hip_lib()
    dev = torch.device("cuda", 0)
    n = len(genomes)
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(g) for g in genomes])
    # the inputs wait on the device; the copies into the arrays the entry reads are device-side work of the caller's stream
    src_codes = torch.from_numpy(np.concatenate(genomes)).to(dev)
    src_off = torch.from_numpy(offsets).to(dev)
    d_codes = torch.zeros_like(src_codes)
    d_off = torch.zeros_like(src_off)
    d_hll = torch.empty((n, 16384), dtype=torch.uint8, device=dev)
    d_smh = torch.empty((n, m), dtype=torch.int64, device=dev)
    d_aux = torch.empty((n, 1 << p_aux), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(device=dev)
    info = BuildInfo()
    with torch.cuda.stream(stream):
        d_codes.copy_(src_codes, non_blocking=True)
        d_off.copy_(src_off, non_blocking=True)
        d_hll.fill_(0xAB)
        d_smh.fill_(0x2B)
        d_aux.fill_(0xAB)
        rc = lib.selhip_build_sketches_split(d_codes.data_ptr(), d_off.data_ptr(), None, n, k, m, p_aux, 64, d_hll.data_ptr(), d_smh.data_ptr(),
                                             d_aux.data_ptr(), C.byref(info), stream.cuda_stream)
    assert rc == 0, lib.selhip_last_error(None)
    got = (d_hll.cpu().numpy(), d_smh.cpu().numpy().view(np.uint64), d_aux.cpu().numpy())
    assert_rows_equal(got, ref.oracle, "caller's stream")
    assert (info.split_genomes, info.fallback_genomes) == (3, 1)
