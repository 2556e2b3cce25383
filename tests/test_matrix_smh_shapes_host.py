"""What the public header says about the kernels of the SuperMinHash matrices, without a GPU: the two read-only names of
selhip_ctx_get_param and the hook that forces the generic kernel.  (host_plan.hpp exports nothing of the matrix
plan: the unit arithmetic of the new kernels is matrix_units with another tile height, run by tests/test_matrix_smh_shapes_gpu.py.)"""
import re

from conftest import ROOT


def test_header_names_the_kernels():
    text = re.sub(r"\s*\n \*\s*", " ", (ROOT / "include" / "selection_hip.h").read_text())
    assert '"matrix_smh_path_used" (the kernel of the last matrix call with a SuperMinHash measure, section 2f: 1 = the whole-row register tile, 0 = any other kernel; -1 = none yet)' in text
    used = text[text.index('"matrix_smh_kernel_used"'):][:700]
    for word in ("0 = generic", "1 = the whole-row register tile", "2 = the narrow kernel of m = 32 or 64", "3 = the wide kernel", "-1 = none yet", '"matrix_smh_generic"'):
        assert word in used, word
