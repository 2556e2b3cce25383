"""What the public header says about the kernels of criterion smh_c's count pass, without a GPU: the two read-only names of
selhip_ctx_get_param, the four kinds and the hook that forces the generic kernel.  (smhc_kind is a constexpr of
the kernel translation unit and exported nowhere; what it returns is read back through "smhc_kernel_used" by
tests/test_smhc_shapes_gpu.py, where a context exists to refuse "smhc_generic" = 2 as well.)"""
import re

from conftest import ROOT


def test_header_names_the_kernels():
    text = re.sub(r"\s*\n \*\s*", " ", (ROOT / "include" / "selection_hip.h").read_text())
    assert 'get_param "smhc_path_used": the stage-1 kernel of the last such pass, 1 = the fast path (m = 128, 256, 512, 1024), 0 = any other kernel, -1 = none yet' in text
    used = text[text.index('get_param "smhc_kernel_used"'):][:900]
    for word in ("0 = generic", "1 = the whole-row register tile", "2 = the narrow kernel of m = 32 or 64", "3 = the wide kernel", "-1 = none yet", '"smhc_generic" 1',
                 "any other value is refused (SELHIP_E_BADARG)"):
        assert word in used, word
