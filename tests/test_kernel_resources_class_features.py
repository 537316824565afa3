"""Register / scratch budget of the kernels of csrc/class_features.hip.  The per-class accumulators of class_feature_planes must be
registers: a single byte of scratch means an accumulator array is indexed at run time, the one way that kernel goes badly wrong.
The VGPR budget is the one the file's header comment states, and that is at most 128 (at least 4 waves per SIMD).  Reads the code
object metadata only.  Cross-compiles to gfx950 assembly; no GPU."""
import os
import re
import shutil

import pytest

from test_kernel_resources import HIPCC, ROOT, _asm, _kernel_meta


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.isfile(HIPCC), reason="hipcc not available")
def test_class_feature_kernels_use_no_scratch_and_keep_four_waves_per_simd(tmp_path):
    src = open(os.path.join(ROOT, "da-sac_amd", "csrc", "class_features.hip")).read()
    stated = re.search(r"no scratch, <= (\d+) VGPRs", src[:src.index("#include")])
    assert stated, "the header comment of class_features.hip states its VGPR budget"
    budget = int(stated.group(1))
    assert budget <= 128, budget
    meta = _kernel_meta(_asm(tmp_path, "class_features"))
    kernels = {"label_nodes": 2, "class_feature_planes": 2, "class_feature_finish": 1}      # name fragment -> instantiations
    assert len(meta) == sum(kernels.values()), sorted(meta)
    for kernel, count in kernels.items():
        names = [n for n in meta if kernel in n]
        assert len(names) == count, names
        for name in names:
            scratch, vgprs, lds = meta[name]
            print("{}: {} VGPRs, {} B scratch, {} B LDS".format(name, vgprs, scratch, lds))
            assert scratch == 0, (name, scratch)
            assert vgprs <= budget, (name, vgprs)
