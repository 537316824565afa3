"""Register / scratch budget of the kernels of dasac_view_consistency (csrc/consistency.hip): streaming counting kernels, so no
scratch at all and at most 128 VGPRs -- the budget csrc/validation.hip states for its counting kernels, four waves per SIMD.  Reads
the code object metadata only.  Cross-compiles to gfx950 assembly; no GPU."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _asm, _kernel_meta


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.isfile(HIPCC), reason="hipcc not available")
def test_view_consistency_kernels_use_no_scratch_and_keep_four_waves_per_simd(tmp_path):
    txt = _asm(tmp_path, "consistency")
    meta = _kernel_meta(txt)
    names = [n for n in meta if "view_consistency" in n]
    assert len(names) == 3, names                          # C = 19 with T = 2 and T = 4 compiled in, and the runtime path
    assert sorted(meta) == sorted(names), sorted(meta)     # every kernel of the file
    for name in names:
        scratch, vgprs, _ = meta[name]
        print("{}: {} VGPRs, {} B scratch".format(name, vgprs, scratch))
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128, (name, vgprs)
