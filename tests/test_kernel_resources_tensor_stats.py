"""Register / scratch budget of the two kernels of dasac_tensor_stats (csrc/optim.hip): streaming reductions, so no scratch at
all and at most 64 VGPRs (full occupancy, 8 waves per SIMD).  Reads the code object metadata only.  Cross-compiles to gfx950
assembly; no GPU."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _asm, _kernel_meta


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.isfile(HIPCC), reason="hipcc not available")
def test_tensor_stats_kernels_use_no_scratch_and_fit_full_occupancy(tmp_path):
    txt = _asm(tmp_path, "optim")
    meta = _kernel_meta(txt)
    for kernel in ("tensor_stats_chunks", "tensor_stats_finish"):
        names = [n for n in meta if kernel in n]
        assert len(names) == 1, names
        scratch, vgprs, _ = meta[names[0]]
        print("{}: {} VGPRs, {} B scratch".format(kernel, vgprs, scratch))
        assert scratch == 0, scratch
        assert vgprs <= 64, vgprs
