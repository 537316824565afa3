"""Register / scratch budget of the count kernels of csrc/validation.hip (mask_counts, confusion_counts) and csrc/sampling.hip
(label_hist): streaming kernels, so no scratch at all; validation.hip states "<= 128 VGPRs, four waves per SIMD" for its kernels
(built from the helpers of csrc/count_stream.hpp), and label_hist keeps what it took when those helpers were split off.
Reads the code object metadata only.  Cross-compiles to gfx950 assembly; no GPU."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _asm, _kernel_meta

LABEL_HIST_VGPRS = 26      # label_hist's vgpr_count at commit 2dae377, the last one before csrc/count_stream.hpp


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.isfile(HIPCC), reason="hipcc not available")
@pytest.mark.parametrize("src,kernels,budget", [("validation", {"mask_counts": 2, "confusion_counts": 4}, 128),
                                                ("sampling", {"label_hist": 1}, LABEL_HIST_VGPRS)])
def test_count_kernels_use_no_scratch_and_stay_inside_their_vgpr_budget(tmp_path, src, kernels, budget):
    meta = _kernel_meta(_asm(tmp_path, src))
    for kernel, count in kernels.items():                  # C = 19 and the runtime-C path, with and without reliability tables
        assert sum(kernel in n for n in meta) == count, sorted(meta)
    assert sum(kernels.values()) == len(meta), sorted(meta)      # every kernel of the file
    for name, (scratch, vgprs, _) in sorted(meta.items()):
        print("{}: {} VGPRs, {} B scratch".format(name, vgprs, scratch))
        assert scratch == 0, (name, scratch)
        assert vgprs <= budget, (name, vgprs)
