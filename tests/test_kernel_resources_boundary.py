"""Register / scratch / LDS budget of the kernels of dasac_boundary_counts (csrc/boundary.hip): no scratch at all, at most 128 VGPRs
(four waves per SIMD, the budget of the counting kernels of csrc/validation.hip) and at most 64 KB of LDS per workgroup -- the
static segment from the code object, and the dynamic size the launch asks for at the largest R and C, restated from the file's own
layout.  Reads the code object metadata only.  Cross-compiles to gfx950 assembly; no GPU."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _asm, _kernel_meta


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.isfile(HIPCC), reason="hipcc not available")
def test_boundary_kernels_use_no_scratch_128_vgprs_and_64_kb_of_lds(tmp_path):
    txt = _asm(tmp_path, "boundary")
    meta = _kernel_meta(txt)
    names = sorted(meta)
    assert len(names) == 3 and sum("boundary_prepare" in n for n in names) == 2 and sum("boundary_stencil" in n for n in names) == 1, names
    for name in names:
        scratch, vgprs, lds = meta[name]
        print("{}: {} VGPRs, {} B scratch, {} B static LDS".format(name, vgprs, scratch, lds))
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128, (name, vgprs)
        assert lds <= 64 * 1024, (name, lds)
    # the stencil's LDS is dynamic: histogram [R+1][5][C] u32, row table [32+2R][64] u32, staged bytes [32+2R][64+2R]
    R, C = 16, 64
    assert ((R + 1) * 5 * C + (32 + 2 * R) * 64) * 4 + (32 + 2 * R) * (64 + 2 * R) <= 64 * 1024
