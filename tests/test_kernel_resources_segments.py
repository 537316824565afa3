"""Register / scratch / LDS budget of the connected-component kernels (csrc/segments.hip): no scratch at all, at most 128 VGPRs (four
waves per SIMD, the budget of the other counting kernels) and at most 64 KB of LDS per workgroup -- the static segment from the
code object, and the dynamic size seg_tabulate's launch asks for at the largest C, restated from the file's own layout.  Reads the
code object metadata only.  Cross-compiles to gfx950 assembly; no GPU."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _asm, _kernel_meta

KERNELS = ("seg_local", "seg_merge", "seg_resolve", "seg_broadcast", "seg_filter_apply", "seg_prepare", "seg_tabulate")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.isfile(HIPCC), reason="hipcc not available")
def test_segment_kernels_use_no_scratch_128_vgprs_and_64_kb_of_lds(tmp_path):
    meta = _kernel_meta(_asm(tmp_path, "segments"))
    names = sorted(meta)
    # seg_resolve with and without the layer counters, seg_filter_apply for uint8 and int64 maps
    assert len(names) == 9 and all(sum(k in n for n in names) == (2 if k in ("seg_resolve", "seg_filter_apply") else 1) for k in KERNELS), names
    for name in names:
        scratch, vgprs, lds = meta[name]
        print("{}: {} VGPRs, {} B scratch, {} B static LDS".format(name, vgprs, scratch, lds))
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128, (name, vgprs)
        assert lds <= 64 * 1024, (name, lds)
    # seg_local: parents (int32) and class bytes of one 32 x 64 tile
    local, = [n for n in names if "seg_local" in n]
    assert meta[local][2] == 32 * 64 * (4 + 1)
    # seg_tabulate's LDS is dynamic: the histogram [2][24][4][C] u32
    assert 2 * 24 * 4 * 64 * 4 <= 64 * 1024
