"""The three kernels of the Winograd weight gradient (input_transform, grad_transform, wgrad_finish of csrc/winograd.hip), each in
its F(4x4,3x3) and its F(2x2,3x3) instantiation, use no scratch and spill nothing: no private segment, no spill count in the code
object metadata, no scratch instruction and no SGPR-spill lane move in their bodies; wgrad_finish holds the four split lanes' points
and the block's 64 x 9 gradients in LDS, 4*P*64*4 + 64*9*4 + 16 bytes.  The method of test_kernel_resources_wgrad_batched.py:
cross-compiles to gfx950 assembly; no GPU."""
import os
import re
import shutil

import pytest

from test_kernel_resources import HIPCC, _asm, _kernel_meta

# substring of the mangled name (the form is the template argument) -> (VGPR budget, LDS bytes)
KERNELS = {"input_transformINS0_2F4E": (168, 0), "grad_transformINS0_2F4E": (168, 0), "wgrad_finishINS0_2F4E": (168, 39184),   # three waves per SIMD at the least
           "input_transformINS0_2F2E": (128, 0), "grad_transformINS0_2F2E": (128, 0), "wgrad_finishINS0_2F2E": (128, 18704)}   # four


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.isfile(HIPCC), reason="hipcc not available")
def test_winograd4_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    txt = _asm(tmp_path, "winograd")
    meta = _kernel_meta(txt)
    for kernel, (budget, lds_bytes) in KERNELS.items():
        names = [n for n in meta if kernel in n]
        assert len(names) == 1, (kernel, names)
        scratch, vgprs, lds = meta[names[0]]
        print("{}: {} VGPRs, {} B scratch, {} B LDS".format(kernel, vgprs, scratch, lds))
        assert scratch == 0, (kernel, scratch)
        assert vgprs <= budget, (kernel, vgprs)
        assert lds == lds_bytes, (kernel, lds)
        (block,) = [b for b in re.split(r"\n\s+- \.agpr_count:", txt.split("amdhsa.kernels:")[1])[1:]         # as _kernel_meta cuts them
                    if re.search(r"\.name:\s+" + re.escape(names[0]) + r"\s", b)]
        for key in ("sgpr_spill_count", "vgpr_spill_count"):
            assert int(re.search(r"\." + key + r":\s+(\d+)", block).group(1)) == 0, (kernel, key)
        body = txt[txt.index("\n" + names[0] + ":"):]
        body = body[:body.index("s_endpgm")].split("\n")
        bad = [l.strip() for l in body if "scratch_" in l or "v_readlane" in l or "v_writelane" in l]
        assert not bad, (kernel, bad[:3])
