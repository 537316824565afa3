"""The kernels of the Winograd F(4x4,3x3) forward and data gradient (filter_transform<F4>, the two instantiations of output_transform4
and relu_bits_pack of csrc/winograd.hip) and filter_transform<F2> use no scratch, no LDS and spill nothing: no private segment, no spill count in the code object
metadata, no scratch instruction and no SGPR-spill lane move in their bodies.  The method of test_kernel_resources_winograd4.py:
cross-compiles to gfx950 assembly; no GPU."""
import os
import re
import shutil

import pytest

from test_kernel_resources import HIPCC, _asm, _kernel_meta

# substring of the mangled name (the form is the template argument) -> instantiations
KERNELS = {"filter_transformINS0_2F4E": 1, "output_transform4": 2, "relu_bits_pack": 1, "filter_transformINS0_2F2E": 1}


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.isfile(HIPCC), reason="hipcc not available")
def test_winograd4_conv_kernels_use_no_scratch_no_lds_and_spill_nothing(tmp_path):
    txt = _asm(tmp_path, "winograd")
    meta = _kernel_meta(txt)
    for kernel, count in KERNELS.items():
        names = [n for n in meta if kernel in n]
        assert len(names) == count, (kernel, names)
        for name in names:
            scratch, vgprs, lds = meta[name]
            print("{}: {} VGPRs, {} B scratch, {} B LDS".format(name, vgprs, scratch, lds))
            assert scratch == 0 and lds == 0, (name, scratch, lds)
            assert vgprs <= 128, (name, vgprs)                # four waves per SIMD at the least: the kernels hide latency by occupancy
            (block,) = [b for b in re.split(r"\n\s+- \.agpr_count:", txt.split("amdhsa.kernels:")[1])[1:]     # as _kernel_meta cuts them
                        if re.search(r"\.name:\s+" + re.escape(name) + r"\s", b)]
            for key in ("sgpr_spill_count", "vgpr_spill_count"):
                assert int(re.search(r"\." + key + r":\s+(\d+)", block).group(1)) == 0, (name, key)
            body = txt[txt.index("\n" + name + ":"):]
            body = body[:body.index("s_endpgm")].split("\n")
            bad = [l.strip() for l in body if "scratch_" in l or "v_readlane" in l or "v_writelane" in l]
            assert not bad, (name, bad[:3])
