"""Register / scratch budget of the batched weight-gradient kernel (conv_wgrad_batched of csrc/conv_wgrad.hip), the budget of its
siblings in test_kernel_resources.py: at most 168 VGPRs (3 waves per SIMD), at most 64 bytes of scratch, and no scratch
instruction or SGPR spill (v_readlane / v_writelane) inside a loop that carries MFMAs.  Cross-compiles to gfx950 assembly; no GPU."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _asm, _kernel_meta, _loops

KERNEL = "conv_wgrad_batched"


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.isfile(HIPCC), reason="hipcc not available")
def test_batched_weight_gradient_kernel_fits_its_occupancy_and_keeps_its_mfma_loop_free_of_spills(tmp_path):
    txt = _asm(tmp_path, "conv_wgrad")
    meta = _kernel_meta(txt)
    names = [n for n in meta if KERNEL in n]
    assert len(names) == 1, names
    scratch, vgprs, _ = meta[names[0]]
    print("{}: {} VGPRs, {} B scratch".format(KERNEL, vgprs, scratch))
    assert vgprs <= 168, vgprs
    assert scratch <= 64, scratch
    body = txt[txt.index("\n" + names[0] + ":"):]
    body = body[:body.index("s_endpgm")].split("\n")
    assert sum("v_mfma" in l for l in body) >= 32
    loops = [lp for lp in _loops(body) if lp[1] >= 16]
    assert loops, "the pixel loop is a loop"
    for lbody, _ in loops:
        bad = [l.strip() for l in lbody if "scratch_" in l or "v_readlane" in l or "v_writelane" in l]
        assert not bad, bad[:3]
