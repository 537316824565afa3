"""Register / scratch / LDS budget of the kernels of dasac_crf_meanfield (csrc/crf.hip): no scratch at all, at most 128 VGPRs (four
waves per SIMD) and at most 64 KB of LDS per workgroup -- the static segment from the code object, and the dynamic size the launch
asks for at every halo, class and channel count, restated from the file's own layout.  Reads the code object metadata only.
Cross-compiles to gfx950 assembly; no GPU."""
import os
import shutil

import pytest

from test_kernel_resources import HIPCC, _asm, _kernel_meta

TILE_H, TILE_W, CHUNK, BUDGET = 16, 64, 5, 64 * 1024


def _plane_bytes(halo):
    return (TILE_H + 2 * halo) * (TILE_W + 2 * halo) * 4


def _chunk(C, Ci, halo):
    """Class planes staged at once: what fits beside the image's Ci planes, at most CHUNK, at most C (crf_chunk)."""
    return min(BUDGET // _plane_bytes(halo) - Ci, CHUNK, C)


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.isfile(HIPCC), reason="hipcc not available")
def test_crf_kernels_use_no_scratch_128_vgprs_and_64_kb_of_lds(tmp_path):
    meta = _kernel_meta(_asm(tmp_path, "crf"))
    names = sorted(meta)
    # C = 19 over three image channels (with the default window's halo compiled in, and any halo), the generic C per channel count 1..4
    assert len(names) == 6 and all("crf_iteration" in n for n in names) and sum("ILi19ELi3E" in n for n in names) == 2, names
    for name in names:
        scratch, vgprs, lds = meta[name]
        print("{}: {} VGPRs, {} B scratch, {} B static LDS".format(name, vgprs, scratch, lds))
        assert scratch == 0, (name, scratch)
        assert vgprs <= 128, (name, vgprs)
        assert lds <= BUDGET, (name, lds)


def test_crf_dynamic_lds_fits_64_kb_at_every_halo():
    """Dynamic LDS: (Ci + ck) planes of (16 + 2 r d) x (64 + 2 r d) floats; at the limits r d = 8, C = 32, Ci = 4 two class planes fit."""
    assert _chunk(32, 4, 8) == 2 and (4 + 2) * _plane_bytes(8) == 61440 <= BUDGET
    assert _chunk(19, 3, 5) == 5 and (3 + 5) * _plane_bytes(5) == 61568 <= BUDGET          # the defaults
    for halo in range(1, 9):
        for Ci in range(1, 5):
            for C in (1, 2, 19, 32):
                ck = _chunk(C, Ci, halo)
                assert ck >= 1 and (Ci + ck) * _plane_bytes(halo) <= BUDGET, (halo, Ci, C, ck)
