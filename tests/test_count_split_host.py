"""The blocks-per-image rule of the quad-streaming count kernels (csrc/count_split.hpp) on the host: tools/count_split_check.cpp, a
stand-alone program, prints the split for images from one pixel to 2^33 + 5, batches of 1, 3 and 8 and 256 or 248 usable CUs, with
and without the limit that keeps a block's u32 bins exact, and with a limit of 7 quads so that the limit decides.  Every row must
equal the rule as dasac_mask_counts wrote it out before the header existed (restated here), and the blocks must cover the image
with none left empty.  Built with AddressSanitizer and UBSan (host code only, its own `main`; no GPU, nothing loaded into Python)."""
import os
import subprocess

import pytest

from test_winograd_index_host import ROOT, _compiler

BLOCK, BLOCKS_PER_CU, MIN_QUADS_PER_THREAD = 256, 8, 4
LIMITS = (1 << 29, 0, 7)        # the count kernels' limit, none, and one small enough to decide the split (2^29 never does here)


def _rule(HW, B, cus, max_block_quads):
    n_quads = (HW + 3) >> 2
    bpi = (n_quads + MIN_QUADS_PER_THREAD * BLOCK - 1) // (MIN_QUADS_PER_THREAD * BLOCK)
    fill = (cus * BLOCKS_PER_CU + B - 1) // B
    bpi = min(bpi, fill)
    if max_block_quads:
        bpi = max(bpi, (n_quads + max_block_quads - 1) // max_block_quads)
    return bpi, (n_quads + bpi - 1) // bpi


@pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")
def test_quad_split_is_the_rule_mask_counts_spelled_out_and_covers_every_image(tmp_path):
    exe = tmp_path / "count_split_check"
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "da-sac_amd", "csrc"), os.path.join(ROOT, "tools", "count_split_check.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    rows = {tuple(r[:4]): tuple(r[4:]) for r in (tuple(int(x) for x in line.split()) for line in out.stdout.splitlines())}
    want = [(limit, HW, B, cus) for limit in LIMITS for HW in (1, 3, 63, 4096, 769 * 769, 1024 * 2048, (1 << 33) + 5)
            for B in (1, 3, 8) for cus in (256, 248)]
    assert sorted(rows) == sorted(want)
    for limit, HW, B, cus in want:
        bpi, per = rows[(limit, HW, B, cus)]
        assert (bpi, per) == _rule(HW, B, cus, limit), (limit, HW, B, cus, bpi, per)
        n_quads = (HW + 3) >> 2
        assert bpi * per >= n_quads > (bpi - 1) * per, (limit, HW, B, cus, bpi, per)
        assert not limit or per <= limit, (limit, HW, B, cus, per)
    assert rows[(7, 4096, 1, 256)] == (147, 7) and rows[(0, 4096, 1, 256)] == (1, 1024)      # the limit is obeyed, and only where set
