"""The two launch plans of dasac_ce_loss_bwd_low (csrc/upsample_index.hpp: ce_rows_plan for ce_bwd_rows, ce_wave_plan for
ce_bwd_rows_wave) on the host: tools/ce_bwd_plan_check.cpp, a stand-alone program, walks phases 1 and 2 of both kernels on a real
array of C x pitch floats for every (w, W) with w in 1..130 and W in w..13*w (every W: no thinning was needed) and for the shapes
below, and counts every broken promise: a column outside its segment, a tap outside the segment's x range, an LDS index at or past
the pitch, a wave segment wider than 256 pixels or 64 columns, a column with more taps than SPAN, row chunks that do not cover H.
Built with AddressSanitizer and UBSan (host code only, its own `main`; no GPU, nothing loaded into Python).

The pinned lines are what the launcher computed before the plans existed (its arithmetic restated apart from the header and run
over the same shapes): the header must keep giving them, since a slip there changes the launch geometry -- and the kernel's speed --
without changing one output bit."""
import os
import subprocess

import pytest

from test_winograd_index_host import ROOT, _compiler

# B H w W cus | rows plan: seg_cols n_seg span pitch | wave plan: ok cols n_seg span pitch taps rows n_chunks
LOW_CASES = """\
2 65 13 97 256 | 13 1 100 113 | 1 13 1 100 113 15 4 17
3 33 7 49 256 | 7 1 52 59 | 1 7 1 52 59 15 4 9
1 8 6 12 256 | 6 1 12 14 | 1 6 1 12 14 4 4 2
2 38 6 46 256 | 6 1 48 54 | 1 6 1 48 54 17 4 10
2 50 9 71 256 | 9 1 72 81 | 1 9 1 72 81 18 4 13
1 33 33 35 256 | 33 1 36 41 | 1 33 1 36 41 3 4 9
2 40 30 60 256 | 30 1 60 68 | 1 30 1 60 68 4 4 10
1 65 9 65 256 | 9 1 68 77 | 1 9 1 68 77 15 4 17
1 38 6 46 256 | 6 1 48 54 | 1 6 1 48 54 17 4 10
2 17 5 33 256 | 5 1 36 41 | 1 5 1 36 41 15 4 5
""".splitlines()
# where the wave kernel is refused (W < 4; 31 and 48 taps): the rows plan and the refusal are pinned
REFUSED = ["2 10 4 3 256 | 4 1 4 5 | 0 ", "1 65 5 65 256 | 5 1 68 77 | 0 ", "2 20 2 49 256 | 2 1 52 59 | 0 "]
BIG = """\
1 769 97 769 256 | 35 3 296 333 | 1 25 4 216 243 15 4 193
1 769 97 769 248 | 35 3 296 333 | 1 25 4 216 243 15 4 193
8 769 97 769 256 | 35 3 296 333 | 1 25 4 216 243 15 13 60
8 769 97 769 248 | 35 3 296 333 | 1 25 4 216 243 15 13 60
16 769 97 769 256 | 35 3 296 333 | 1 25 4 216 243 15 25 31
16 769 97 769 248 | 35 3 296 333 | 1 25 4 216 243 15 25 31
1 1025 129 1025 256 | 35 4 296 333 | 1 26 5 224 252 15 4 257
1 1025 129 1025 248 | 35 4 296 333 | 1 26 5 224 252 15 4 257
8 1025 129 1025 256 | 35 4 296 333 | 1 26 5 224 252 15 21 49
8 1025 129 1025 248 | 35 4 296 333 | 1 26 5 224 252 15 21 49
16 1025 129 1025 256 | 35 4 296 333 | 1 26 5 224 252 15 41 25
16 1025 129 1025 248 | 35 4 296 333 | 1 26 5 224 252 15 43 24
1 512 129 1024 256 | 35 4 296 333 | 1 26 5 224 252 16 4 128
1 512 129 1024 248 | 35 4 296 333 | 1 26 5 224 252 16 4 128
8 512 129 1024 256 | 35 4 296 333 | 1 26 5 224 252 16 11 47
8 512 129 1024 248 | 35 4 296 333 | 1 26 5 224 252 16 11 47
16 512 129 1024 256 | 35 4 296 333 | 1 26 5 224 252 16 21 25
16 512 129 1024 248 | 35 4 296 333 | 1 26 5 224 252 16 22 24
""".splitlines()


@pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")
def test_ce_bwd_plans_keep_every_promise_the_kernels_rely_on_and_the_launchers_geometry(tmp_path):
    exe = tmp_path / "ce_bwd_plan_check"
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "da-sac_amd", "csrc"),
                           os.path.join(ROOT, "tools", "ce_bwd_plan_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    lines = out.stdout.splitlines()
    assert lines[-1] == "ce bwd plan check: 102310 (w, W) pairs, 0 bad"      # sum over w = 1..130 of 12 w + 1
    shapes = lines[:-1]
    assert len(shapes) == len(LOW_CASES) + len(REFUSED) + len(BIG)
    for want in LOW_CASES + BIG:
        assert want in shapes, want
    for want in REFUSED:
        assert any(line.startswith(want) for line in shapes), want
    # the workload: 8 crops, 97 -> 769, 256 CUs: 25 columns x 4 segments, 216 pixels, 15 taps (SPAN 16), 13 rows x 60 chunks
    B, n_seg, pitch, n_chunks = 8, 4, 243, 60
    assert "8 769 97 769 256 | 35 3 296 333 | 1 25 4 216 243 15 13 60" in shapes
    assert B * n_chunks * n_seg == 1920 and 19 * pitch * 4 == 18468
