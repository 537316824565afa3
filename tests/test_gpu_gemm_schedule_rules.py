"""The host rules of gemm_schedule_ref.py equal the shipped library's, on a grid of shapes and at every reserved-CU setting: the
schedule a shape gets, its split-K tail, the weight gradient's workspace.  No kernel is launched: the four calls are host
arithmetic plus one device query (the persistent schedules need all 256 CUs), so the model that test_gemm_schedule_cpu.py
checks without a GPU is the rule the kernels of test_gpu_conv_schedules_exact.py run by."""
import itertools

import pytest

import conv_lattice as cl
import gemm_schedule_ref as R

pytestmark = pytest.mark.gpu


def shapes():
    """(Nb, OH, OW, M, K): every exact kernel case, then a grid over batch, plane, channels and contraction length that crosses the
    tile sizes, the 64 / 16 K-step thresholds, whole rounds of 1024 tiles and the weight gradient's 200000-pixel branch."""
    out = []
    for c in cl.STREAMK_CASES + [cl.SCHEDULE_CASE, cl.TAIL_CASE] + cl.TAIL_CASES + cl.WGRAD_CASES:
        name, cin, cout, br, stride, (N, H, W) = c
        OH, OW = cl.out_hw(br, stride, H, W)
        out.append((N, OH, OW, cout, cin * sum(b[0] * b[1] for b in br)))
    planes = [(1, 1), (7, 9), (16, 16), (33, 41), (59, 70), (97, 97), (128, 129), (129, 128), (160, 160), (193, 193), (448, 447), (448, 448)]
    Ms = [3, 19, 32, 33, 64, 65, 128, 129, 200, 256, 384, 512, 640, 1024, 1100]
    Ks = [3, 16, 147, 255, 256, 1008, 1024, 1040, 1168, 2304, 4608]
    out += [(Nb, OH, OW, M, K) for (Nb, (OH, OW), M, K) in itertools.product((1, 2, 5, 8), planes, Ms, Ks)]
    return out


def test_the_model_equals_the_library_at_every_reserved_cu_setting():
    from dasac_hip import lib as L
    lib = L.load()
    grid = shapes()
    assert len(grid) > 5000
    counts = {}
    prev = lib.dasac_reserved_cus()
    try:
        for asked in (0, 8, 13, 64, 128):
            lib.dasac_set_reserved_cus(asked)
            reserved = lib.dasac_reserved_cus()
            assert reserved == R.clamp_reserved(asked)
            bad = []
            for Nb, OH, OW, M, K in grid:
                got = (lib.dasac_conv_gemm_schedule(Nb, OH, OW, M, K), lib.dasac_conv_gemm_tail_split(Nb, OH, OW, M, K),
                       lib.dasac_conv_wgrad_workspace(Nb, OH, OW, M, K))
                want = (R.gemm_schedule(Nb, OH, OW, M, K, reserved), R.gemm_tail_split(Nb, OH, OW, M, K, reserved),
                        R.wgrad_workspace(Nb, OH, OW, M, K))
                if got != want:
                    bad.append(((Nb, OH, OW, M, K), got, want))
                counts[(reserved, "stream-K")] = counts.get((reserved, "stream-K"), 0) + want[0]
                counts[(reserved, "tail")] = counts.get((reserved, "tail"), 0) + (want[1] > 0)
                counts[(reserved, "split<8")] = counts.get((reserved, "split<8"), 0) + (0 < want[1] < 8)
            assert not bad, (asked, len(bad), bad[:5])
    finally:
        lib.dasac_set_reserved_cus(prev)
    assert lib.dasac_reserved_cus() == prev
    print("shapes: {}; per reserved setting: {}".format(len(grid), counts))
    assert all(v > 20 for v in counts.values())                    # the grid reaches every answer at every setting
    assert lib.dasac_conv_gemm_workspace() == R.gemm_workspace()
