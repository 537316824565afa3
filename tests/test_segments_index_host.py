"""Index arithmetic of the connected-component kernels (csrc/segments_index.hpp) on the host: tools/segments_index_check.cpp, a
stand-alone program, prints for image sizes around the tile edges, for every border pixel and both connectivities, the neighbour
indices the merge kernel would visit.  Checked here against a restatement in Python: nothing outside the image, nothing across a
row wrap, and every adjacent pair of pixels that lie in different tiles visited at least once; also the bin rule and the tile <->
image index map.  Built with AddressSanitizer and UBSan (host code only, its own `main`; no GPU, nothing loaded into Python)."""
import os
import subprocess

import pytest

from test_winograd_index_host import ROOT, _compiler


def _adjacent_pairs_across_tiles(H, W, TH, TW, connectivity):
    """{(smaller index, larger index)} of all adjacent pixel pairs whose pixels lie in different tiles."""
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    pairs = set()
    for y in range(H):
        for x in range(W):
            for dy, dx in steps:
                v, u = y + dy, x + dx
                if 0 <= v < H and 0 <= u < W and (y // TH, x // TW) != (v // TH, u // TW):
                    pairs.add((y * W + x, v * W + u))
    return pairs


@pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")
def test_the_merge_kernel_visits_every_pair_across_a_tile_seam_and_nothing_outside_the_image(tmp_path):
    exe = tmp_path / "segments_index_check"
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "da-sac_amd", "csrc"), os.path.join(ROOT, "tools", "segments_index_check.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    lines = [line.split() for line in out.stdout.splitlines()]
    assert lines[-1] == "segments index check: done".split()
    (TH, TW, bins), = [tuple(int(v) for v in l[1:]) for l in lines if l[0] == "T"]
    assert bins == 24

    # the bin rule: min(floor(log2(size)), 23)
    got_bins = {int(l[1]): int(l[2]) for l in lines if l[0] == "B"}
    assert {2 ** k for k in range(31)} <= set(got_bins) and {1, 2, 3, 2 ** 23 - 1, 2 ** 23, 2 ** 31 - 1} <= set(got_bins)
    for size, b in got_bins.items():
        assert b == min(size.bit_length() - 1, bins - 1), (size, b)

    shapes = {}
    for l in lines:
        if l[0] == "L":
            H, W, tiles_y, tiles_x, once = (int(v) for v in l[1:])
            assert (tiles_y, tiles_x, once) == (-(-H // TH), -(-W // TW), 1), l
            shapes[(H, W)] = {4: [], 8: []}
    want_shapes = {(1, 1), (1, 7), (7, 1), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH, 2 * TW), (2 * TH + 3, 2 * TW + 5),
                   (TH + 1, 3), (3, TW + 1), (3 * TH + 1, 1), (1, 3 * TW + 1)}
    assert set(shapes) == want_shapes
    for l in lines:
        if l[0] == "P":
            H, W, conn, item, y, x, vertical, n = (int(v) for v in l[1:9])
            assert len(l) == 9 + n and 1 <= n <= (3 if conn == 8 else 1), l
            shapes[(H, W)][conn].append((item, y, x, vertical, [int(v) for v in l[9:]]))

    for (H, W), by_conn in shapes.items():
        for conn, rows in by_conn.items():
            want_items = (-(-H // TH) - 1) * W + (-(-W // TW) - 1) * H
            assert [r[0] for r in rows] == list(range(want_items)), (H, W, conn)
            visited = set()
            for item, y, x, vertical, nbs in rows:
                assert 0 <= y < H and 0 <= x < W
                assert (x % TW == 0 and x > 0) if vertical else (y % TH == 0 and y > 0), (H, W, item, y, x, vertical)
                for nb in nbs:
                    assert 0 <= nb < H * W, (H, W, conn, y, x, nb)                      # inside the image
                    v, u = divmod(nb, W)
                    assert max(abs(v - y), abs(u - x)) == 1, (H, W, conn, y, x, nb)     # adjacent in 2-D: never across a row end
                    assert conn == 8 or abs(v - y) + abs(u - x) == 1
                    assert (v // TH, u // TW) != (y // TH, x // TW)                     # only pairs the tile pass could not see
                    visited.add((min(nb, y * W + x), max(nb, y * W + x)))
                assert len(set(nbs)) == len(nbs)
            assert visited == _adjacent_pairs_across_tiles(H, W, TH, TW, conn), (H, W, conn)
    assert not shapes[(TH, TW)][8] and not shapes[(1, 7)][4] and len(shapes[(TH + 1, TW + 1)][8]) == (TW + 1) + (TH + 1)
