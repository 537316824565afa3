"""Winograd F(4x4,3x3) on the host: the three matrices of tests/winograd4_ref.py (points 0, 1, -1, 2, -1/2, inf) satisfy the forward
and the weight-gradient identity in float64, the row formulas the kernels spell out are those matrices, and the index arithmetic of
the four-output tiling (csrc/winograd_index.hpp with TM = 4) keeps every offset of input_transform4 / grad_transform4 inside its
tensor: tools/winograd_index_check.cpp, dilations 1, 2, 4, extents including 5, 8, 17, 33, 97.  No GPU."""
import os
import subprocess

import numpy as np
import pytest
import torch

import winograd4_ref as W4
from test_winograd_index_host import ROOT, _compiler

A, BT, G = W4.f64(W4.A), W4.f64(W4.BT), W4.f64(W4.G)


def _correlate(d, g):
    """4x4 outputs of a 6x6 patch and a 3x3 filter"""
    return np.array([[(d[i:i + 3, j:j + 3] * g).sum() for j in range(4)] for i in range(4)])


def test_forward_identity_in_float64():
    rng = np.random.default_rng(0)
    for _ in range(20):
        d, g = rng.standard_normal((6, 6)), rng.standard_normal((3, 3))
        y = A.T @ ((G @ g @ G.T) * (BT @ d @ BT.T)) @ A
        assert np.abs(y - _correlate(d, g)).max() <= 1e-12


def test_weight_gradient_identity_in_float64():
    rng = np.random.default_rng(1)
    tiles = 7
    d, dy = rng.standard_normal((tiles, 6, 6)), rng.standard_normal((tiles, 4, 4))
    acc = sum((A @ dy[t] @ A.T) * (BT @ d[t] @ BT.T) for t in range(tiles))
    dw = G.T @ acc @ G
    ref = np.array([[sum((dy[t] * d[t, a:a + 4, b:b + 4]).sum() for t in range(tiles)) for b in range(3)] for a in range(3)])
    assert np.abs(dw - ref).max() <= 1e-12


def test_row_formulas_are_the_matrices():
    """bt6 / a6 / gt3 (what the kernels compute, term by term) against B^T, A and G^T in float64; the point whose row of A is all
    ones is evaluation point 1, entry (1, 1) = SUM_ENTRY of the 6x6 points."""
    g = torch.Generator().manual_seed(2)
    for fn, mat, n in ((W4.bt6, BT, 6), (W4.a6, A, 4), (lambda *p: W4.gt3(*p, single=False), G.T, 6)):
        v = torch.randn(n, 5, generator=g, dtype=torch.float64)
        got = torch.stack(fn(*v.unbind(0)), 0).numpy()
        assert np.abs(got - mat @ v.numpy()).max() <= 1e-12
    assert all(v == 1 for v in W4.A[1]) and W4.POINTS[1] == 1 and W4.SUM_ENTRY == 1 * 6 + 1


@pytest.mark.parametrize("shape", [(2, 3, 5, 9, 11, 1), (1, 4, 3, 17, 19, 2), (1, 2, 3, 5, 7, 2), (1, 3, 2, 13, 9, 4)], ids=lambda s: "x".join(map(str, s)))
def test_emulated_weight_gradient_equals_aten_in_float64(shape):
    """The emulation the GPU test measures against, run in float64: the weight gradient and the channel sums of dz, overhanging
    tiles, unequal phases and phases shorter than one tile included."""
    N, C, M, H, W, d = shape
    g = torch.Generator().manual_seed(sum(shape))
    x, dz = torch.randn(N, C, H, W, generator=g, dtype=torch.float64), torch.randn(N, M, H, W, generator=g, dtype=torch.float64)
    dw, sums = W4.wgrad(x, dz, d, single=False)
    ref = torch.nn.grad.conv2d_weight(x, (M, C, 3, 3), dz, padding=d, dilation=d)
    assert float((dw - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max()))
    assert float((sums - dz.sum((0, 2, 3))).abs().max()) <= 1e-12 * H * W


@pytest.mark.skipif(_compiler() is None, reason="no host C++ compiler")
def test_index_check_reports_no_bad_offset_for_four_output_tiles(tmp_path):
    exe = tmp_path / "winograd_index_check"
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "da-sac_amd", "csrc"), os.path.join(ROOT, "tools", "winograd_index_check.cpp"),
                           "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    assert "winograd index check, m = 4: 0 bad" in out.stdout
    assert "m=4 N=8 C=256 M=256 97x97 d=2: 25 x 25 tiles per image, T=5000 (0 padding)" in out.stdout
    assert "m=4 N=1 C=512 M=512 97x97 d=4: 25 x 25 tiles per image, T=628 (3 padding)" in out.stdout
    assert "m=4 N=1 C=256 M=256 17x17 d=2: 5 x 5 tiles per image, T=28 (3 padding)" in out.stdout
