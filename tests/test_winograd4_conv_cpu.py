"""Winograd F(4x4,3x3) forward and data gradient on the CPU (no GPU): the identity Y = A^T [(G g G^T) (.) (B^T d B)] A with the matrices
of winograd4_ref.py, the row formulas of winograd4_conv_ref.py (what filter_transform4 / output_transform4 of csrc/winograd.hip spell
out) against those matrices, and the emulated convolution, forward and transposed, against float64 conv2d."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import winograd4_conv_ref as W4C
import winograd4_ref as W4

G, A, BT = W4.f64(W4.G), W4.f64(W4.A), W4.f64(W4.BT)


def test_identity_of_one_tile_with_the_exact_matrices():
    """One 6x6 patch and one 3x3 filter: the 4x4 outputs are the valid correlation, to 1e-12."""
    rng = np.random.default_rng(0)
    d, g = rng.standard_normal((6, 6)), rng.standard_normal((3, 3))
    y = A.T @ ((G @ g @ G.T) * (BT @ d @ BT.T)) @ A
    want = np.array([[(d[i:i + 3, j:j + 3] * g).sum() for j in range(4)] for i in range(4)])
    assert np.abs(y - want).max() <= 1e-12 * max(1.0, np.abs(want).max())


def test_row_formulas_are_the_rows_of_the_matrices():
    rng = np.random.default_rng(1)
    g3, y6 = rng.standard_normal(3), rng.standard_normal(6)
    assert np.abs(np.array(W4C.g6(*g3, single=False)) - G @ g3).max() <= 1e-15
    assert np.abs(np.array(W4C.at4(*y6)) - A.T @ y6).max() <= 1e-14


# (N, Cin, Cout, H, W, dilation): whole tiles, overhang, unequal phases, phases shorter than a tile
SHAPES = [(1, 3, 5, 8, 8, 1), (2, 4, 3, 9, 11, 1), (1, 5, 4, 17, 19, 2), (1, 3, 6, 33, 35, 4), (1, 4, 4, 5, 7, 2)]


@pytest.mark.parametrize("shape", SHAPES, ids=["{}x{}to{}_{}x{}_d{}".format(*s) for s in SHAPES])
def test_emulated_forward_and_data_gradient_against_float64_conv2d(shape):
    N, Cin, Cout, H, W, d = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(N, Cin, H, W, generator=g, dtype=torch.float64)
    dz = torch.randn(N, Cout, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64)
    fwd = F.conv2d(x, w, padding=d, dilation=d)
    dx = F.conv_transpose2d(dz, w, padding=d, dilation=d)
    for got, want in ((W4C.conv(x, w, d, False, single=False), fwd), (W4C.conv(dz, w, d, True, single=False), dx)):
        assert got.shape == want.shape
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def test_float32_emulation_stays_in_float32_and_close():
    N, Cin, Cout, H, W, d = 1, 16, 8, 17, 19, 2
    g = torch.Generator().manual_seed(5)
    x, w = torch.randn(N, Cin, H, W, generator=g), torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    got = W4C.conv(x, w, d)
    assert got.dtype == torch.float32
    want = F.conv2d(x.double(), w.double(), padding=d, dilation=d)
    err = float((got.double() - want).abs().max()) / float(want.abs().max())
    assert 0 < err < 1e-5, err
