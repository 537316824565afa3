"""Winograd F(4x4,3x3) with the evaluation points 0, 1, -1, 2, -1/2, inf, as csrc/winograd.hip runs the weight gradient (a helper, not
a conftest): the three matrices as exact fractions, the row formulas the kernels spell out (bt6 / a6 / gt3 there), and an emulation of
the whole weight gradient on the CPU in the arithmetic of the operands it is given -- float32 operands give the kernels' transforms
in float32, with the tile sum as the only thing done in another order.

    Y  = A^T [(G g G^T) (.) (B^T d B)] A                     forward: 4x4 outputs of a 6x6 patch d and a 3x3 filter g
    dW = G^T [sum over tiles (A dY A^T) (.) (B^T d B)] G     weight gradient

A is the Vandermonde matrix of the points, B^T the transposed interpolation matrix with its rows scaled to integers, G the
Vandermonde matrix carrying the inverse factors."""
from fractions import Fraction as F

import numpy as np
import torch

POINTS = (F(0), F(1), F(-1), F(2), F(-1, 2), None)          # None: the point at infinity
A = [[F(1), F(0), F(0), F(0)],
     [F(1), F(1), F(1), F(1)],
     [F(1), F(-1), F(1), F(-1)],
     [F(1), F(2), F(4), F(8)],
     [F(1), F(-1, 2), F(1, 4), F(-1, 8)],
     [F(0), F(0), F(0), F(1)]]
BT = [[F(v) for v in row] for row in ([2, 3, -4, -3, 2, 0],
                                      [0, 2, 5, 1, -2, 0],
                                      [0, 2, 1, -5, 2, 0],
                                      [0, -1, -2, 1, 2, 0],
                                      [0, -2, 1, 2, -1, 0],
                                      [0, 2, 3, -4, -3, 2])]
G = [[F(1, 2), F(0), F(0)],
     [F(1, 6), F(1, 6), F(1, 6)],
     [F(1, 6), F(-1, 6), F(1, 6)],
     [F(1, 30), F(1, 15), F(2, 15)],
     [F(16, 15), F(-8, 15), F(4, 15)],
     [F(0), F(0), F(1, 2)]]
SUM_ENTRY = 7               # point (1, 1): the row of A for evaluation point 1 is all ones, so (A dY A^T)[1][1] is the tile's pixel sum


def f64(m):
    return np.array([[float(v) for v in row] for row in m], dtype=np.float64)


# ---- the row formulas of the kernels: each takes the entries along one axis and returns the transformed entries ------------------
def bt6(d0, d1, d2, d3, d4, d5):
    return [(2.0 * (d0 + d4) + 3.0 * (d1 - d3)) - 4.0 * d2,
            (2.0 * (d1 - d4) + 5.0 * d2) + d3,
            (2.0 * (d1 + d4) + d2) - 5.0 * d3,
            (d3 - d1) + 2.0 * (d4 - d2),
            2.0 * (d3 - d1) + (d2 - d4),
            (2.0 * (d1 + d5) + 3.0 * (d2 - d4)) - 4.0 * d3]


def a6(y0, y1, y2, y3):
    return [y0,
            (y0 + y2) + (y1 + y3),
            (y0 + y2) - (y1 + y3),
            (y0 + 4.0 * y2) + (2.0 * y1 + 8.0 * y3),
            (y0 + 0.25 * y2) - (0.5 * y1 + 0.125 * y3),
            y3]


def gt3(p0, p1, p2, p3, p4, p5, single=True):
    """single: the constants are float32 values, products of float32 constants rounded to float32, as the kernel compiles them."""
    r = np.float32 if single else np.float64
    k6, k15, k30 = r(1) / r(6), r(1) / r(15), r(1) / r(30)
    c16, c8, c2, c4 = (float(r(n) * k15) for n in (16, 8, 2, 4))
    k6, k15, k30 = float(k6), float(k15), float(k30)
    return [(0.5 * p0 + k6 * (p1 + p2)) + (k30 * p3 + c16 * p4),
            k6 * (p1 - p2) + (k15 * p3 - c8 * p4),
            (k6 * (p1 + p2) + 0.5 * p5) + (c2 * p3 + c4 * p4)]


def both_axes(fn, t, **kw):
    """fn along the second-to-last axis, then along the last one (the kernels' order: columns first)."""
    t = torch.stack(fn(*t.unbind(-2), **kw), -2)
    return torch.stack(fn(*t.unbind(-1), **kw), -1)


# ---- the weight gradient, emulated ---------------------------------------------------------------------------------------------
def _tiles(img, lead, width):
    """img [N, C, h, w], one dilation phase -> [N, C, ty, tx, width, width]: windows `width` wide, 4 apart, starting `lead` before
    the first sample, zeros outside."""
    h, w = img.shape[-2:]
    ty, tx = -(-h // 4), -(-w // 4)
    pad = torch.zeros(img.shape[:2] + (4 * ty + 2 * lead, 4 * tx + 2 * lead), dtype=img.dtype)
    pad[..., lead:lead + h, lead:lead + w] = img
    return pad.unfold(2, width, 4).unfold(3, width, 4)


def wgrad(x, dz, d, single=True):
    """(unscaled dW [M, C, 3, 3], sum of dz [M]) of the 3x3 convolution of dilation = padding = d, through the F(4x4,3x3) transforms
    in the dtype of x and dz; the sum over tiles runs one tile at a time (phase after phase, image after image)."""
    M, C = dz.shape[1], x.shape[1]
    acc = torch.zeros(M, C, 6, 6, dtype=x.dtype)
    sums = torch.zeros(M, dtype=x.dtype)
    for py in range(d):
        for px in range(d):
            xs, zs = x[:, :, py::d, px::d], dz[:, :, py::d, px::d]
            if xs.shape[-2] == 0 or xs.shape[-1] == 0:
                continue
            v = both_axes(bt6, _tiles(xs, 1, 6))                   # [N, C, ty, tx, 6, 6]
            m = both_axes(a6, _tiles(zs, 0, 4))                    # [N, M, ty, tx, 6, 6]
            v = v.permute(0, 2, 3, 1, 4, 5).reshape(-1, C, 6, 6)
            m = m.permute(0, 2, 3, 1, 4, 5).reshape(-1, M, 6, 6)
            for t in range(v.shape[0]):
                acc += m[t][:, None] * v[t][None]
                sums += m[t][:, 1, 1]
    return both_axes(gt3, acc, single=single), sums
