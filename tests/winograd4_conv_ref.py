"""Forward and data gradient of a dilated 3x3 convolution as Winograd F(4x4,3x3), emulated on the CPU (a helper next to
winograd4_ref.py, whose matrices, points and input-transform row formula it uses; not a conftest): the row formulas that
filter_transform4 and output_transform4 of csrc/winograd.hip spell out (g6 / at4 there), and the whole convolution

    Y = A^T [(G g G^T) (.) (B^T d B)] A          per dilation phase, per 4x4-output tile, summed over the input channels

in the arithmetic of the operands it is given: float32 operands give the kernels' transforms in float32, with the channel sum of the
point products run one channel after the other (the K loop of the point GEMMs is sequential too; only its grouping differs)."""
import numpy as np
import torch

import winograd4_ref as W4


def g6(g0, g1, g2, single=True):
    """G g along one axis.  single: the constants are float32 values, products of float32 constants rounded to float32, as the
    kernel compiles them."""
    r = np.float32 if single else np.float64
    k6, k15, k30 = r(1) / r(6), r(1) / r(15), r(1) / r(30)
    c2, c4, c8, c16 = (float(r(n) * k15) for n in (2, 4, 8, 16))
    k6, k15, k30 = float(k6), float(k15), float(k30)
    return [0.5 * g0,
            k6 * ((g0 + g2) + g1),
            k6 * ((g0 + g2) - g1),
            (k30 * g0 + k15 * g1) + c2 * g2,
            (c16 * g0 - c8 * g1) + c4 * g2,
            0.5 * g2]


def at4(y0, y1, y2, y3, y4, y5):
    """A^T y along one axis."""
    return [(y0 + (y1 + y2)) + (y3 + y4),
            (y1 - y2) + (2.0 * y3 - 0.5 * y4),
            (y1 + y2) + (4.0 * y3 + 0.25 * y4),
            ((y1 - y2) + y5) + (8.0 * y3 - 0.125 * y4)]


def filter_points(w, transposed=False, single=True):
    """w [Cout, Cin, 3, 3] (any scale already folded in) -> U [M, K, 6, 6]; transposed: the filter rotated by 180 degrees with the
    channels swapped, the data gradient's."""
    if transposed:
        w = w.flip(2, 3).transpose(0, 1)
    return W4.both_axes(g6, w.contiguous(), single=single)


def conv(x, w, d, transposed=False, single=True):
    """[N, M, H, W]: the 3x3 convolution of dilation = padding = d of x [N, K, H, W] with w [Cout, Cin, 3, 3] (transposed: the
    data gradient of dz = x), through the F(4x4,3x3) transforms in the dtype of x and w."""
    u = filter_points(w, transposed, single)                       # [M, K, 6, 6]
    N, K, H, W = x.shape
    M = u.shape[0]
    out = torch.zeros(N, M, H, W, dtype=x.dtype)
    for py in range(d):
        for px in range(d):
            xs = x[:, :, py::d, px::d]
            h, wd = xs.shape[-2:]
            if h == 0 or wd == 0:
                continue
            v = W4.both_axes(W4.bt6, W4._tiles(xs, 1, 6))           # [N, K, ty, tx, 6, 6]
            y = torch.zeros((N, M) + tuple(v.shape[2:]), dtype=x.dtype)
            for k in range(K):
                y += v[:, k, None] * u[None, :, k, None, None]
            o = W4.both_axes(at4, y)                               # [N, M, ty, tx, 4, 4]
            ty, tx = o.shape[2:4]
            o = o.permute(0, 1, 2, 4, 3, 5).reshape(N, M, 4 * ty, 4 * tx)
            out[:, :, py::d, px::d] = o[:, :, :h, :wd]
    return out
