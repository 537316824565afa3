"""Max pooling (csrc/pool.hip) against float64 ATen on the CPU, exactly, through dasac_hip.ops.

Forward: selecting a maximum rounds nothing, so F.max_pool2d(x.double(), ..., return_indices=True) is the reference for y bit for
bit, and its indices for the argmax code: flat = (oh*s - p + code // k) * W + (ow*s - p + code % k).  ATen takes the first maximum
in row-major window order and, with NaNs, the last NaN of the window; the kernels' `v > best || v != v` scan does the same.  The
sign bit is asserted against the reference alone: for k <= 11, arg >> 7 == (y_ref > 0) (0 for negative, zero and NaN pooled
values); for k > 11 bit 7 belongs to the code (code = arg) and the backward reads y.

Inputs: the integers -2..2 as float32 -- every window has ties, many are all-negative or all-zero (drawn uniformly for windows up
to 3 x 3; for larger windows positives are rarer, or no window would be without one: every configuration but the few-window planes
asserts that it has both kinds) -- and, per configuration, one more input with two adjacent NaNs (away from the border wherever the
plane has an interior).  Windows that are all -inf are left
out: there the kernel keeps code 0, which may name a padded position, while ATen names the first in-bounds element; behind a ReLU
it cannot occur.

Backward: dy holds integers in -8..8, so every dx value is a sum of at most 25 small integers, exact in fp32 in any order:
torch.equal with the float64 autograd gradient (relu_mask=False), and with the float64 autograd gradient of dy * (y_ref > 0)
(relu_mask=True: a window contributes iff its pooled value is positive).  One random-float dy per configuration is held to
tests/fp64_yardstick.py's rule (fp32 autograd as the yardstick), so that a routing that merely preserves integers is not all that
is tested.

Which configuration reaches which kernel (`_fwd_kernel` / `_bwd_kernel` restate the two launchers, and the test asserts it):
  maxpool_fwd_quad<3,2> + maxpool_bwd_3s2p1   (3,2,1,*): 33x41 ceil (odd H: the 2 x 4 block's second row is missing; OW = 21: a
                                              one-output tail, ow0 + 2 >= OW: the non-wide loads), 7x5, 10x9 floor, 1x1, 2x38
  maxpool_fwd_quad<3,2> + maxpool_bwd<3,2>    (3,2,0,*): 12x14 ceil, 9x11 floor, 3x3 (one window)
  maxpool_fwd_quad<2,2> + maxpool_bwd<2,2>    (2,2,*,*): 16x24, 9x11 floor and ceil, pad 1 at 8x10, 2x2
  maxpool_fwd<3,1> + maxpool_bwd<3,1>         (3,1,1) 12x13, (3,1,0) 5x6
  maxpool_fwd<0,0> + maxpool_bwd<0,0>         (5,3,2) ceil, (4,4,0), (7,1,3); k > 11: (13,4,6) ceil and (15,15,0)
Second pass of the capped grid (stream_grid's default cap x 256 threads, restated): 6 planes of 349527 x 2 for the stem-pool pair
and 6 planes of 174764 x 3 for the <3,1> pair; a narrow plane makes every quad a tail, so the item count is planes x rows.

Measured on the MI355X: every exact condition holds; random-float dy, worst err_hip / (2 * err_aten + 1e-6):
  0.11 on the second pass of the <3,1> pair, at most 0.064 on the small configurations, for relu_mask on and off alike; exactly 0
  where no two windows overlap (2x2/2, 4x4/4, 15x15/15: a dx value is one dy value)
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from fp64_yardstick import _ratio, _report

pytestmark = pytest.mark.gpu
K_NUM_CU = 256              # common.hpp kNumCu
SIGN_MAX_K = 11             # pool.hip kPoolSignMaxK


def _fwd_kernel(k, s):
    """dasac_maxpool_fwd's dispatch (pool.hip)"""
    return {(3, 2): "fwd_quad<3,2>", (2, 2): "fwd_quad<2,2>", (3, 1): "fwd<3,1>"}.get((k, s), "fwd<0,0>")


def _bwd_kernel(k, s, p):
    """dasac_maxpool_bwd's dispatch (pool.hip)"""
    if (k, s, p) == (3, 2, 1):
        return "bwd_3s2p1"
    return {(3, 2): "bwd<3,2>", (2, 2): "bwd<2,2>", (3, 1): "bwd<3,1>"}.get((k, s), "bwd<0,0>")


def _default_cap():
    """stream_grid's default max_blocks (common.hpp): (kNumCu - reserved_cus()) * 16"""
    from dasac_hip import lib as L
    return (K_NUM_CU - L.load().dasac_reserved_cus()) * 16


# (k, s, p, ceil_mode, H, W), forward kernel, backward kernel
CONFIGS = [
    ((3, 2, 1, True, 33, 41), "fwd_quad<3,2>", "bwd_3s2p1"),
    ((3, 2, 1, True, 7, 5), "fwd_quad<3,2>", "bwd_3s2p1"),
    ((3, 2, 1, False, 10, 9), "fwd_quad<3,2>", "bwd_3s2p1"),
    ((3, 2, 1, True, 1, 1), "fwd_quad<3,2>", "bwd_3s2p1"),
    ((3, 2, 1, False, 2, 38), "fwd_quad<3,2>", "bwd_3s2p1"),
    ((3, 2, 0, True, 12, 14), "fwd_quad<3,2>", "bwd<3,2>"),
    ((3, 2, 0, False, 9, 11), "fwd_quad<3,2>", "bwd<3,2>"),
    ((3, 2, 0, True, 3, 3), "fwd_quad<3,2>", "bwd<3,2>"),
    ((2, 2, 0, False, 16, 24), "fwd_quad<2,2>", "bwd<2,2>"),
    ((2, 2, 0, False, 9, 11), "fwd_quad<2,2>", "bwd<2,2>"),
    ((2, 2, 0, True, 9, 11), "fwd_quad<2,2>", "bwd<2,2>"),
    ((2, 2, 1, False, 8, 10), "fwd_quad<2,2>", "bwd<2,2>"),
    ((2, 2, 0, False, 2, 2), "fwd_quad<2,2>", "bwd<2,2>"),
    ((3, 1, 1, False, 12, 13), "fwd<3,1>", "bwd<3,1>"),
    ((3, 1, 0, False, 5, 6), "fwd<3,1>", "bwd<3,1>"),
    ((5, 3, 2, True, 21, 23), "fwd<0,0>", "bwd<0,0>"),
    ((4, 4, 0, False, 16, 16), "fwd<0,0>", "bwd<0,0>"),
    ((7, 1, 3, False, 9, 10), "fwd<0,0>", "bwd<0,0>"),
    ((13, 4, 6, True, 30, 41), "fwd<0,0>", "bwd<0,0>"),       # k > 11: the sign bit stays out of the byte
    ((15, 15, 0, False, 30, 45), "fwd<0,0>", "bwd<0,0>"),
]
# (k, s, p, ceil_mode, planes, H, W): the smallest narrow planes whose item counts exceed the default grid cap x 256
SECOND_PASS = [
    (3, 2, 1, True, 6, 349527, 2),       # fwd_quad<3,2>: 6 x 174764 x 1 quads; bwd_3s2p1: 6 x 174764 x 1 blocks of 2 x 4
    (3, 1, 1, False, 6, 174764, 3),      # fwd<3,1>: 6 x 174764 x 3 outputs; bwd<3,1>: 6 x 174764 x 1 quads
]


def _id(cfg):
    k, s, p, ceil, H, W = cfg
    return "k{}s{}p{}{}_{}x{}".format(k, s, p, "c" if ceil else "f", H, W)


def test_the_configurations_reach_every_kernel_of_both_launchers():
    for (k, s, p, ceil, H, W), fwd, bwd in CONFIGS:
        assert _fwd_kernel(k, s) == fwd and _bwd_kernel(k, s, p) == bwd, (k, s, p)
    assert {c[1] for c in CONFIGS} == {"fwd_quad<3,2>", "fwd_quad<2,2>", "fwd<3,1>", "fwd<0,0>"}
    assert {c[2] for c in CONFIGS} == {"bwd_3s2p1", "bwd<3,2>", "bwd<2,2>", "bwd<3,1>", "bwd<0,0>"}
    assert any(c[0][0] > SIGN_MAX_K for c in CONFIGS)
    from dasac_hip import ops
    # (3,2,1,ceil,33,41): OH = 17 windows over 33 rows (row 2p + 1 = 33 is missing for p = 16), OW = 21: the last quad of a row
    # starts at ow0 = 20, so ow0 + 2 >= OW
    assert ops.pool_out(33, 3, 2, 1, True) == 17 and ops.pool_out(41, 3, 2, 1, True) == 21


def _integers(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


def _lattice(shape, k, seed):
    """integers -2..2 as float32: uniform for windows up to 3 x 3; for larger windows positives are made rare enough (about half
    of the full windows hold none) that the sign bit, or the backward's read of y for k > 11, still decides something"""
    if k <= 3:
        return _integers(shape, -2, 2, seed)
    g = torch.Generator().manual_seed(seed)
    positive = torch.rand(shape, generator=g) < 1.0 - 0.5 ** (1.0 / (k * k))
    return torch.where(positive, torch.randint(1, 3, shape, generator=g), torch.randint(-2, 1, shape, generator=g)).float()


def _with_nans(x):
    """two horizontally adjacent NaNs in plane (0, 0), off the border wherever the plane has an interior"""
    x = x.clone()
    H, W = x.shape[2:]
    r, c = H // 2, max(0, W // 2 - 1)
    x[0, 0, r, c] = float("nan")
    x[0, 0, r, min(c + 1, W - 1)] = float("nan")
    if H >= 3 and W >= 4:
        assert 0 < r < H - 1 and 0 < c and c + 1 < W - 1
    return x


def _check_forward(x, k, s, p, ceil):
    """y bit for bit, the argmax code against ATen's indices, the sign bit against the reference; returns (y, arg, y_ref)"""
    from dasac_hip import ops
    H, W = x.shape[2:]
    y64, idx = F.max_pool2d(x.double(), k, s, p, ceil_mode=ceil, return_indices=True)
    y, arg = ops.maxpool_fwd(x.cuda(), k, s, p, ceil)
    assert y.shape == y64.shape and arg.shape == y64.shape and arg.dtype == torch.uint8
    assert torch.allclose(y.cpu().double(), y64, rtol=0.0, atol=0.0, equal_nan=True)
    a = arg.cpu().long()
    code = (a & 0x7f) if k <= SIGN_MAX_K else a
    oh = torch.arange(y64.shape[2]).view(1, 1, -1, 1)
    ow = torch.arange(y64.shape[3]).view(1, 1, 1, -1)
    flat = (oh * s - p + code // k) * W + (ow * s - p + code % k)
    assert torch.equal(flat, idx)
    if k <= SIGN_MAX_K:
        assert torch.equal((a >> 7).bool(), y64 > 0)
    return y, arg, y64


def _bwd_reference(x, dy, k, s, p, ceil, relu_mask, dtype):
    x = x.to(dtype).requires_grad_(True)
    y = F.max_pool2d(x, k, s, p, ceil_mode=ceil)
    g = dy.to(dtype)
    if relu_mask:
        g = g * (y.detach() > 0)
    (dx,) = torch.autograd.grad(y, x, g)
    return dx


def _check_backward(what, x, y, arg, k, s, p, ceil, seed):
    from dasac_hip import ops
    H, W = x.shape[2:]
    dy_int = _integers(tuple(y.shape), -8, 8, seed)
    dy_float = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed + 1))
    ratios = {}
    for relu_mask in (False, True):
        dx = ops.maxpool_bwd(dy_int.cuda(), y, arg, (H, W), k, s, p, relu_mask=relu_mask)
        assert torch.equal(dx.cpu().double(), _bwd_reference(x, dy_int, k, s, p, ceil, relu_mask, torch.float64)), (what, relu_mask)
        dx = ops.maxpool_bwd(dy_float.cuda(), y, arg, (H, W), k, s, p, relu_mask=relu_mask)
        ratios["relu_mask {}".format(int(relu_mask))] = _ratio(dx, _bwd_reference(x, dy_float, k, s, p, ceil, relu_mask, torch.float64),
                                                               _bwd_reference(x, dy_float, k, s, p, ceil, relu_mask, torch.float32))
    _report("maxpool_bwd", what, ratios)


@pytest.mark.parametrize("config", CONFIGS, ids=[_id(c[0]) for c in CONFIGS])
def test_maxpool_forward_and_backward_are_exact(config):
    (k, s, p, ceil, H, W), _, _ = config
    x = _lattice((2, 3, H, W), k, seed=k + s + p + H + W)
    y, arg, y64 = _check_forward(x, k, s, p, ceil)
    share = float((y64 <= 0).float().mean())
    print("maxpool {}: {:.3g} of the pooled values are not positive".format(_id(config[0]), share))
    assert 0.0 < share < 1.0 or y64.numel() <= 12, config                 # both kinds of window, but on the smallest planes
    _check_backward(_id(config[0]), x, y, arg, k, s, p, ceil, seed=H + W)
    _check_forward(_with_nans(x), k, s, p, ceil)


def test_the_lattice_has_ties_and_windows_without_a_positive_value():
    """what the -2..2 lattice is for, on the reference alone: at 2x2 windows a good share of the pooled values is negative or zero"""
    x = _integers((2, 3, 16, 24), -2, 2, seed=2 + 2 + 0 + 16 + 24)
    y = F.max_pool2d(x.double(), 2, 2, 0)
    assert float((y < 0).float().mean()) > 0.01 and float((y == 0).float().mean()) > 0.05 and float((y > 0).float().mean()) > 0.3


@pytest.mark.parametrize("case", SECOND_PASS, ids=["k{}s{}_{}x{}x{}".format(c[0], c[1], c[4], c[5], c[6]) for c in SECOND_PASS])
def test_maxpool_second_pass_of_the_capped_grid(case):
    from dasac_hip import ops
    k, s, p, ceil, planes, H, W = case
    OH, OW = ops.pool_out(H, k, s, p, ceil), ops.pool_out(W, k, s, p, ceil)
    threads = _default_cap() * 256
    # the item counts of the two launchers (pool.hip: items4 / total in dasac_maxpool_fwd, items2 / items in dasac_maxpool_bwd)
    fwd_items = planes * OH * ((OW + 3) // 4) if _fwd_kernel(k, s).startswith("fwd_quad") else planes * OH * OW
    bwd_items = planes * ((H + 1) // 2) * ((W + 3) // 4) if _bwd_kernel(k, s, p) == "bwd_3s2p1" else planes * H * ((W + 3) // 4)
    assert fwd_items > threads and bwd_items > threads and planes * H * W < 20e6
    x = _integers((1, planes, H, W), -2, 2, seed=H)
    y, arg, _ = _check_forward(x, k, s, p, ceil)
    _check_backward(case, x, y, arg, k, s, p, ceil, seed=W)


def test_maxpool_refusals():
    from dasac_hip import ops
    from dasac_hip import lib as L
    with pytest.raises(L.DasacError, match="bad arguments"):
        ops.maxpool_fwd(torch.zeros(1, 1, 20, 20).cuda(), 16, 1, 0, False)              # k = 16: the code would not fit the byte
    lib = L.load()
    buf = (ctypes.c_float * 4)()
    at = ctypes.addressof(buf)                                                          # never dereferenced: refused on the host
    #                            x   planes    H        W        OH       OW      k  s  p  y   arg
    assert lib.dasac_maxpool_fwd(at, 1 << 11, 1 << 10, 1 << 10, 1 << 10, 1 << 10, 3, 1, 1, at, at, None) != 0
    assert b"too large" in lib.dasac_last_error()
    assert not any(buf)
