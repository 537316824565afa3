"""The element-wise kernels of csrc/pointwise.hip (scale_planes, add2, relu_mask) bit for bit against their one-line torch
expressions on the CPU, and class_state (csrc/class_prior.hip) against float64 restatements of sac.py:104-117, 120, 151-152, through
dasac_hip.ops.

scale_planes = x * m[:, :, None, None] (Dropout2d), add = a + b (skip joins; with and without out=, and with out aliasing a as
the engine's upsample-and-add layer calls it), relu_mask = torch.where(y > 0, dy, 0) (the ReLU backward).  One IEEE operation or
a select per element: every finite, infinite and zero result must carry the CPU's bits, -0.0 included; NaNs must sit at the same
positions (IEEE leaves the payload of a NaN an operation produces to the hardware, so payloads are not compared).  Sizes 1, 255,
257, a [2,5,7,9] tensor and one above stream_grid's default cap x 256 threads (the grid-stride loop's second trip).  Inputs carry
-0.0, NaN and +-inf; relu_mask gives 0 for y = 0.0, -0.0 and NaN.

class_state: four successive calls (the third with update=False: chi keeps its bits) for C = 1, 19, 32 and focal_p = 1, 2, 3
(products) and 2.5 (powf).  chi, disc and focal follow tests/fp64_yardstick.py's rule with the oracle's fp32 update_running_conf /
threshold_discount / focal_weight as the yardstick.  The initialisation branch (sac.py:111-113) is taken both ways in the first
call: classes whose chi equals beta and whose batch mean is above the tolerance 1e-8 adopt the mean; classes with a mean below it
do not; classes whose chi is one ulp above or below beta do not.  The comparison with beta is the reference's fp32 one (chi is an
fp32 tensor; beta reaches the comparison rounded to fp32); no mean lies within 1e-6 relative of the tolerance (asserted on the
float64 reference).

Measured on the MI355X: every bit-exact condition holds; class_state, worst err_hip / (2 * err_aten + 1e-6):
  chi 0.047, disc 0.16, focal 0.13 (focal_p = 3; 0.094 through powf at 2.5) -- the 1e-6 floor is most of the bound
"""
import numpy as np
import pytest
import torch

from fp64_yardstick import _ratio, _report

pytestmark = pytest.mark.gpu
K_NUM_CU = 256              # common.hpp kNumCu
NAN, INF = float("nan"), float("inf")


def _default_cap():
    """stream_grid's default max_blocks (common.hpp): (kNumCu - reserved_cus()) * 16"""
    from dasac_hip import lib as L
    return (K_NUM_CU - L.load().dasac_reserved_cus()) * 16


def _same_bits(got, ref):
    got, ref = got.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    if got.shape != ref.shape or got.dtype != torch.float32 or ref.dtype != torch.float32:
        return False
    nan = torch.isnan(ref)
    return torch.equal(torch.isnan(got), nan) and torch.equal(got.view(torch.int32)[~nan], ref.view(torch.int32)[~nan])


def _plant(t, values):
    """the special values at the head of the flattened tensor, as many as fit"""
    flat = t.view(-1)
    n = min(len(values), flat.numel())
    flat[:n] = torch.tensor(values[:n])
    return t


def _flat_sizes():
    big = _default_cap() * 256 + 257
    return [(1,), (255,), (257,), (2, 5, 7, 9), (big,)]


def test_the_large_size_makes_a_thread_loop():
    assert _flat_sizes()[-1][0] > _default_cap() * 256 and 2 * 3 * 419 * 419 > _default_cap() * 256


# (dy, y): -0.0, NaN and +-inf pass where y > 0 and are dropped where it is not; y = 0.0, -0.0 and NaN give 0
RELU_PAIRS = [(-0.0, 1.0), (NAN, 1.0), (INF, 2.0), (NAN, -1.0), (INF, 0.0), (1.5, 0.0), (1.5, -0.0), (-INF, 1e-30), (2.0, NAN),
              (-0.0, -1.0), (3.0, 1e-45), (3.0, -1e-45)]


def test_relu_mask_is_a_select_bit_for_bit():
    from dasac_hip import ops
    for i, shape in enumerate(_flat_sizes()):
        g = torch.Generator().manual_seed(i)
        dy = _plant(torch.randn(shape, generator=g), [p[0] for p in RELU_PAIRS])
        y = _plant(torch.randn(shape, generator=g), [p[1] for p in RELU_PAIRS])
        if len(shape) == 1 and shape[0] == 1:
            dy, y = torch.tensor([1.5]), torch.tensor([-0.0])
        ref = torch.where(y > 0, dy, torch.zeros(()))
        got = ops.relu_mask(dy.cuda(), y.cuda())
        assert _same_bits(got, ref), shape
        zero = (y == 0) | torch.isnan(y)
        assert bool((got.cpu()[zero].view(torch.int32) == 0).all())                  # +0.0, not -0.0, not NaN
    # a select moves bits: the NaN's payload and sign survive
    odd = torch.tensor([0x7fc12345, -0x3fedcb], dtype=torch.int32).view(torch.float32)      # a positive and a negative quiet NaN
    assert bool(torch.isnan(odd).all())
    got = ops.relu_mask(odd.cuda(), torch.ones(2).cuda())
    assert torch.equal(got.cpu().view(torch.int32), odd.view(torch.int32))


ADD_PAIRS = [(-0.0, -0.0), (-0.0, 0.0), (NAN, 1.0), (1.0, NAN), (INF, 1.0), (INF, -INF), (3e38, 3e38), (-3e38, -3e38), (1.0, 2.0 ** -24),
             (1.0, 2.0 ** -24 + 2.0 ** -40), (1e-45, 1e-45), (1e-38, -1.1e-38)]


def test_add_with_and_without_out_and_in_place():
    from dasac_hip import ops
    for i, shape in enumerate(_flat_sizes()):
        g = torch.Generator().manual_seed(10 + i)
        a = _plant(torch.randn(shape, generator=g), [p[0] for p in ADD_PAIRS])
        b = _plant(torch.randn(shape, generator=g), [p[1] for p in ADD_PAIRS])
        ref = a + b
        ad, bd = a.cuda(), b.cuda()
        assert _same_bits(ops.add(ad, bd), ref), shape
        out = torch.full(shape, 7.0).cuda()
        assert ops.add(ad, bd, out=out) is out and _same_bits(out, ref), shape
        assert _same_bits(ad, a) and _same_bits(bd, b)                               # the operands are untouched
        alias = a.clone().cuda()
        assert ops.add(alias, bd, out=alias) is alias and _same_bits(alias, ref), shape


def test_scale_planes_is_one_multiply_per_element():
    from dasac_hip import ops
    shapes = [(1, 1, 1, 1), (1, 1, 1, 255), (257, 1, 1, 1), (2, 5, 7, 9), (2, 3, 419, 419)]
    specials = [-0.0, NAN, INF, -INF, 1e-45, 3e38, 0.0, -1e-38]
    for i, shape in enumerate(shapes):
        g = torch.Generator().manual_seed(20 + i)
        x = _plant(torch.randn(shape, generator=g), specials)
        # Dropout2d's keep / (1 - p): planes of 0 and of 2, and one negative and one -0.0 factor where there is room
        m = torch.where(torch.rand(shape[:2], generator=g) < 0.3, torch.zeros(()), torch.full((), 2.0))
        m.view(-1)[0] = 2.0                                                          # the plane with the special values is kept
        if m.numel() >= 4:
            m.view(-1)[1], m.view(-1)[2], m.view(-1)[3] = 0.0, -1.5, -0.0
        ref = x * m[:, :, None, None]
        assert _same_bits(ops.scale_planes(x.cuda(), m.cuda()), ref), shape


# ---- class_state ---------------------------------------------------------------------------------------------------------------
BETA, MOMENTUM, TOL = 1e-3, 0.99, 1e-8        # cfg.THRESHOLD_BETA, cfg.STAT_MOMENTUM, _update_running_conf's tolerance


def _state_step64(chi, avg, update):
    """sac.py:104-117 in float64; the equality with beta is the reference's fp32 comparison (module docstring)"""
    if update:
        fresh = (avg > TOL) & (chi == float(np.float32(BETA)))
        chi = torch.where(fresh, avg, chi)
        chi = chi * MOMENTUM + (1 - MOMENTUM) * avg
    return chi


def _vectors64(chi, p):
    """sac.py:151-152 and sac.py:120 in float64"""
    return 1.0 - torch.exp(-chi / BETA), (1 - chi.clamp(0.0)) ** p


@pytest.mark.parametrize("focal_p", [1.0, 2.0, 3.0, 2.5])
@pytest.mark.parametrize("C", [1, 19, 32])
def test_class_state_against_fp64(C, focal_p):
    from dasac_hip import ops
    from oracle import head_ref
    B, Hh, W = 2, 5, 7
    g = torch.Generator().manual_seed(C)
    beta32 = torch.tensor(BETA)
    role = torch.arange(C) % 4               # 0: at beta, mean above the tolerance; 1: at beta, mean below; 2 / 3: one ulp off beta
    chi32 = torch.full((C,), BETA)
    chi32[role == 2] = torch.nextafter(beta32, torch.tensor(1.0))
    chi32[role == 3] = torch.nextafter(beta32, torch.tensor(0.0))
    assert bool((chi32[role >= 2] != beta32).all()) and bool((chi32[role < 2] == BETA).all())
    chi64, chi_dev = chi32.double(), chi32.clone().cuda()
    for it, update in enumerate((True, True, False, True)):
        scale = torch.rand(C, generator=g) * 0.8 + 0.1
        scale[role == 1] = 2e-10
        probs = torch.rand(B, C, Hh, W, generator=g) * scale.view(1, C, 1, 1)
        avg64 = probs.double().mean(0).view(C, -1).mean(-1)
        assert bool(((avg64 / TOL - 1).abs() > 1e-6).all())
        assert bool((avg64[role == 1] < TOL).all()) and bool((avg64[role != 1] > TOL).all())
        if it == 0:                          # the branch of sac.py:111-113, both ways, on the reference
            fresh = (avg64 > TOL) & (chi64 == float(np.float32(BETA)))
            assert torch.equal(fresh, role == 0)
        chi64 = _state_step64(chi64, avg64, update)
        if update:
            chi32 = head_ref.update_running_conf(chi32, probs, BETA, MOMENTUM)
        before = chi_dev.clone()
        sums = probs.double().sum((0, 2, 3)).cuda()
        disc, focal = ops.class_state(chi_dev, sums, B, Hh * W, BETA, MOMENTUM, update, focal_p)
        if not update:
            assert torch.equal(before.view(torch.int32), chi_dev.view(torch.int32))
        elif it == 0 and C > 1:
            # adopted classes sit at their mean, the others near beta: far apart, whatever the rounding
            got = chi_dev.cpu().double()
            assert bool(((got[role == 0] / avg64[role == 0] - 1).abs() < 1e-5).all())
            assert bool((got[role != 0] < 0.011).all()) and bool((avg64[role == 0] > 0.012).all())
        d64, f64 = _vectors64(chi64, focal_p)
        _report("class_state", (C, focal_p, it), {
            "chi": _ratio(chi_dev, chi64, chi32),
            "disc": _ratio(disc, d64, head_ref.threshold_discount(chi32, BETA)),
            "focal": _ratio(focal, f64, head_ref.focal_weight(chi32, focal_p))})
