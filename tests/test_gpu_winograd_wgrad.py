"""Winograd F(2x2,3x3) weight gradient of the wide dilated 3x3 convolutions (csrc/winograd.hip grad_transform / wgrad_finish around
conv_wgrad_batched of csrc/conv_wgrad.hip; ops.winograd_wgrad): accuracy against float64 ATen with the direct path as the yardstick,
bit-exactness on the summable lattice, the routing predicate's refusals and the engine routing on one layer4-shaped bottleneck.
Shapes are the smallest that reach every way to go wrong: both channel orientations (M and K swapped), dilations 1, 2 and 4 on
11 x 9 and 13 x 10 maps (unequal phases, tiles that hang over both edges), tile counts that are no multiple of the 32-pixel K-step
(ragged last step) and one shape with four pixel splits, the last of them ragged."""
import functools

import pytest
import torch
import torch.nn as nn

import conv_lattice as CL
from conftest import rel_err

pytestmark = pytest.mark.gpu

# (N, Cin, Cout, H, W, dilation) -> tiles T: 60, 60, 144, 84 (one split each), 816 (4 splits of 224, 224, 224, 144 tiles)
SHAPES = [(2, 128, 256, 11, 9, 1), (2, 256, 128, 11, 9, 2), (3, 128, 256, 13, 10, 4), (2, 256, 128, 13, 10, 2), (3, 128, 128, 33, 31, 1)]
IDS = ["{}x{}to{}_{}x{}_d{}".format(*s) for s in SHAPES]
SPANS = ("winograd_wgrad_input", "winograd_wgrad_grad", "winograd_wgrad_gemm", "winograd_wgrad_finish")


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs and the float64 references of one shape, computed once and shared (read-only) by the tests."""
    N, Cin, Cout, H, W, d = shape
    g = torch.Generator().manual_seed(2000 + H * W + d + Cin)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    scale = torch.rand(Cout, generator=g) + 0.5
    dz = torch.randn(N, Cout, H, W, generator=g)
    gw = torch.nn.grad.conv2d_weight(x.double(), (Cout, Cin, 3, 3), dz.double(), padding=d, dilation=d)      # unscaled
    return {"x": x, "w": w, "scale": scale, "dz": dz, "dw": gw * scale.double().view(-1, 1, 1, 1),
            "dot": (gw * w.double()).sum((1, 2, 3)), "sum_dz": dz.double().sum((0, 2, 3))}


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def _max_err(a, ref):
    a = a.detach().double().cpu()
    assert bool(torch.isfinite(a).all()), "an element was not written"
    return float((a - ref).abs().max())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_weight_gradient_against_fp64_with_the_direct_path_as_yardstick(shape):
    """dW, the dot rows summed and sum_dz: Winograd error <= 4 x the direct path's measured error on the same inputs (the rule of
    tests/test_gpu_winograd.py for the forward and the data gradient).  Outputs are pre-filled with NaN: every element is written."""
    from dasac_hip import ops
    N, Cin, Cout, H, W, d = shape
    c = _case(shape)
    x, w, scale, dz = (c[k].cuda() for k in ("x", "w", "scale", "dz"))
    spec = ops.ConvSpec(Cin, Cout, [(3, 3, d, d)])
    assert ops.winograd_ok(spec)
    rows = ops.dot_rows(spec)

    dot_d, sum_d = _nan(rows, Cout), _nan(Cout)
    (dw_d,) = ops.conv_wgrad(spec, dz, x, [w], scale=scale, dot=dot_d, sum_dz=sum_d, outs=[_nan(Cout, Cin, 3, 3)])
    dot_w, sum_w = _nan(rows, Cout), _nan(Cout)
    dw_w = ops.winograd_wgrad(spec, dz, x, w, scale=scale, dot=dot_w, sum_dz=sum_w, out=_nan(Cout, Cin, 3, 3))
    for name, direct, wino in (("dw", dw_d, dw_w), ("dot", dot_d.sum(0), dot_w.sum(0)), ("sum_dz", sum_d, sum_w)):
        e_direct, e_wino = _max_err(direct, c[name]), _max_err(wino, c[name])
        print("wgrad {:6s} {}: direct {:.3e}  winograd {:.3e}  ratio {:.2f}".format(name, shape, e_direct, e_wino, e_wino / e_direct))
        assert e_direct > 0
        assert e_wino <= 4 * e_direct, (name, e_wino, e_direct)


@pytest.mark.parametrize("with_scale", [False, True], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4]], ids=[IDS[2], IDS[4]])
def test_weight_gradient_is_bit_exact_on_the_summable_lattice(shape, with_scale):
    """Integer operands: A dY A^T and B^T x B are integers of magnitude <= 4 max|dz| and <= 4 max|x|, so every point sum over the T
    tiles is an exact integer below T * 16 max|dz| max|x|; G^T (.) G adds at most 16 of them in quarter steps (the lattice spacing
    `winograd_quantum` of the forward's G g G^T), and the power-of-two scale is exact.  With 16 * bound below 2^24 * quantum no
    order of summation rounds: dW and sum_dz equal the float64 reference bit for bit.  (`winograd_exact_ok` bounds the forward's
    contraction over channels, not this one over tiles; the bound here is the corresponding one.)"""
    from dasac_hip import lib as L
    from dasac_hip import ops
    N, Cin, Cout, H, W, d = shape
    branches = [(3, 3, d, d)]
    o = CL.plain_operands(Cin, Cout, branches, 1, (N, H, W), seed=11)
    x, dz, w = o["x"], o["dz"], o["ws"][0]
    scale = o["scale"] if with_scale else None
    T = L.load().dasac_winograd_tiles(N, H, W, d)
    bound = T * 16.0 * float(dz.abs().max()) * float(x.abs().max())
    assert 16 * bound < CL.P24 * CL.winograd_quantum(None) and float(dz.abs().double().sum((0, 2, 3)).max()) < CL.P24
    (ref,) = CL.conv_dw(dz, x, [w], branches, 1, scale)
    spec = ops.ConvSpec(Cin, Cout, branches)
    sums = _nan(Cout)
    dw = ops.winograd_wgrad(spec, dz.cuda(), x.cuda(), w.cuda(), scale=None if scale is None else scale.cuda(), sum_dz=sums,
                            out=_nan(Cout, Cin, 3, 3))
    assert float(ref.abs().max()) > 0
    assert torch.equal(dw.cpu(), CL.f32(ref))               # torch.equal, as tests/test_gpu_conv_exact.py: NaN equals nothing
    assert torch.equal(sums.cpu(), CL.f32(dz.double().sum((0, 2, 3))))


def _bottleneck(inplanes, planes, dilation):
    from models.deeplabv2 import Bottleneck, BatchNorm
    torch.manual_seed(3)
    down = nn.Sequential(nn.Conv2d(inplanes, 4 * planes, 1, bias=False), BatchNorm(4 * planes))
    blk = Bottleneck(inplanes, planes, dilation=dilation, downsample=down)
    for m in blk.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight)
        elif isinstance(m, BatchNorm):
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.2)
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.5, 1.5)
    return blk.cuda().eval()


def _run(plan, x, gout, mode):
    """One forward and backward through the engine under conv algorithm `mode`: (parameter gradients, profile by span name)."""
    from dasac_hip import engine as E
    from dasac_hip import ops
    ops.set_conv_algorithm(mode)
    try:
        eng = E.Engine(plan)
        for p in eng.params:
            p.grad = None
        ops.PROFILE.start()
        E.run_plan(eng, x).backward(gout)
        names = ops.PROFILE.stop()
        return [p.grad.clone() for p in eng.params], names
    finally:
        ops.set_conv_algorithm("auto")


def _plan_of(blk):
    from dasac_hip import engine as E
    P = E.Plan()
    plan = P.finish(blk.plan(P, 0))
    (conv2,) = [op for op in plan.ops if op.spec.taps == 9]
    return plan, conv2.spec


# what the batched launch cannot do: a tile count that is no multiple of 4 (2 x 35 tiles), input channels that are no multiple of
# 128, split-bf16 arithmetic.  (planes, N, H, W, precision)
REFUSED = {"T%4": (128, 2, 11, 9, "fp32"), "C%128": (192, 2, 13, 11, "fp32"), "bf16x3": (128, 2, 13, 11, "bf16x3")}


@pytest.mark.parametrize("why", list(REFUSED))
def test_predicate_refuses_what_the_launch_cannot_do_and_the_engine_stays_direct(why, monkeypatch):
    from dasac_hip import ops
    planes, N, H, W, precision = REFUSED[why]
    monkeypatch.setattr(ops, "WINOGRAD_WGRAD_MIN_CHANNEL_PRODUCT", 0)       # width is not what refuses these
    ops.set_precision(precision)
    try:
        plan, spec = _plan_of(_bottleneck(64, planes, 4))
        assert not ops.winograd_wgrad_routed(spec, N, H, W)
        g = torch.Generator().manual_seed(5)
        x, gout = torch.randn(N, 64, H, W, generator=g).cuda(), torch.randn(N, 4 * planes, H, W, generator=g).cuda()
        grads_a, names_a = _run(plan, x, gout, "auto")
        grads_d, _ = _run(plan, x, gout, "direct")
    finally:
        ops.set_precision("fp32")
    assert not any(s in names_a for s in SPANS)
    for a, b in zip(grads_a, grads_d):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_engine_routes_the_layer4_weight_gradient_and_gradients_agree_with_the_direct_path(monkeypatch):
    """The layer4 bottleneck of tests/test_gpu_winograd.py (2 x 64 x 13 x 11, conv2 512 -> 512, dilation 4, frozen BN): the new
    spans once under "auto" and not at all under "direct", every parameter gradient within that file's 1e-3 (of the tensor's
    maximum) bound, identical bits from two "auto" runs."""
    from dasac_hip import ops
    monkeypatch.setattr(ops, "WINOGRAD_WGRAD_MIN_CHANNEL_PRODUCT", 512 * 512)
    plan, spec = _plan_of(_bottleneck(64, 512, 4))
    assert ops.winograd_wgrad_routed(spec, 2, 13, 11)
    x, gout = torch.randn(2, 64, 13, 11, device="cuda"), torch.randn(2, 2048, 13, 11, device="cuda")
    grads_d, names_d = _run(plan, x, gout, "direct")
    grads_w, names_w = _run(plan, x, gout, "auto")
    grads_w2, _ = _run(plan, x, gout, "auto")
    for s in SPANS:
        assert s not in names_d and names_w[s]["launches"] == 1, s
    assert names_w["winograd_wgrad_gemm"]["flops"] == 2.0 * 16 * 512 * 512 * 112
    errs = [rel_err(a, b) for a, b in zip(grads_w, grads_d)]
    print("parameter gradients, winograd vs direct: worst rel err {:.2e}".format(max(errs)))
    assert max(errs) < 1e-3, errs
    for a, b in zip(grads_w, grads_w2):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
