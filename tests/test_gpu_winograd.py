"""Winograd F(2x2,3x3) path of the wide dilated 3x3 convolutions (csrc/winograd.hip, ops.winograd_*): accuracy of the forward and the
data gradient against an fp64 convolution with the direct path as the yardstick, the epilogue's bit-exact contracts, and the engine
routing on one layer4-shaped bottleneck.  Shapes are the smallest that reach every path of the index arithmetic: a map narrower than
two dilations (one-tile and empty phases), odd sizes, dilation 1, and the real 97 x 97 / dilation 4 phase geometry at 16 channels."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

# (N, Cin, Cout, H, W, dilation)
SHAPES = [(2, 32, 128, 9, 7, 4), (1, 32, 128, 11, 13, 2), (2, 16, 128, 10, 10, 1), (1, 16, 128, 97, 97, 4)]
IDS = ["{}x{}to{}_{}x{}_d{}".format(*s) for s in SHAPES]


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs and the fp64 references of one shape, computed once and shared (read-only) by the tests."""
    N, Cin, Cout, H, W, d = shape
    g = torch.Generator().manual_seed(1000 + H * W + d)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    scale = torch.rand(Cout, generator=g) + 0.5
    dz = torch.randn(N, Cout, H, W, generator=g)
    ws = (w.double() * scale.double().view(-1, 1, 1, 1))
    fwd = F.conv2d(x.double(), ws, padding=d, dilation=d)
    dx = F.conv_transpose2d(dz.double(), ws, padding=d, dilation=d)
    return {"x": x, "w": w, "scale": scale, "dz": dz, "fwd": fwd, "dx": dx}


def _max_err(a, ref):
    return float((a.detach().double().cpu() - ref).abs().max())


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_and_data_gradient_against_fp64_with_the_direct_path_as_yardstick(shape):
    """Winograd error <= 4 x the direct path's measured error on the same inputs (a 4x4 patch sum grows magnitudes by at most 4 and
    the transforms add two roundings on each side)."""
    from dasac_hip import ops
    N, Cin, Cout, H, W, d = shape
    c = _case(shape)
    dev = torch.device("cuda")
    x, w, scale, dz = (c[k].to(dev) for k in ("x", "w", "scale", "dz"))
    spec = ops.ConvSpec(Cin, Cout, [(3, 3, d, d)])
    assert ops.winograd_ok(spec, False) and ops.winograd_ok(spec, True)

    direct = ops.conv_forward(spec, x, [w], scale=scale)
    wino = ops.winograd_conv(x, ops.winograd_filter(spec, w, False, scale), torch.empty_like(direct), d)
    e_direct, e_wino = _max_err(direct, c["fwd"]), _max_err(wino, c["fwd"])
    print("forward  {}: direct {:.3e}  winograd {:.3e}  ratio {:.2f}".format(shape, e_direct, e_wino, e_wino / e_direct))

    direct_dx = ops.conv_dgrad(spec, dz, [w], (H, W), scale=scale)
    wino_dx = ops.winograd_conv(dz, ops.winograd_filter(spec, w, True, scale), torch.empty_like(direct_dx), d)
    g_direct, g_wino = _max_err(direct_dx, c["dx"]), _max_err(wino_dx, c["dx"])
    print("dgrad    {}: direct {:.3e}  winograd {:.3e}  ratio {:.2f}".format(shape, g_direct, g_wino, g_wino / g_direct))

    assert e_direct > 0 and g_direct > 0
    assert e_wino <= 4 * e_direct, (e_wino, e_direct)
    assert g_wino <= 4 * g_direct, (g_wino, g_direct)


def _pack_bits(positive):
    """[M, Npix] bool -> [M, ceil(Npix / 32)] words, bit (pix & 31) of word pix >> 5, as int64 values of the uint32 words."""
    M, n = positive.shape
    w32 = (n + 31) // 32
    padded = np.zeros((M, w32 * 32), dtype=np.uint64)
    padded[:, :n] = positive
    return (padded.reshape(M, w32, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.int64)


def _words(bits, M):
    return (bits.words.cpu().numpy().astype(np.int64) & 0xFFFFFFFF).reshape(M, -1)


@pytest.mark.parametrize("shape", SHAPES[:3], ids=IDS[:3])
def test_output_transform_epilogue_is_bit_exact(shape):
    """stored == relu(unmasked + shift) bit for bit; the recorded bits == stored > 0; the masked mode zeroes exactly the cleared bits."""
    from dasac_hip import ops
    from dasac_hip import lib as L
    N, _, M, H, W, d = shape
    dev = torch.device("cuda")
    T = L.load().dasac_winograd_tiles(N, H, W, d)
    g = torch.Generator().manual_seed(7 + H)
    y = torch.randn(16, M, T, generator=g).to(dev)
    shift = torch.randn(M, generator=g).to(dev)
    plain = ops.winograd_output(y, torch.empty(N, M, H, W, device=dev), d)

    bits = ops.ReluBits(N, M, H, W, dev)
    bits.words.fill_(-1)                                  # every word must be written, the bits past the last pixel as zeros
    stored = ops.winograd_output(y, torch.empty(N, M, H, W, device=dev), d, shift=shift, relu=True, bits_out=bits)
    want = torch.relu(plain + shift.view(1, M, 1, 1))
    assert torch.equal(stored.view(torch.int32), want.view(torch.int32))
    positive = (stored > 0).permute(1, 0, 2, 3).reshape(M, -1).cpu().numpy()
    assert 0.2 < positive.mean() < 0.8
    assert np.array_equal(_words(bits, M), _pack_bits(positive))

    # shift and ReLU off, as in the data gradient: exactly the elements whose bit is clear become zero
    mask = ops.ReluBits(N, M, H, W, dev)
    mask.words.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, mask.words.shape, generator=g, dtype=torch.int64).to(torch.int32))
    masked = ops.winograd_output(y, torch.empty(N, M, H, W, device=dev), d, mask_bits=mask)
    word = torch.from_numpy(_words(mask, M)).to(dev)
    pix = torch.arange(N * H * W, device=dev)
    keep = ((word[:, pix >> 5] >> (pix & 31)) & 1).bool().view(M, N, H, W).permute(1, 0, 2, 3)
    assert 0.3 < float(keep.float().mean()) < 0.7
    want = torch.where(keep, plain, torch.zeros_like(plain))
    assert torch.equal(masked.view(torch.int32), want.view(torch.int32))
    # the recorded pattern of one call masks the next like the fp32 activation would
    again = ops.winograd_output(y, torch.empty(N, M, H, W, device=dev), d, mask_bits=bits)
    assert torch.equal(again, torch.where(stored > 0, plain, torch.zeros_like(plain)))


def test_engine_routes_a_layer4_bottleneck_and_gradients_agree_with_the_direct_path():
    """One bottleneck with layer4's conv2 (512 -> 512, dilation 4, frozen BN) through the engine with the Winograd path on and
    off: same output, every parameter gradient within the 1e-3 (of the tensor's maximum) bound of tests/test_gpu_models.py."""
    import torch.nn as nn
    from dasac_hip import engine as E
    from dasac_hip import ops
    from models.deeplabv2 import Bottleneck, BatchNorm
    torch.manual_seed(3)
    down = nn.Sequential(nn.Conv2d(64, 2048, 1, bias=False), BatchNorm(2048))
    blk = Bottleneck(64, 512, dilation=4, downsample=down)
    for m in blk.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight)
        elif isinstance(m, BatchNorm):
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.2)
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.5, 1.5)
    blk.cuda().eval()
    P = E.Plan()
    plan = P.finish(blk.plan(P, 0))
    x = torch.randn(2, 64, 13, 11, device="cuda")
    gout = torch.randn(2, 2048, 13, 11, device="cuda")
    conv2 = [op for op in plan.ops if op.spec.taps == 9]
    assert len(conv2) == 1 and ops.winograd_routed(conv2[0].spec, False, 2, 13, 11) and ops.winograd_routed(conv2[0].spec, True, 2, 13, 11)

    def run(mode):
        ops.set_conv_algorithm(mode)
        try:
            eng = E.Engine(plan)
            for p in eng.params:
                p.grad = None
            ops.PROFILE.start()
            out = E.run_plan(eng, x)
            out.backward(gout)
            names = ops.PROFILE.stop()
            return out.detach(), [p.grad.clone() for p in eng.params], names
        finally:
            ops.set_conv_algorithm("auto")

    out_d, grads_d, names_d = run("direct")
    out_w, grads_w, names_w = run("auto")
    assert "winograd_input" not in names_d and names_w["winograd_input"]["launches"] == 2      # forward + data gradient
    assert names_w["winograd_output"]["launches"] == 2
    assert rel_err(out_w, out_d) < 1e-4
    errs = [rel_err(a, b) for a, b in zip(grads_w, grads_d)]
    print("parameter gradients, winograd vs direct: worst rel err {:.2e}".format(max(errs)))
    assert max(errs) < 1e-3, errs
