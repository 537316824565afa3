"""Winograd F(4x4,3x3) forward and data gradient of the wide dilated 3x3 convolutions (filter_transform4 / input_transform4 /
output_transform4 of csrc/winograd.hip around conv_gemm_batched with 36 entries; ops.winograd4_conv): accuracy against float64 ATen
with a float32 emulation of the same transforms as the bound, the epilogue's bit-exact contracts, operands between guard bands, the
workspace contract, and the engine routing.  Shapes (N, Cin, Cout, H, W, dilation):
    (1, 16, 128, 9, 8, 1)       two tiles on the short axis, the minimum; 6 tiles padded to 8
    (1, 32, 128, 17, 19, 1)     ragged last tile; 25 tiles padded to 28
    (3, 48, 256, 21, 23, 2)     three images, unequal phases, 256 outputs (two row tiles of the point GEMMs); 108 tiles
    (2, 64, 128, 33, 35, 4)     q % 4 == 0, so leftover tiles of the longer phases; 198 tiles padded to 200
The transposed (data-gradient) runs swap the channel counts, so that the output is the 128- or 256-wide side in both."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import winograd4_conv_ref as W4C
from conftest import rel_err
from test_gpu_winograd import _pack_bits, _words

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, 128, 9, 8, 1), (1, 32, 128, 17, 19, 1), (3, 48, 256, 21, 23, 2), (2, 64, 128, 33, 35, 4)]
CASES = [(s, t) for s in SHAPES for t in (False, True)]
IDS = ["{}x{}to{}_{}x{}_d{}{}".format(*s, "_T" if t else "") for s, t in CASES]


def _spec_dims(shape, transposed):
    """(spec channel counts Cin, Cout; gathered channels K; output channels M): the output side is always the wide one."""
    N, small, wide, H, W, d = shape
    Cin, Cout = (wide, small) if transposed else (small, wide)
    return Cin, Cout, small, wide


@functools.lru_cache(maxsize=None)
def _case(shape, transposed):
    """Inputs, the float64 reference and the float32 emulation of one case, computed once and shared (read-only) by the tests."""
    N, _, _, H, W, d = shape
    Cin, Cout, K, M = _spec_dims(shape, transposed)
    g = torch.Generator().manual_seed(5000 + H * W + d + int(transposed))
    x = torch.randn(N, K, H, W, generator=g)
    if not transposed:
        x = torch.relu(x)                                              # post-ReLU activations, as the layers see them
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    scale = torch.rand(Cout, generator=g) + 0.5
    shift = torch.randn(M, generator=g) * 0.1
    ws = w.double() * scale.double().view(-1, 1, 1, 1)
    conv = F.conv_transpose2d if transposed else F.conv2d
    ref = conv(x.double(), ws, padding=d, dilation=d)
    emu = W4C.conv(x, w * scale.view(-1, 1, 1, 1), d, transposed)      # float32 throughout
    return {"x": x, "w": w, "scale": scale, "shift": shift, "ref": ref, "emu": emu}


def _max_err(a, ref):
    a = a.detach().double().cpu()
    assert bool(torch.isfinite(a).all()), "an element was not written"
    return float((a - ref).abs().max())


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


@pytest.mark.parametrize("shape,transposed", CASES, ids=IDS)
def test_against_fp64_with_the_emulated_transforms_as_the_bound(shape, transposed):
    """Output pre-filled with NaN (every element is written and finite); error against float64 <= 2 x the error of the same
    transforms emulated in float32 on the CPU (the bound of tests/test_gpu_winograd4_wgrad.py) and <= 1e-4 of the tensor maximum.
    The ratio to the direct kernel's error is printed (profiles/EXPERIMENTS.md records it), not bounded.  Two runs give the same bits."""
    from dasac_hip import ops
    N, _, _, H, W, d = shape
    Cin, Cout, K, M = _spec_dims(shape, transposed)
    c = _case(shape, transposed)
    x, w, scale = (c[k].cuda() for k in ("x", "w", "scale"))
    spec = ops.ConvSpec(Cin, Cout, [(3, 3, d, d)])
    assert ops.winograd_ok(spec, transposed)
    direct = ops.conv_dgrad(spec, x, [w], (H, W), scale=scale) if transposed else ops.conv_forward(spec, x, [w], scale=scale)
    u = ops.winograd4_filter(spec, w, transposed, scale)
    wino = ops.winograd4_conv(x, u, _nan(N, M, H, W), d)
    again = ops.winograd4_conv(x, u, _nan(N, M, H, W), d)
    ref = c["ref"]
    e_direct, e_wino, e_emu = _max_err(direct, ref), _max_err(wino, ref), _max_err(c["emu"], ref)
    top = float(ref.abs().max())
    print("conv4 {} {}: direct {:.3e}  F(4x4) {:.3e}  emulated {:.3e}  ratio to direct {:.2f}  to emulated {:.2f}  of max {:.2e}".format(
        "dgrad  " if transposed else "forward", shape, e_direct, e_wino, e_emu, e_wino / e_direct, e_wino / max(e_emu, 1e-30), e_wino / top))
    assert e_direct > 0 and e_emu > 0
    assert e_wino <= 2 * e_emu, (e_wino, e_emu)
    assert e_wino <= 1e-4 * top, (e_wino, top)
    assert torch.equal(wino.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize("shape,transposed", CASES, ids=IDS)
def test_epilogue_is_bit_exact(shape, transposed):
    """stored == relu(plain + shift) bit for bit; the recorded bits == stored > 0 of the path's own output, every word written (the
    bits past the last pixel as zeros); a masked run equals the unmasked one with exactly the cleared elements zero."""
    from dasac_hip import ops
    N, _, _, H, W, d = shape
    Cin, Cout, K, M = _spec_dims(shape, transposed)
    c = _case(shape, transposed)
    dev = torch.device("cuda")
    x, w, scale, shift = (c[k].cuda() for k in ("x", "w", "scale", "shift"))
    spec = ops.ConvSpec(Cin, Cout, [(3, 3, d, d)])
    u = ops.winograd4_filter(spec, w, transposed, scale)
    plain = ops.winograd4_conv(x, u, _nan(N, M, H, W), d)

    bits = ops.ReluBits(N, M, H, W, dev)
    bits.words.fill_(-1)
    stored = ops.winograd4_conv(x, u, _nan(N, M, H, W), d, shift, relu=True, bits_out=bits)
    want = torch.relu(plain + shift.view(1, M, 1, 1))
    assert torch.equal(stored.view(torch.int32), want.view(torch.int32))
    positive = (stored > 0).permute(1, 0, 2, 3).reshape(M, -1).cpu().numpy()
    assert 0.2 < positive.mean() < 0.8
    assert np.array_equal(_words(bits, M), _pack_bits(positive))

    g = torch.Generator().manual_seed(11 + H)
    mask = ops.ReluBits(N, M, H, W, dev)
    mask.words.copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, mask.words.shape, generator=g, dtype=torch.int64).to(torch.int32))
    masked = ops.winograd4_conv(x, u, _nan(N, M, H, W), d, mask_bits=mask)
    word = torch.from_numpy(_words(mask, M)).to(dev)
    pix = torch.arange(N * H * W, device=dev)
    keep = ((word[:, pix >> 5] >> (pix & 31)) & 1).bool().view(M, N, H, W).permute(1, 0, 2, 3)
    assert 0.3 < float(keep.float().mean()) < 0.7
    assert torch.equal(masked.view(torch.int32), torch.where(keep, plain, torch.zeros_like(plain)).view(torch.int32))
    # the recorded pattern of one call masks the next like the fp32 activation would
    again = ops.winograd4_conv(x, u, _nan(N, M, H, W), d, mask_bits=bits)
    assert torch.equal(again, torch.where(stored > 0, plain, torch.zeros_like(plain)))


# ---- routing ---------------------------------------------------------------------------------------------------------------------
def test_predicate():
    from dasac_hip import ops
    l4, l3 = ops.ConvSpec(512, 512, [(3, 3, 4, 4)]), ops.ConvSpec(256, 256, [(3, 3, 2, 2)])
    for transposed, grad in ((False, True), (False, False), (True, True)):
        routed = (512, 512, 4, transposed, grad) in ops.WINOGRAD4_ROUTES
        assert ops.winograd4_routed(l4, transposed, 2, 33, 33, grad) == routed
        assert not ops.winograd4_routed(l4, transposed, 2, 13, 11, grad) and not ops.winograd4_routed(l4, transposed, 2, 33, 31, grad)
    assert ops.winograd4_routed(l3, False, 1, 17, 17, False) == ((256, 256, 2, False, False) in ops.WINOGRAD4_ROUTES)
    assert not ops.winograd4_routed(l3, False, 1, 15, 17, False)
    # a grad-enabled pass of layer3 keeps the direct launches tests/test_gpu_fullres.py counts, whatever was measured
    assert not ops.winograd4_routed(l3, False, 8, 97, 97, True) and not ops.winograd4_routed(l3, True, 8, 97, 97, True)
    assert not ops.winograd4_routed(ops.ConvSpec(512, 512, [(3, 3, 1, 1)]), False, 8, 64, 128, False)       # VGG16: not measured
    ops.set_conv_algorithm("direct")
    try:
        assert not ops.winograd4_routed(l4, True, 2, 33, 33, True)
    finally:
        ops.set_conv_algorithm("auto")


ALL_L4 = {(512, 512, 4, True, True), (512, 512, 4, False, True), (512, 512, 4, False, False)}
SPANS4 = ("winograd4_input", "winograd4_output")


def _engine_run(plan, x, gout, mode):
    """(output, parameter gradients or None, profile by span name): gout None runs under torch.no_grad()."""
    from dasac_hip import engine as E
    from dasac_hip import ops
    ops.set_conv_algorithm(mode)
    try:
        eng = E.Engine(plan)
        for p in eng.params:
            p.grad = None
        ops.PROFILE.start()
        if gout is None:
            with torch.no_grad():
                out = E.run_plan(eng, x)
        else:
            out = E.run_plan(eng, x)
            out.backward(gout)
        names = ops.PROFILE.stop()
        return out.detach(), None if gout is None else [p.grad.clone() for p in eng.params], names
    finally:
        ops.set_conv_algorithm("auto")


def _relu_patterns(plan, x, mode):
    """The sign pattern of every activation of one kept forward under conv algorithm `mode`."""
    from dasac_hip import engine as E
    from dasac_hip import ops
    ops.set_conv_algorithm(mode)
    try:
        _, saved = E.Engine(plan).forward(x, keep=True)
        return {k: a > 0 for k, a in saved["acts"].items()}
    finally:
        ops.set_conv_algorithm("auto")


def test_engine_routes_a_layer4_bottleneck_and_agrees_with_the_direct_path(monkeypatch):
    """512 planes, dilation 4, 2 x 33 x 33 (H // d = 8), all three layer4 routes on whatever the measured table says: forward and
    data gradient take the F(4x4) spans once each, output within 1e-4 and parameter gradients within 1e-3 of the direct path's.

    The gradient of a ReLU network is continuous in the activations only while the ReLU pattern stays: among the 1.1 million
    pre-activations of conv2 one may lie within the two paths' rounding difference of zero, and that single flipped ReLU moves whole
    gradient rows by about 1e-2 of their maximum -- for ANY two roundings.  Measured on the MI355X against the direct path, worst
    parameter gradient at the seeds 545 / 1 / 2: the existing F(2x2) path 2.5e-6 / 1.6e-2 / 8.6e-3, F(4x4) 1.6e-2 / 4.3e-6 / 8.6e-3;
    the data gradient alone as F(4x4) adds 1e-6 to the F(2x2) figures; 3 - 6 of the block's 5.5 million ReLU decisions differed at
    each of four further draws.  So the two ReLUs behind the routed convolution (conv2's and the block's last) get BN shifts that
    keep every one of their pre-activations well above zero -- the test checks that it is so -- and the block compares what this
    test is about, the arithmetic of the two paths.  conv1's ReLU in front keeps its mixed pattern (it is the same direct launch
    under both algorithms), so the F(4x4) data gradient is masked with real bits."""
    from dasac_hip import ops
    from test_gpu_winograd_wgrad import _bottleneck, _plan_of
    monkeypatch.setattr(ops, "WINOGRAD4_ROUTES", ALL_L4)
    blk = _bottleneck(64, 512, 4)
    g = torch.Generator().manual_seed(545)
    x, gout = torch.randn(2, 64, 33, 33, generator=g), torch.randn(2, 2048, 33, 33, generator=g).cuda()
    blk.cpu()
    with torch.no_grad():                                  # shifts that put the smallest pre-activation as far above zero as it was below
        a1 = torch.relu(blk.bn1(blk.conv1(x)))
        z2 = blk.bn2(blk.conv2(a1))
        blk.bn2.bias.add_(2.0 * float(-z2.min()))
        z3 = blk.bn3(blk.conv3(torch.relu(blk.bn2(blk.conv2(a1))))) + blk.downsample(x)
        blk.bn3.bias.add_(2.0 * float(-z3.min()))
    blk.cuda()
    x = x.cuda()
    plan, spec = _plan_of(blk)
    assert ops.winograd4_routed(spec, False, 2, 33, 33, True) and ops.winograd4_routed(spec, True, 2, 33, 33, True)
    pd, pw = _relu_patterns(plan, x, "direct"), _relu_patterns(plan, x, "auto")
    assert sum(int((pd[k] != pw[k]).sum()) for k in pd) == 0
    on = sorted(float(p.float().mean()) for k, p in pd.items() if k != 0)
    assert on[-2:] == [1.0, 1.0] and 0.2 < on[0] < 0.8, on            # conv2's and the last ReLU all on, conv1's mixed
    out_d, grads_d, names_d = _engine_run(plan, x, gout, "direct")
    out_w, grads_w, names_w = _engine_run(plan, x, gout, "auto")
    out_w2, grads_w2, _ = _engine_run(plan, x, gout, "auto")
    for s in SPANS4:
        assert s not in names_d and names_w[s]["launches"] == 2, s                  # forward + data gradient
    assert "winograd_input" not in names_w and "winograd_output" not in names_w
    assert rel_err(out_w, out_d) < 1e-4
    errs = [rel_err(a, b) for a, b in zip(grads_w, grads_d)]
    print("layer4 bottleneck, F(4x4) vs direct: output {:.2e}, worst parameter gradient {:.2e}".format(rel_err(out_w, out_d), max(errs)))
    assert max(errs) < 1e-3, errs
    assert torch.equal(out_w.view(torch.int32), out_w2.view(torch.int32))
    for a, b in zip(grads_w, grads_w2):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_engine_routes_layer3_in_no_grad_forwards_only(monkeypatch):
    """256 planes, dilation 2, 1 x 17 x 17: under torch.no_grad() the conv2 takes the F(4x4) spans; with grad enabled its forward and
    data gradient take none and still run as conv_gemm launches (the launch count tests/test_gpu_fullres.py asserts)."""
    from dasac_hip import ops
    from test_gpu_winograd_wgrad import _bottleneck, _plan_of
    monkeypatch.setattr(ops, "WINOGRAD4_ROUTES", {(256, 256, 2, False, False)})
    plan, spec = _plan_of(_bottleneck(64, 256, 2))
    g = torch.Generator().manual_seed(273)
    x, gout = torch.randn(1, 64, 17, 17, generator=g).cuda(), torch.randn(1, 1024, 17, 17, generator=g).cuda()
    out_d, _, names_d = _engine_run(plan, x, None, "direct")
    out_n, _, names_n = _engine_run(plan, x, None, "auto")
    for s in SPANS4:
        assert s not in names_d and names_n[s]["launches"] == 1, s
    assert names_n["conv_gemm<batched>"]["launches"] == 1
    assert rel_err(out_n, out_d) < 1e-4
    _, _, names_g = _engine_run(plan, x, gout, "auto")
    _, _, names_gd = _engine_run(plan, x, gout, "direct")
    assert not any(s.startswith(("winograd4_input", "winograd4_output", "winograd_input", "winograd_output")) for s in names_g), sorted(names_g)
    gemm = lambda names: sum(v["launches"] for k, v in names.items() if k.startswith("conv_gemm") and "batched" not in k)
    assert gemm(names_g) == gemm(names_gd) > 0


# ---- operand placement and workspace ---------------------------------------------------------------------------------------------
PLACED = SHAPES[3]          # 2 x 9 x 11 = 198 tiles padded to 200, dilation 4: the padding tiles lie next to the guards


@pytest.mark.parametrize("transposed", [False, True], ids=["forward", "dgrad"])
def test_operands_between_guards_at_every_alignment_phase(monkeypatch, transposed):
    from dasac_hip import ops
    from test_gpu_operand_placement import _gen, _sweep
    N, _, _, H, W, d = PLACED
    Cin, Cout, K, M = _spec_dims(PLACED, transposed)
    spec = ops.ConvSpec(Cin, Cout, [(3, 3, d, d)])

    def case(a):
        g = _gen(sum(PLACED))
        w = a.place(torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5)
        x, shift, scale = a.place(torch.randn(N, K, H, W, generator=g)), a.place(torch.randn(M, generator=g)), a.place(torch.rand(Cout, generator=g) + 0.5)
        u = ops.winograd4_filter(spec, w, transposed, scale)
        dev = x.device
        bits = ops.ReluBits(N, M, H, W, dev)
        y = ops.winograd4_conv(x, u, a.torch.empty((N, M, H, W), dtype=torch.float32, device=dev), d, shift, relu=True, bits_out=bits)
        masked = ops.winograd4_conv(x, u, a.torch.empty((N, M, H, W), dtype=torch.float32, device=dev), d, mask_bits=bits)
        return [u, y, bits, masked]
    _sweep(monkeypatch, case)


@pytest.mark.parametrize("transposed", [False, True], ids=["forward", "dgrad"])
def test_wrapper_runs_on_exactly_the_workspace_it_asks_for(monkeypatch, transposed):
    from dasac_hip import ops
    from test_gpu_workspace_contract import _gen, _three_runs
    N, _, _, H, W, d = PLACED
    Cin, Cout, K, M = _spec_dims(PLACED, transposed)
    g = _gen(sum(PLACED))
    spec = ops.ConvSpec(Cin, Cout, [(3, 3, d, d)])
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5).cuda()
    x, shift = torch.randn(N, K, H, W, generator=g).cuda(), torch.randn(M, generator=g).cuda()
    u = ops.winograd4_filter(spec, w, transposed)

    def run():
        return [ops.winograd4_conv(x, u, _nan(N, M, H, W), d, shift, relu=True)]
    _three_runs(monkeypatch, run, "winograd4_conv")


def test_output_entry_point_refuses_a_workspace_one_byte_short():
    from dasac_hip import lib as L
    from test_gpu_workspace_contract import _filled, _refuses_one_byte_short
    lib, s = L.load(), L.stream_ptr()
    N, _, M, H, W, d = PLACED
    T = lib.dasac_winograd4_tiles(N, H, W, d)
    assert T == 200
    out = _filled((N, M, H, W))
    _refuses_one_byte_short("dasac_winograd4_output", 144 * M * T, lambda p, n: lib.dasac_winograd4_output(
        p, n, N, M, H, W, d, None, 0, None, None, out.data_ptr(), s), [out], poison=0x00)
