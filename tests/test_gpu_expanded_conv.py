"""The tap-expanded ASPP convolution (ops.ExpandedConv: dasac_conv_pack_expanded, the dense 1x1 GEMM over E = taps*Cp rows,
dasac_tap_gather, dasac_tap_scatter, dasac_conv_wgrad_finish_expanded) driven the way engine.py drives every DeepLabv2
classifier, against float64 ATen on the CPU: out = sum_b conv2d(x, w_b, bias_b, padding=p_b, dilation=d_b) and its autograd
gradients.  (test_gpu_conv.py's `aspp4` case runs the generic multi-branch conv_gemm, not this path.)

Cases cover Cout 19 (Cp 20, E 720: production), 32 (E 1152, the quad weight-gradient tile), 16 and 2..5 (E < 256); Cin 2048,
1024, 192 (64-row k tiles) and 96 (Cin % 64 != 0); the ASPP branch set, a mixed set with unequal taps per branch, and 63 taps;
maps where only the centre taps land, partial overlap, cfg-3 size, non-square, several images; fp32 and bf16x3.

Forward and data gradient are bounded per element by tau * (|x| (*) |w|), the float64 conv of the absolute values: a
max-normalised error would hide a wrong small output.  Worst measured ratio got/bound on the MI355X: fp32 0.04 (tau 1e-5),
bf16x3 0.38 (tau 3e-5, the data gradient of the 2048 -> 2 case); weight gradients 7e-7 (fp32) and 6e-6 (bf16x3) of the
tensor max."""
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu
TAU = {"fp32": 1e-5, "bf16x3": 3e-5}
TOL_W = {"fp32": 1e-5, "bf16x3": 1e-4}        # weight gradients: error / tensor max

ASPP = [(3, 3, 6, 6), (3, 3, 12, 12), (3, 3, 18, 18), (3, 3, 24, 24)]      # deeplabv2.py:101-116, 36 taps
MIXED = [(1, 1, 1, 0), (3, 3, 2, 2), (5, 5, 1, 2)]                          # 1 + 9 + 25 taps: tap0 = 0, 1, 10
SEVEN = [(3, 3, d, d) for d in range(1, 8)]                                 # 63 taps

CASES = [
    # name, cin, cout, branches, (N, H, W), precision
    ("r101_cfg3", 2048, 19, ASPP, (2, 97, 97), "fp32"),
    ("r101_cfg3_x3", 2048, 19, ASPP, (2, 97, 97), "bf16x3"),
    ("r101_centre_only_cout2_x3", 2048, 2, ASPP, (1, 5, 7), "bf16x3"),
    ("vgg_centre_only", 1024, 19, ASPP, (1, 5, 7), "fp32"),
    ("vgg_cout32_quad", 1024, 32, ASPP, (2, 33, 41), "fp32"),
    ("vgg_mixed_nonsquare", 1024, 19, MIXED, (1, 65, 129), "fp32"),
    ("k64_cout16", 192, 16, ASPP, (3, 9, 13), "fp32"),
    ("k64_cout16_mixed_x3", 192, 16, MIXED, (1, 65, 129), "bf16x3"),
    ("k64_seven", 192, 19, SEVEN, (2, 33, 41), "fp32"),
    ("k64_cout32_x3", 192, 32, ASPP, (1, 65, 129), "bf16x3"),
    ("c96_cout3", 96, 3, ASPP, (2, 33, 41), "fp32"),
    ("c96_mixed", 96, 19, MIXED, (3, 9, 13), "fp32"),
    ("c96_seven_cout5_x3", 96, 5, SEVEN, (3, 9, 13), "bf16x3"),
    ("c96_cout19_x3", 96, 19, ASPP, (2, 33, 41), "bf16x3"),
]
_REF = {}
_USES = {}
for _c in CASES:
    _USES[repr(_c[1:5])] = _USES.get(repr(_c[1:5]), 0) + 1


def _inputs(cin, cout, branches, shape):
    N, H, W = shape
    g = torch.Generator().manual_seed(cin * 131 + cout * 7 + H + len(branches))
    x = (torch.randn(N, cin, H, W, generator=g) - 0.3).clamp_min(0)          # a ReLU output, as the classifier's input is
    ws = [torch.randn(cout, cin, kh, kw, generator=g) / (cin * kh * kw) ** 0.5 for kh, kw, _, _ in branches]
    bs = [torch.randn(cout, generator=g) for _ in branches]
    dout = torch.randn(N, cout, H, W, generator=g)
    res = torch.randn(N, cin, H, W, generator=g)
    return x, ws, bs, dout, res


def _reference(case):
    """float64: out, dx, dW per branch, d bias, and the absolute-value convs that scale the per-element bounds.  Cached for
    the cases that share inputs (fp32 / bf16x3 of one geometry), dropped after the last of them."""
    key = repr(case[1:5])
    if key in _REF:
        ref = _REF[key]
    else:
        _, cin, cout, branches, shape, _ = case
        x, ws, bs, dout, res = _inputs(cin, cout, branches, shape)
        xr = x.double().requires_grad_(True)
        wr = [w.double().requires_grad_(True) for w in ws]
        br = [b.double().requires_grad_(True) for b in bs]
        out = sum(F.conv2d(xr, w, b, 1, p, d) for w, b, (_, _, d, p) in zip(wr, br, branches))
        out.backward(dout.double())
        xa, da = x.double().abs(), dout.double().abs()
        with torch.no_grad():
            abs_fwd = sum(F.conv2d(xa, w.detach().abs(), None, 1, p, d) for w, (_, _, d, p) in zip(wr, branches))
            abs_fwd += sum(b.detach().abs() for b in br).view(1, -1, 1, 1)
            abs_dx = sum(torch.nn.grad.conv2d_input(x.shape, w.detach().abs(), da, 1, p, d) for w, (_, _, d, p) in zip(wr, branches))
        ref = dict(x=x, ws=ws, bs=bs, dout=dout, res=res, out=out.detach(), dx=xr.grad, dw=[w.grad for w in wr], db=br[0].grad,
                   abs_fwd=abs_fwd, abs_dx=abs_dx)
        _REF[key] = ref
    _USES[key] -= 1
    if _USES[key] == 0:
        del _REF[key]
    return ref


def _bound_ratio(got, ref, absref, tau):
    """max over elements of |got - ref| / (tau * absref + floor)."""
    err = (got.double().cpu() - ref).abs()
    floor = 1e-12 * float(absref.max())
    return float((err / (tau * absref + floor)).max())


def _dense(buf):
    """[Kpad][Mpad] view of a packed operand (element (k, m) at ((k >> 2) * Mpad + m) * 4 + (k & 3))."""
    kp, mp = buf.shape
    return buf.view(kp // 4, mp, 4).permute(0, 2, 1).reshape(kp, mp)


def _expected_dense(ex, ws, transposed, shape):
    """The packed operand as a dense matrix: row / column e = tap * Cp + co holds W_b[co, :, a, c]; pad channels co >= Cout,
    K padding and M padding are zero."""
    spec = ex.spec
    we = torch.zeros(spec.taps, ex.cp, spec.cin)
    tap0 = 0
    for w, (kh, kw, _, _) in zip(ws, spec.branches):
        we[tap0:tap0 + kh * kw, :spec.cout] = w.permute(2, 3, 0, 1).reshape(kh * kw, spec.cout, spec.cin)
        tap0 += kh * kw
    me = we.reshape(ex.E, spec.cin)
    dense = torch.zeros(shape)
    if transposed:
        dense[:ex.E, :spec.cin] = me
    else:
        dense[:spec.cin, :ex.E] = me.t()
    return dense


def _expected_scatter(ex, dout):
    """D[b, t*Cp + co, oh, ow] = dout[b, co, oh - dh_t, ow - dw_t] (zero off the map and for co >= Cout): a copy, no arithmetic."""
    N, cout, H, W = dout.shape
    shifts = [(a * d - p, c * d - p) for kh, kw, d, p in ex.spec.branches for a in range(kh) for c in range(kw)]
    P = max(max(abs(s) for s in t) for t in shifts)
    dp = F.pad(dout, (P, P, P, P))
    D = torch.zeros(N, ex.spec.taps, ex.cp, H, W)
    for t, (dh, dw) in enumerate(shifts):
        D[:, t, :cout] = dp[:, :, P - dh:P - dh + H, P - dw:P - dw + W]
    return D.view(N, ex.E, H, W)


def _check_packs(ex, wd, ws, prec):
    """Packing into a NaN-filled buffer and repacking new weights into that reused buffer (what Engine.packed does after an
    optimiser step) give exactly a fresh pack; in fp32 the buffer is checked element by element, padding included."""
    from dasac_hip import lib as L
    lib = L.load()
    out = []
    for tr in (False, True):
        M, K = (ex.spec.cin, ex.E) if tr else (ex.E, ex.spec.cin)
        shape = (lib.dasac_conv_kpad(K), lib.dasac_conv_mpad(M))
        buf = torch.full(shape, float("nan"), device="cuda")
        for scale in (1.0, 1.01):
            wsc = [w * scale for w in wd]
            got = ex.pack(wsc, tr, out=buf)
            assert got is buf and got.shape == shape
            fresh = ex.pack(wsc, tr)
            assert torch.equal(got, fresh), (tr, scale)
            if prec == "fp32":
                assert not getattr(got, "dasac_x3", False)
                want = _expected_dense(ex, [w * scale for w in ws], tr, shape)
                assert torch.equal(_dense(got).cpu(), want), (tr, scale)
        out.append(ex.pack(wd, tr))
    return out


def _relu_bits_of(x):
    """The ReLU bit pattern of x (a ReLU output) as the producing conv's epilogue records it: an identity 1x1 conv_gemm with
    relu and bits_out reproduces x exactly (products with 1 and 0) and writes its bits."""
    from dasac_hip import ops
    N, C, H, W = x.shape
    spec = ops.ConvSpec(C, C, [(1, 1, 1, 0)], 1)
    eye = torch.eye(C, device="cuda").view(C, C, 1, 1).contiguous()
    order = ops.gemm_order(spec, False)
    table, packed = ops.conv_table(spec, H, W, False, x.device, order), ops.conv_pack(spec, [eye], False, None, order=order)
    y = torch.empty_like(x)
    bits = ops.ReluBits(N, C, H, W, x.device)
    ops.conv_gemm(x, packed, table, y, (H, W), 1, C, spec.K, 1, None, None, None, True, bits_out=bits)
    assert torch.equal(y, x)
    return bits


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_expanded_conv_against_fp64(case):
    from dasac_hip import ops
    name, cin, cout, branches, shape, prec = case
    N, H, W = shape
    spec = ops.ConvSpec(cin, cout, branches, 1)
    ex = ops.ExpandedConv(spec)
    assert ex.E == spec.taps * ex.cp and ex.E % 16 == 0 and all((spec.taps * c) % 16 for c in range(cout, ex.cp))
    ref = _reference(case)
    x, ws, bs, dout, res = (ref[k] for k in ("x", "ws", "bs", "dout", "res"))
    tau = TAU[prec]
    saved = ops.PRECISION
    ops.set_precision(prec)
    try:
        xd, wd, doutd, resd = x.cuda(), [w.cuda() for w in ws], dout.cuda(), res.cuda()
        bias_sum = sum(b.cuda() for b in bs)                 # what Engine.fold hands the forward
        packed_f, packed_t = _check_packs(ex, wd, ws, prec)
        table_f = ops.conv_table(ex.spec1, H, W, False, xd.device)
        table_t = ops.conv_table(ex.spec1, H, W, True, xd.device)

        def run():
            out = ex.forward(xd, packed_f, table_f, bias_sum)
            d = ex.scatter(doutd)
            dws = ex.wgrad(d, xd, wd, table_f)
            dbias = ops.channel_sums(doutd)
            dx = ex.dgrad(d, packed_t, table_t, (H, W))
            dx_m = ex.dgrad(d, packed_t, table_t, (H, W), res=resd, mask=xd)
            return out, d, dws, dbias, dx, dx_m

        out, d, dws, dbias, dx, dx_m = run()
        torch.cuda.synchronize()
        r_out = _bound_ratio(out, ref["out"], ref["abs_fwd"], tau)
        assert out.shape == (N, cout, H, W) and r_out <= 1.0, (name, "forward", r_out)
        assert rel_err(out, ref["out"]) < tau
        # scatter: an exact copy of shifted dout planes; the pad channels co >= Cout exactly zero
        assert torch.equal(d.cpu(), _expected_scatter(ex, dout))
        assert not d.view(N, spec.taps, ex.cp, H, W)[:, :, cout:].any()
        # weight gradients: the split count of dasac_conv_wgrad_finish_expanded must be the one conv_wgrad_impl used
        w_err = max(rel_err(a, b) for a, b in zip(dws, ref["dw"]))
        assert w_err < TOL_W[prec], (name, "wgrad", w_err)
        assert rel_err(dbias, ref["db"]) < 1e-6
        r_dx = _bound_ratio(dx, ref["dx"], ref["abs_dx"], tau)
        assert r_dx <= 1.0, (name, "dgrad", r_dx)
        xpos = x > 0
        want_m = (ref["dx"] + res.double()) * xpos
        r_m = _bound_ratio(dx_m, want_m, (ref["abs_dx"] + res.double().abs()) * xpos, tau)
        assert r_m <= 1.0, (name, "masked dgrad", r_m)
        assert not dx_m.cpu()[~xpos].any()
        if ops.bits_ok(cin, ex.E):                           # the engine's route: the producer's ReLU bits
            assert prec == "fp32"
            dx_b = ex.dgrad(d, packed_t, table_t, (H, W), res=resd, mask=_relu_bits_of(xd))
            assert torch.equal(dx_b, dx_m)
        else:
            assert prec == "bf16x3"
        # determinism: a second run gives the same bits everywhere
        again = run()
        for a, b in zip((out, d, dbias, dx, dx_m) + tuple(dws), again[:2] + again[3:] + tuple(again[2])):
            assert torch.equal(a, b)
        print("{}: forward {:.3g}, dgrad {:.3g}, masked {:.3g} of the bound; wgrad {:.3g}".format(name, r_out, r_dx, r_m, w_err))
    finally:
        ops.set_precision(saved)


def test_more_than_64_taps_is_refused_before_any_launch():
    """The shift table holds 64 taps: 65 return the library's error from the host (nothing launched, nothing written); the
    Python wrapper refuses such a spec up front."""
    from dasac_hip import lib as L
    from dasac_hip import ops
    lib = L.load()
    br = SEVEN + [(1, 1, 1, 0), (1, 1, 1, 0)]                # 65 taps
    cols = [torch.tensor(c, dtype=torch.int32) for c in zip(*br)]
    ptrs = [c.data_ptr() for c in cols]
    y = torch.zeros(65 * 4 * 4, device="cuda")
    out = torch.full((4,), 7.0, device="cuda")
    rc = lib.dasac_tap_gather(y.data_ptr(), *ptrs, len(br), 1, 1, None, 1, 2, 2, out.data_ptr(), L.stream_ptr())
    assert rc != 0 and b"more than 64 taps" in lib.dasac_last_error()
    rc = lib.dasac_tap_scatter(out.data_ptr(), *ptrs, len(br), 1, 1, 1, 2, 2, y.data_ptr(), L.stream_ptr())
    assert rc != 0 and b"more than 64 taps" in lib.dasac_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and not y.any()
    with pytest.raises(AssertionError):
        ops.ExpandedConv(ops.ConvSpec(8, 3, br, 1))
    ops.ExpandedConv(ops.ConvSpec(8, 3, SEVEN, 1))           # 63 taps are accepted


def test_engine_rebuilds_expanded_packs_after_an_in_place_update():
    """After an in-place update of the classifier weights (what FusedSGD does), the engine's expanded packs -- forward and
    data-gradient layouts -- equal a fresh ExpandedConv.pack bit for bit, and the next forward of the classifier matches
    float64 sum_b conv2d on the activations it was given."""
    from types import SimpleNamespace as NS
    import torch.nn as nn
    import models
    from oracle import nets_ref as Nr
    from oracle.step_ref import DEFAULT_CFG
    cfg = NS(**dict(DEFAULT_CFG, INIT_MODEL="", OPT_NESTEROV=False))
    net = models.get_model(cfg, 0, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    net.backbone.load_state_dict(Nr.resnet101_state(seed=2, randomize_bn=True, he_init=True), strict=True)
    net.cuda().train()
    bb = net.backbone
    x = torch.randn(1, 3, 65, 97, generator=torch.Generator().manual_seed(0)).cuda()
    bb._logits(x).sum().backward()
    eng = bb._engine
    ops_e = [op for op in eng.plan.ops if op.kind == "conv" and op.expanded is not None]
    assert len(ops_e) == 1
    op = ops_e[0]
    before = [eng.packed(op, tr).clone() for tr in (False, True)]
    with torch.no_grad():
        for c in op.convs:
            c.weight.mul_(1.01)
            c.bias.mul_(1.01)
    bb._logits(x).sum().backward()                           # forward and backward: both layouts are rebuilt
    for tr, old in zip((False, True), before):
        got = eng._packs[(id(op), tr)][1]
        fresh = op.expanded.pack([c.weight.detach() for c in op.convs], tr)
        assert torch.equal(got, fresh) and not torch.equal(got, old), tr
    with torch.no_grad():
        _, saved = eng.forward(x, True)
    xin, got = saved["acts"][op.src], saved["acts"][op.dst]
    want = sum(F.conv2d(xin.double().cpu(), c.weight.detach().double().cpu(), c.bias.detach().double().cpu(), 1, c.padding,
                        c.dilation) for c in op.convs)
    xa = xin.double().cpu().abs()
    absref = sum(F.conv2d(xa, c.weight.detach().double().cpu().abs(), c.bias.detach().double().cpu().abs(), 1, c.padding,
                          c.dilation) for c in op.convs)
    assert got.shape == want.shape and _bound_ratio(got, want, absref, TAU["fp32"]) <= 1.0
