"""The workspace contract between the Python wrappers and the C ABI (include/dasac_hip.h: "`dasac_*_workspace(...)` returns the
bytes a call needs"), with tests/exact_workspace.py standing in for dasac_hip.lib.workspace.

(a) Every wrapper that asks for scratch runs three times -- on its size plus 1 MiB of slack, on exactly its size, and on exactly
    its size filled with zeros instead of 0xFF (a NaN pattern as fp32 and fp64) -- and must return the same bits each time, all
    finite, without touching the guards on either side of the buffer and without a DasacError: an undersized size function, a
    launcher whose own check wants more than its size function states, a kernel that writes past its slab or reads a slot it
    never wrote each break one of these.  The kernels are atomic-free with a fixed summation order (integer atomics in the
    per-class sums of dasac_ce_loss, which commute), so bit equality is the bar everywhere.
(b) dasac_ce_loss_bwd_low picks its path by ws_bytes: with the row buffer alone every block adds the B confidences itself and
    the one-wave kernel is excluded.  Both paths are held to the float64 yardstick of test_gpu_head_fp64.py.
    Measured on the MI355X (err_hip / (2 * err_aten + 1e-6); 0.5 = float32 ATen's own error; the test prints both):
        (2,19,9,13,65,97) m1   row buffer only 0.0623   full size 0.0623
        (2,32,3,5,17,33) m1    row buffer only 0.0629   full size 0.0629
    and for the (2,19,3,2,20,49) m1 row of (a), whose exact runs take the fallback and whose generous run does not: 0.0689 each.
(c) Every entry with a ws_bytes-like argument refuses a workspace one byte short with "workspace" in dasac_last_error(), before
    anything is launched (outputs and the workspace itself keep their fill), and accepts exactly the stated size."""
import numpy as np
import pytest
import torch

import conv_lattice as cl
from conv_lattice import SCHEDULE_CASE, TAIL_CASE
from exact_workspace import ExactWorkspace
from fp64_yardstick import _ratio, _report
from test_gpu_head_fp64 import GSCALE, _ce_inputs, _ce_reference

pytestmark = pytest.mark.gpu

RUNS = (("generous", 1 << 20, 0xFF), ("exact", 0, 0xFF), ("exact-zero", 0, 0x00))
SENTINEL = 0x5A


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.detach().contiguous().view(-1).view(torch.uint8)


def _three_runs(monkeypatch, run, what, same_as_generous=True):
    """run() -> list of output tensors, once per entry of RUNS under an ExactWorkspace; returns the three output lists."""
    from dasac_hip import lib as L
    outs = []
    for name, slack, poison in RUNS:
        ws = ExactWorkspace(slack, poison)
        monkeypatch.setattr(L, "workspace", ws)
        try:
            got = [t for t in run() if t is not None]
        except L.DasacError as exc:
            raise AssertionError("{}: the {} run was refused -- a launcher's check wants more than the size function states: {}".format(
                what, name, exc))
        n = ws.check()
        assert n >= 1, "{}: no workspace was requested".format(what)
        for i, t in enumerate(got):
            assert bool(torch.isfinite(t).all()), "{}: output {} of the {} run is not finite".format(what, i, name)
        outs.append(got)
        ws.requests.clear()
    monkeypatch.undo()
    first = 0 if same_as_generous else 1
    for (name, _, _), got in list(zip(RUNS, outs))[first + 1:]:
        assert len(got) == len(outs[first])
        for i, (a, b) in enumerate(zip(outs[first], got)):
            assert a.shape == b.shape and a.dtype == b.dtype
            assert torch.equal(_bits(a), _bits(b)), "{}: output {} differs between the {} and the {} run".format(what, i, RUNS[first][0], name)
    return outs


# ---- (a) the wrappers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W", [(3, 19, 25, 40), (1, 5, 1, 3)], ids=["3x19x1000", "1x5x3"])
def test_pseudo_labels(monkeypatch, B, C, H, W):
    from dasac_hip import ops
    g = _gen(B + C + H * W)
    probs = torch.softmax(3 * torch.randn(B, C, H, W, generator=g), 1).cuda()
    ignore = (torch.rand(B, H, W, generator=g) < 0.2).cuda()
    disc = (torch.rand(C, generator=g) * 0.5 + 0.5).cuda()
    _three_runs(monkeypatch, lambda: ops.pseudo_labels(probs, ignore, 0.75, 0.05, disc, want_idx=True), "pseudo_labels")


@pytest.mark.parametrize("case", [SCHEDULE_CASE, TAIL_CASE], ids=["stream_k", "split_k_tail"])
def test_conv_forward_and_dgrad(monkeypatch, case):
    from dasac_hip import ops
    lib = ops.L.load()
    name, cin, cout, br, stride, (N, H, W) = case
    spec = ops.ConvSpec(cin, cout, br, stride)
    if case is SCHEDULE_CASE:
        assert lib.dasac_conv_gemm_schedule(N, H, W, cout, spec.K) == 1 and lib.dasac_conv_gemm_tail_split(N, H, W, cout, spec.K) == 0
    else:
        assert lib.dasac_conv_gemm_tail_split(N, H, W, cout, spec.K) > 1
    print("dgrad of {}: schedule {}, tail_split {}".format(name, lib.dasac_conv_gemm_schedule(N, H, W, cin, spec.Kt),
                                                           lib.dasac_conv_gemm_tail_split(N, H, W, cin, spec.Kt)))
    o = cl.plain_operands(cin, cout, br, stride, (N, H, W))
    x, wd, dz = o["x"].cuda(), [w.cuda() for w in o["ws"]], o["dz"].cuda()
    shift, res = o["shift"].cuda(), o["res_out"].cuda()

    def run():
        return [ops.conv_forward(spec, x, wd), ops.conv_forward(spec, x, wd, None, shift, res, relu=True),
                ops.conv_dgrad(spec, dz, wd, (H, W))]
    _three_runs(monkeypatch, run, "conv_gemm " + name)         # (the bits themselves: test_gpu_conv_exact.py, on these operands)


@pytest.mark.parametrize("transposed", [False, True], ids=["forward", "transposed"])
@pytest.mark.parametrize("shape", [(2, 32, 128, 9, 7, 4), (1, 32, 128, 11, 13, 2)], ids=lambda s: "x".join(map(str, s)))
def test_winograd_conv(monkeypatch, shape, transposed):
    from dasac_hip import ops
    N, Cin, Cout, H, W, d = shape
    g = _gen(sum(shape))
    spec = ops.ConvSpec(Cin, Cout, [(3, 3, d, d)])
    assert ops.winograd_ok(spec, transposed)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5).cuda()
    C, M = (Cout, Cin) if transposed else (Cin, Cout)
    x = torch.randn(N, C, H, W, generator=g).cuda()
    shift = torch.randn(M, generator=g).cuda()
    u = ops.winograd_filter(spec, w, transposed)

    def run():
        out = torch.full((N, M, H, W), float("nan"), device="cuda")
        return [ops.winograd_conv(x, u, out, d, shift, relu=True)]
    _three_runs(monkeypatch, run, "winograd_conv")


def test_winograd_weight_gradient(monkeypatch):
    from dasac_hip import ops
    from test_gpu_winograd_wgrad import SHAPES
    N, Cin, Cout, H, W, d = SHAPES[2]
    g = _gen(7)
    spec = ops.ConvSpec(Cin, Cout, [(3, 3, d, d)])
    x, dz = torch.randn(N, Cin, H, W, generator=g).cuda(), torch.randn(N, Cout, H, W, generator=g).cuda()
    w, scale = torch.randn(Cout, Cin, 3, 3, generator=g).cuda(), (torch.rand(Cout, generator=g) + 0.5).cuda()
    rows = ops.dot_rows(spec)

    def run():
        dot, sums = (torch.full(s, float("nan"), device="cuda") for s in ((rows, Cout), (Cout,)))
        dw = ops.winograd_wgrad(spec, dz, x, w, scale=scale, dot=dot, sum_dz=sums, out=torch.full((Cout, Cin, 3, 3), float("nan"), device="cuda"))
        return [dw, dot, sums]
    _three_runs(monkeypatch, run, "winograd_wgrad")


# name, cin, cout, (kh, kw, dilation, padding), stride, (H, W) at batch 2
WGRAD_CASES = [("dilated3x3", 128, 80, (3, 3, 2, 2), 1, (29, 31)), ("strided1x1", 256, 128, (1, 1, 1, 0), 2, (33, 35)),
               ("stem7x7", 3, 64, (7, 7, 1, 3), 2, (65, 67)), ("raggedM", 64, 76, (1, 1, 1, 0), 1, (23, 27))]


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_conv_wgrad(monkeypatch, case, prec):
    from dasac_hip import ops
    name, cin, cout, br, stride, (H, W) = case
    spec = ops.ConvSpec(cin, cout, [br], stride)
    OH, OW = spec.out_hw(H, W)
    g = _gen(cin + cout + H)
    x, dz = torch.randn(2, cin, H, W, generator=g).cuda(), torch.randn(2, cout, OH, OW, generator=g).cuda()
    w = torch.randn(cout, cin, br[0], br[1], generator=g).cuda()
    monkeypatch.setattr(ops, "PRECISION", prec)

    def run():
        sums = torch.full((cout,), float("nan"), device="cuda")
        (dw,) = ops.conv_wgrad(spec, dz, x, [w], sum_dz=sums, outs=[torch.full_like(w, float("nan"))])
        return [dw, sums]
    _three_runs(monkeypatch, run, "conv_wgrad {} {}".format(name, prec))


def test_expanded_weight_gradient(monkeypatch):
    from dasac_hip import ops
    from test_gpu_expanded_conv import CASES, _inputs
    case = min((c for c in CASES if c[5] == "fp32"), key=lambda c: c[1] * c[2] * c[4][0] * c[4][1] * c[4][2] * sum(b[0] * b[1] for b in c[3]))
    name, cin, cout, branches, (N, H, W), _ = case
    print("expanded case", name)
    ex = ops.ExpandedConv(ops.ConvSpec(cin, cout, branches, 1))
    x, ws, _, dout, _ = _inputs(cin, cout, branches, (N, H, W))
    xd, wd = x.cuda(), [w.cuda() for w in ws]
    d = ex.scatter(dout.cuda())
    table = ops.conv_table(ex.spec1, H, W, False, xd.device)
    _three_runs(monkeypatch, lambda: ex.wgrad(d, xd, wd, table, outs=[torch.full_like(w, float("nan")) for w in wd]), "expanded wgrad")


def test_upsample_bwd(monkeypatch):
    from dasac_hip import ops
    g = _gen(3)
    grad_up = torch.randn(2, 19, 33, 49, generator=g).cuda()
    gs = torch.tensor([GSCALE]).cuda()
    _three_runs(monkeypatch, lambda: [ops.upsample_bwd(grad_up, (5, 7), gs)], "upsample_bwd")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", [(2, 19, 3, 7), (3, 7, 5, 7)], ids=lambda s: "x".join(map(str, s)))
def test_ce_loss(monkeypatch, shape, mode):
    from dasac_hip import ops
    x, y, cw, conf = _ce_inputs(*shape, mode, 3.0, seed=sum(shape) + mode)
    xd, yd, cwd, cd, gs = x.cuda(), y.cuda(), cw.cuda(), None if conf is None else conf.cuda(), torch.tensor([GSCALE]).cuda()
    outs = _three_runs(monkeypatch, lambda: ops.ce_loss(xd, yd, cwd, cd, want_grad=True, want_per_class=True, gscale=gs), "ce_loss")
    assert len(outs[0]) == 3


LOW = [((2, 19, 9, 13, 65, 97), 1), ((3, 19, 5, 7, 33, 49), 0), ((1, 7, 4, 6, 8, 12), 1), ((2, 19, 3, 2, 20, 49), 1)]


def _low_inputs(shape, mode):
    """The inputs of test_gpu_head_fp64's low-resolution gradient test and its two CPU references."""
    from dasac_hip import ops
    B, C, h, w, H, W = shape
    _, y, cw, conf = _ce_inputs(B, C, H, W, mode, 3.0, seed=sum(shape))
    low = torch.randn(B, C, h, w, generator=_gen(sum(shape) + 1)) * 3
    up, _, _ = ops.upsample_softmax(low.cuda(), (H, W))
    _, g64, _ = _ce_reference(low, y, cw, conf, torch.float64, size=(H, W))
    _, g32, _ = _ce_reference(low, y, cw, conf, torch.float32, size=(H, W))
    return up, y.cuda(), cw.cuda(), None if conf is None else conf.cuda(), torch.tensor([GSCALE]).cuda(), g64, g32


@pytest.mark.parametrize("shape,mode", LOW, ids=["{}_m{}".format("x".join(map(str, s)), m) for s, m in LOW])
def test_ce_loss_bwd_low(monkeypatch, shape, mode):
    """(2,19,3,2,20,49) m1: the up-factor is above 16, so the size function's tail has no room for the confidence sums: the exact
    runs take the fallback, the generous one the precomputed sums -- both documented, not compared bit for bit; each is held to
    the float64 yardstick instead."""
    from dasac_hip import lib as L
    from dasac_hip import ops
    B, C, h, w, H, W = shape
    up, y, cw, conf, gs, g64, g32 = _low_inputs(shape, mode)
    need = L.load().dasac_ce_loss_bwd_low_workspace(B, C, H, w)
    tmp = (B * C * H * w * 4 + 255) // 256 * 256
    tail_fits = need >= tmp + H * W * 4
    assert tail_fits == (shape != (2, 19, 3, 2, 20, 49))
    outs = _three_runs(monkeypatch, lambda: [ops.ce_loss_bwd_low(up, y, (h, w), cw, conf, gscale=gs)], "ce_loss_bwd_low", same_as_generous=tail_fits)
    _report("ce_loss_bwd_low", (shape, mode), {name: _ratio(got[0], g64, g32) for (name, _, _), got in zip(RUNS, outs)})


@pytest.mark.parametrize("N,C,HW", [(3, 5, 77), (2, 64, 4099)])
def test_bn_statistics_and_fused_backward(monkeypatch, N, C, HW):
    from dasac_hip import ops
    g = _gen(N + C + HW)
    z, dy = (torch.randn(N, C, HW, generator=g) * 2 + 0.5).cuda(), torch.randn(N, C, HW, generator=g).cuda()
    gamma, beta = (torch.rand(C, generator=g) + 0.5), torch.randn(C, generator=g)

    def run():
        bn = torch.nn.BatchNorm2d(C)
        with torch.no_grad():
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
        bn.cuda()
        y, stats = ops.bn_train_forward(z, bn, relu=True)
        dz, dg, db = ops.bn_train_backward(dy, z, stats, bn.weight.detach())
        return [ops.class_sums(z), y, stats[0], stats[1], bn.running_mean, bn.running_var, dz, dg, db]
    _three_runs(monkeypatch, run, "bn")


def test_boundary_counts(monkeypatch):
    from dasac_hip import ops
    from test_gpu_boundary import _case
    scores, labels, gt = _case(2, 19, 9, 13, 5)
    ds, dg = [torch.from_numpy(scores[0]).cuda()], torch.from_numpy(gt).cuda()
    dl = [torch.from_numpy(labels).cuda()]
    outs = _three_runs(monkeypatch, lambda: [ops.boundary_counts(ds, dl, dg, radius=3)], "boundary_counts")
    assert int(outs[0][0].sum()) > 0


def test_activation_stats_plan(monkeypatch):
    from dasac_hip import ops
    x = torch.randn(2, 3, 2, generator=_gen(1)).cuda()
    plan = ops.ActivationStatsPlan([(3, 2)], 2)
    _three_runs(monkeypatch, lambda: [plan.run([x])], "activation_stats")


@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_fused_optimizer_step(monkeypatch, kind):
    from dasac_hip.optim import FusedAdam, FusedSGD
    from test_gpu_fused_optim import SHAPES, make_params, three_groups
    grads = [torch.randn(s, generator=_gen(50 + i)).cuda() for i, s in enumerate(SHAPES)]
    kw = dict(max_grad_norm=1.0, track_tensor_stats=True, skip_nonfinite=True)

    def run():
        _, ps = make_params(11)
        opt = FusedAdam(three_groups(ps), betas=(0.9, 0.99), **kw) if kind == "adam" else FusedSGD(three_groups(ps), momentum=0.9, nesterov=True, **kw)
        for p, gr in zip(ps, grads):
            p.grad = gr.clone()
        opt.step()
        state = [v for p in ps for k, v in sorted(opt.state[p].items()) if torch.is_tensor(v) and v.is_cuda]
        assert len(state) >= len(ps) and int(opt.skipped_steps) == 0
        return [p.detach() for p in ps] + state + [opt.tensor_stats.clone(), opt.grad_norm.clone()]
    outs = _three_runs(monkeypatch, run, "fused " + kind)
    assert float(outs[0][-1]) > 1.0                                     # the clip was active


def _view_inputs(H, W, L, seed):
    gen = np.random.RandomState(seed)
    imgs = gen.randint(0, 256, (L, 3, H, W)).astype(np.uint8)
    gt = gen.randint(0, 19, (L, H, W)).astype(np.int64)
    gt[:, :, : W // 8] = -1
    photo = [dict(blur=1.3, jitter=([0, 1, 2, 3], [1.2, 0.8, 1.1, 0.05]), grey=False), dict(blur=None, jitter=([1, 3, 0, 2], [1.4, 0.6, 1.0, 0.1]), grey=False),
             dict(blur=2.0, jitter=None, grey=True), dict(blur=None, jitter=None, grey=False)][:L]
    return torch.from_numpy(imgs).cuda(), torch.from_numpy(gt).cuda(), photo


def test_target_views_augment(monkeypatch):
    import views
    H, W, L = 37, 53, 4
    u8, gt, photo = _view_inputs(H, W, L, 2)
    tv = views.TargetViews((H, W), L)
    outs = _three_runs(monkeypatch, lambda: list(tv.augment(u8, gt, photo, want_u8=True)), "TargetViews.augment")
    assert not torch.equal(outs[0][1], u8)


def test_crop_photometric_in_place(monkeypatch):
    import crops
    H, W = 37, 53
    u8, _, photo = _view_inputs(H, W, 1, 3)
    lab = torch.zeros(H * W, dtype=torch.uint8, device="cuda")

    def run():
        src = crops._Packed(u8.reshape(-1).clone(), lab, [(0, 0)], [(H, W)], [(1, H * W)])
        crops.photometric_in_place(src, 0, True, photo[0]["jitter"])
        return [src.img]
    outs = _three_runs(monkeypatch, run, "crops.photometric_in_place")
    assert not torch.equal(outs[0][0], u8.reshape(-1))


# ---- (b) the fallback of dasac_ce_loss_bwd_low, by argument ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 19, 9, 13, 65, 97), (2, 32, 3, 5, 17, 33)], ids=lambda s: "x".join(map(str, s)))
def test_ce_loss_bwd_low_with_the_row_buffer_alone(shape):
    from dasac_hip import lib as L
    lib = L.load()
    B, C, h, w, H, W = shape
    up, y, cw, conf, gs, g64, g32 = _low_inputs(shape, 1)
    rows = (B * C * H * w * 4 + 255) // 256 * 256
    full = lib.dasac_ce_loss_bwd_low_workspace(B, C, H, w)
    assert full >= rows + H * W * 4                                     # the full size does hold the confidence sums
    ratios = {}
    for name, nbytes in (("row buffer only", rows), ("full size", full)):
        guard = ExactWorkspace(0, 0xFF)
        ws = guard(nbytes, up.device)
        out = torch.full((B, C, h, w), float("nan"), device="cuda")
        rc = lib.dasac_ce_loss_bwd_low(up.data_ptr(), y.data_ptr(), cw.data_ptr(), conf.data_ptr(), B, C, H, W, h, w, 1, gs.data_ptr(),
                                       out.data_ptr(), ws.data_ptr(), ws.numel(), L.stream_ptr())
        assert rc == 0, lib.dasac_last_error()
        assert guard.check() == 1
        ratios[name] = _ratio(out, g64, g32)
    _report("ce_loss_bwd_low by ws_bytes", shape, ratios)


# ---- (c) one byte short ----------------------------------------------------------------------------------------------------------
def _filled(shape, dtype=torch.float32):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(-1).view(torch.uint8).fill_(SENTINEL)
    return t


def _refuses_one_byte_short(entry, need, call, outputs, owner=None, poison=0xFF):
    """call(ws_ptr, ws_bytes) -> return code.  need - 1: refused, nothing launched; need: accepted, guards intact."""
    from dasac_hip import lib as L
    lib = L.load()
    assert need > 0, entry
    guard = ExactWorkspace(0, poison)
    ws = guard(need, torch.device("cuda", torch.cuda.current_device()), owner=owner)
    fill = int(ws[0])
    rc = call(ws.data_ptr(), need - 1)
    err = lib.dasac_last_error()
    torch.cuda.synchronize()
    assert rc != 0 and b"workspace" in err, (entry, rc, err)
    for i, t in enumerate(outputs):
        assert bool((_bits(t) == SENTINEL).all()), "{}: output {} was written by the refused call".format(entry, i)
    assert bool((ws == fill).all()), "{}: the workspace was written by the refused call".format(entry)
    assert guard.check() == 1
    rc = call(ws.data_ptr(), need)
    assert rc == 0, (entry, lib.dasac_last_error())
    assert guard.check() == 1


def test_ce_entries_refuse_one_byte_short():
    from dasac_hip import lib as L
    lib, s = L.load(), L.stream_ptr()
    B, C, H, W = 2, 19, 3, 7
    x, y, cw, conf = (t.cuda() for t in _ce_inputs(B, C, H, W, 1, 3.0, seed=1))
    gs = torch.tensor([GSCALE]).cuda()
    loss, dl, pc = _filled((1,)), _filled((B, C, H, W)), _filled((C,))
    _refuses_one_byte_short("dasac_ce_loss", lib.dasac_ce_loss_workspace(B, C, H * W), lambda p, n: lib.dasac_ce_loss(
        x.data_ptr(), y.data_ptr(), cw.data_ptr(), conf.data_ptr(), B, C, H * W, 1, gs.data_ptr(), loss.data_ptr(), dl.data_ptr(), pc.data_ptr(),
        p, n, s), [loss, dl, pc])
    h, w = 2, 3
    out = _filled((B, C, h, w))
    rows = (B * C * H * w * 4 + 255) // 256 * 256
    _refuses_one_byte_short("dasac_ce_loss_bwd_low", rows, lambda p, n: lib.dasac_ce_loss_bwd_low(
        x.data_ptr(), y.data_ptr(), cw.data_ptr(), conf.data_ptr(), B, C, H, W, h, w, 1, gs.data_ptr(), out.data_ptr(), p, n, s), [out])


def test_bn_entries_refuse_one_byte_short():
    from dasac_hip import lib as L
    lib, s = L.load(), L.stream_ptr()
    N, C, HW = 2, 5, 4099
    g = _gen(4)
    z, dy = torch.randn(N, C, HW, generator=g).cuda(), torch.randn(N, C, HW, generator=g).cuda()
    mean, invstd, gamma = torch.randn(C, generator=g).cuda(), (torch.rand(C, generator=g) + 0.5).cuda(), (torch.rand(C, generator=g) + 0.5).cuda()
    need = lib.dasac_bn_stats_workspace(N, C, HW)
    assert need == N * C * 2 * 2 * 8
    sums = _filled((2 * C,), torch.float64)
    _refuses_one_byte_short("dasac_bn_stats", need, lambda p, n: lib.dasac_bn_stats(z.data_ptr(), N, C, HW, sums.data_ptr(), p, n, s), [sums])
    sums, dg, db = _filled((2 * C,), torch.float64), _filled((C,)), _filled((C,))
    _refuses_one_byte_short("dasac_bn_bwd_reduce", need, lambda p, n: lib.dasac_bn_bwd_reduce(
        dy.data_ptr(), z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), N, C, HW, sums.data_ptr(), dg.data_ptr(), db.data_ptr(), p, n, s), [sums, dg, db])
    dz, dg, db = _filled((N, C, HW)), _filled((C,)), _filled((C,))
    _refuses_one_byte_short("dasac_bn_bwd_fused", need, lambda p, n: lib.dasac_bn_bwd_fused(
        dy.data_ptr(), z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), float(N * HW), N, C, HW, dz.data_ptr(), dg.data_ptr(),
        db.data_ptr(), p, n, s), [dz, dg, db])


def test_conv_gemm_refuses_one_byte_short_on_its_stream_k_case():
    from dasac_hip import ops
    L = ops.L
    lib, s = L.load(), L.stream_ptr()
    name, cin, cout, br, stride, (N, H, W) = SCHEDULE_CASE
    spec = ops.ConvSpec(cin, cout, br, stride)
    assert lib.dasac_conv_gemm_schedule(N, H, W, cout, spec.K) == 1
    o = cl.plain_operands(cin, cout, br, stride, (N, H, W))
    order = ops.gemm_order(spec, False)
    x = o["x"].cuda()
    table = ops.conv_table(spec, H, W, False, x.device, order)
    packed = ops.conv_pack(spec, [w.cuda() for w in o["ws"]], False, None, order=order)
    out = _filled((N, cout, H, W))
    _refuses_one_byte_short("dasac_conv_gemm", lib.dasac_conv_gemm_workspace(), lambda p, n: lib.dasac_conv_gemm(
        x.data_ptr(), packed.data_ptr(), table.data_ptr(), out.data_ptr(), N, cin, H, W, H, W, 1, cout, spec.K, H, W, 1, None, None, None, None,
        None, 0, 0, 0, 0, p, n, s), [out], owner="conv_gemm")
    assert torch.equal(out.cpu(), cl.f32(cl.conv_fwd(o["x"], o["ws"], br, stride)))


# 1x1 128 -> 256 on 40 x 40 at batch 2: the size function, which does not know Cx, takes the larger split count of both k-tile
# widths (12 with 64-row tiles, 8 with the 128-row tiles this Cx runs on) -- a launcher that checks its own 8 slabs only would
# accept the size function's result minus one byte
WIDE_1X1 = ("wide1x1", 128, 256, (1, 1, 1, 0), 1, (40, 40))


@pytest.mark.parametrize("case", [WGRAD_CASES[0], WGRAD_CASES[3], WIDE_1X1], ids=[WGRAD_CASES[0][0], WGRAD_CASES[3][0], WIDE_1X1[0]])
def test_conv_wgrad_entries_refuse_one_byte_short(case):
    from dasac_hip import ops
    L = ops.L
    lib, s = L.load(), L.stream_ptr()
    name, cin, cout, br, stride, (H, W) = case
    spec = ops.ConvSpec(cin, cout, [br], stride)
    OH, OW = spec.out_hw(H, W)
    g = _gen(9)
    x, dz = torch.randn(2, cin, H, W, generator=g).cuda(), torch.randn(2, cout, OH, OW, generator=g).cuda()
    table = ops.conv_table(spec, H, W, False, x.device)
    need = lib.dasac_conv_wgrad_workspace(2, OH, OW, cout, spec.K)
    for entry in ("dasac_conv_wgrad", "dasac_conv_wgrad_x3"):
        fn = getattr(lib, entry)
        _refuses_one_byte_short(entry, need, lambda p, n: fn(dz.data_ptr(), x.data_ptr(), table.data_ptr(), 2, cin, H, W, OH, OW, stride, cout,
                                                             spec.K, p, n, s), [])


def test_batched_wgrad_and_winograd_entries_refuse_one_byte_short():
    from dasac_hip import lib as L
    lib, s = L.load(), L.stream_ptr()
    Nb, C, M, H, W, d = 3, 128, 128, 13, 10, 4
    T = lib.dasac_winograd_tiles(Nb, H, W, d)
    assert T > 0 and T % 4 == 0
    g = _gen(6)
    x, dz = torch.randn(Nb, C, H, W, generator=g).cuda(), torch.randn(Nb, M, H, W, generator=g).cuda()
    w, scale = torch.randn(M, C, 3, 3, generator=g).cuda(), (torch.rand(M, generator=g) + 0.5).cuda()
    a, b = torch.randn(16, M, T, generator=g).cuda(), torch.randn(16, C, T, generator=g).cuda()
    need = lib.dasac_conv_wgrad_batched_workspace(16, M, C, T)
    _refuses_one_byte_short("dasac_conv_wgrad_batched", need, lambda p, n: lib.dasac_conv_wgrad_batched(
        a.data_ptr(), b.data_ptr(), 16, M, C, T, M * T, C * T, 5, p, n, s), [])
    dw, sums = _filled((M, C, 3, 3)), _filled((M,))
    _refuses_one_byte_short("dasac_winograd_wgrad_finish", need, lambda p, n: lib.dasac_winograd_wgrad_finish(
        p, n, M, C, T, w.data_ptr(), scale.data_ptr(), dw.data_ptr(), None, sums.data_ptr(), s), [dw, sums], poison=0x00)
    _refuses_one_byte_short("dasac_winograd_input", 64 * C * T, lambda p, n: lib.dasac_winograd_input(x.data_ptr(), Nb, C, H, W, d, p, n, s), [])
    _refuses_one_byte_short("dasac_winograd_grad_input", 64 * M * T, lambda p, n: lib.dasac_winograd_grad_input(dz.data_ptr(), Nb, M, H, W, d, p, n, s), [])
    out = _filled((Nb, M, H, W))
    _refuses_one_byte_short("dasac_winograd_output", 64 * M * T, lambda p, n: lib.dasac_winograd_output(
        p, n, Nb, M, H, W, d, None, 0, None, None, out.data_ptr(), s), [out], poison=0x00)


def test_view_photometric_refuses_one_byte_short():
    import views
    from dasac_hip import lib as L
    lib, s = L.load(), L.stream_ptr()
    H, W, nv = 37, 53, 4
    u8, gt, photo = _view_inputs(H, W, nv, 2)
    params = np.ascontiguousarray(views.photometric_params(photo))
    mean, std = np.asarray(views.MEAN, dtype=np.float32), np.asarray(views.STD, dtype=np.float32)
    frames, out = _filled((nv, 3, H, W)), _filled((nv, 3, H, W), torch.uint8)
    _refuses_one_byte_short("dasac_view_photometric", lib.dasac_view_photometric_workspace(H, W, nv), lambda p, n: lib.dasac_view_photometric(
        u8.data_ptr(), gt.data_ptr(), H, W, nv, params.ctypes.data, mean.ctypes.data, std.ctypes.data, -1, frames.data_ptr(), out.data_ptr(), p, n,
        s), [frames, out])
