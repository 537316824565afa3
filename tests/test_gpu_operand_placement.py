"""Every op on guarded operands at every alignment phase (tests/guarded_operands.py).

Two properties of the OPERANDS that no per-family test checks: nothing is written outside an output, and the result does not
depend on where an operand lies.  Each case is a small function `case(a)` of an Arena `a` that builds its inputs on the host from
a fixed seed, puts them on the device with `a.place`, calls wrappers whose `torch` is `a.torch`, and returns its output tensors.
`_sweep` runs it
  * twice on the plain arena (ordinary allocations, another pre-fill byte): bit-equal, determinism being the project's contract;
  * once per base phase on a guarded arena (fp32 / int32 operands: 4 phases; byte pipelines: all 16): `arena.check()` -- no guard
    byte changed, no input changed -- then every output bit-equal to the plain run's.
Correctness against float64 is the job of each family's own file; here the plain run is the comparand.

Operands that may be REFUSED off their alignment (DASAC_EINVAL before any launch) -- the closed list, each with the sentence of
include/dasac_hip.h that grants it; no activation, weight, gradient, label, image or bit mask is on it, and the sweep below runs
none of them shifted (an arena keeps int32 [n, k] descriptor tables on a 256-byte boundary):
  * workspaces: "`dasac_*_workspace(...)` returns the bytes a call needs (16-byte aligned pointer)";
  * control blocks and counters: "ctl must be 16-byte aligned" (dasac_grad_norm, the _ctl updates, dasac_tensor_stats);
  * dasac_conv_gemm_batched strides: "per-batch strides must be multiples of 4 elements";
  * conv gather tables: "`table` must be 16-byte aligned here and in every entry that takes it";
  * dasac_ema_update: "`pairs`, `chunks` and `sq` must be 8-byte aligned";
  * optimiser row tables and chunk lists: "`tensors` and `chunks` must be 8-byte aligned, here and in ...";
  * dasac_bn_fold_multi / dasac_conv_pack_multi: "`jobs` and `chunks` must be 8-byte aligned".
The misaligned-descriptor tests at the end pass each such table one int32 off through the C ABI."""
import ctypes
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from guarded_operands import Arena, bits_equal

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A


def _modules():
    import crops
    import views
    import visualise
    from dasac_hip import ops, optim
    return ops, optim, crops, views, visualise


def _flatten(outs):
    flat = []
    for o in outs if isinstance(outs, (tuple, list)) else (outs,):
        if isinstance(o, (tuple, list)):
            flat += _flatten(o)
        elif o is not None and not torch.is_tensor(o):
            flat.append(o.words)                 # ops.ReluBits
        else:
            flat.append(o)
    return flat


def _run(monkeypatch, case, arena):
    from dasac_hip import lib as L
    with monkeypatch.context() as m:
        for mod in _modules():
            m.setattr(mod, "torch", arena.torch)
        try:
            outs = _flatten(case(arena))
        except L.DasacError as exc:
            raise AssertionError("phase {}: an entry refused an operand for where it lies: {}".format(arena.phase, exc))
    arena.check()
    for i, t in enumerate(outs):                     # an output allocated behind the stand-in's back would be checked by no guard
        assert t is None or arena.owns(t), "output {} {} {} was not allocated by the arena".format(i, t.dtype, tuple(t.shape))
    return outs


def _sweep(monkeypatch, case, phases=range(4)):
    plain, again = _run(monkeypatch, case, Arena(None)), _run(monkeypatch, case, Arena(None))
    assert len(plain) == len(again) and any(t is not None for t in plain)
    for i, (a, b) in enumerate(zip(plain, again)):
        assert bits_equal(a, b), "output {}: two plain runs differ".format(i)
    for phase in phases:
        got = _run(monkeypatch, case, Arena(phase))
        assert len(got) == len(plain)
        for i, (a, b) in enumerate(zip(plain, got)):
            assert bits_equal(a, b), "output {} at base phase {} differs from the plain run{}".format(i, phase, _where(a, b))


def _where(a, b):
    if a is None or b is None or a.shape != b.shape or a.dtype != b.dtype:
        return ""
    bad = (a.reshape(-1).view(torch.uint8) != b.reshape(-1).view(torch.uint8)).nonzero()
    return ": {} of {} bytes, first at byte {}".format(bad.numel(), a.numel() * a.element_size(), int(bad[0]))


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- head --------------------------------------------------------------------------------------------------------------------
# low 3x4 -> high 9x13 (W = 1 mod 4, HW = 117: planes at every dword phase, a ragged last quad); low 2x3 -> high 8x12 (whole quads)
HEAD_SHAPES = [((3, 4), (9, 13)), ((2, 3), (8, 12))]
HEAD = [(C, low, high) for C in (19, 5) for low, high in HEAD_SHAPES]
HEAD_IDS = ["C{}_{}x{}".format(C, *high) for C, _, high in HEAD]


@pytest.mark.parametrize("C,low,high", HEAD, ids=HEAD_IDS)
def test_head_upsampling_and_inference(monkeypatch, C, low, high):
    from dasac_hip import ops
    B, (h, w), (H, W) = 2, low, high

    def case(a):
        g = _gen(C + H)
        logits = a.place(3 * torch.randn(B, C, h, w, generator=g))
        ignore = a.place(torch.rand(B, H, W, generator=g) < 0.25)
        grad_up = a.place(torch.randn(B, C, H, W, generator=g))
        gs = a.place(torch.tensor([0.37]))
        lut = a.place(torch.arange(C, dtype=torch.uint8) + 7)
        image = a.place(torch.randn(B, 3, H, W, generator=g))
        src2 = a.place(3 * torch.randn(2 * B, C, h + 1, w + 2, generator=g))       # a 2B batch: its second half is the mirrored source
        outs = list(ops.upsample_softmax(logits, (H, W), ignore, want_up=True, want_probs=True, want_sums=True))
        outs.append(ops.upsample_softmax(logits, (H, W))[0])
        outs.append(ops.upsample_bwd(grad_up, (h, w), gs))
        outs += list(ops.infer_labels(logits, (H, W), lut, want_conf=True))
        outs.append(ops.image_pyramid(image, (h + 2, w + 3), flip=True))
        for mode in ("mean", "max"):
            outs += list(ops.infer_fuse([logits, src2[:B], src2[B:]], [False, False, True], (H, W), mode, lut, want_conf=True, want_probs=True))
        return outs
    _sweep(monkeypatch, case)


@pytest.mark.parametrize("C,low,high", HEAD, ids=HEAD_IDS)
def test_head_losses_and_pseudo_labels(monkeypatch, C, low, high):
    from dasac_hip import ops
    from test_gpu_head_fp64 import _ce_inputs
    B, (h, w), (H, W) = 2, low, high

    def case(a):
        g = _gen(C + W)
        x, y, cw, conf = _ce_inputs(B, C, H, W, 1, 3.0, seed=C + H)
        x, y, cw, conf, gs = a.place(x), a.place(y), a.place(cw), a.place(conf), a.place(torch.tensor([0.37]))
        probs = a.place(torch.softmax(3 * torch.randn(B, C, H, W, generator=g), 1))
        ignore = a.place(torch.rand(B, H, W, generator=g) < 0.2)
        disc = a.place(torch.rand(C, generator=g) * 0.5 + 0.5)
        outs = []
        for c in (None, conf):
            outs += list(ops.ce_loss(x, y, cw, c, want_grad=True, want_per_class=True, gscale=gs))
            outs.append(ops.ce_loss_bwd_low(x, y, (h, w), cw, c, gscale=gs))
        outs += list(ops.pseudo_labels(probs, ignore, 0.75, 0.05, disc, want_idx=True))
        outs.append(ops.class_sums(probs))
        return outs
    _sweep(monkeypatch, case)


@pytest.mark.parametrize("C", [19, 5])
@pytest.mark.parametrize("H,W", [(7, 9), (4, 8)])
def test_head_warps(monkeypatch, C, H, W):
    from dasac_hip import ops
    from test_gpu_head_fp64 import _inverse, _random_thetas
    N, T = 2, 2

    def case(a):
        g = _gen(C + H * W)
        probs = a.place(torch.softmax(2 * torch.randn(N * T, C, H, W, generator=g), 1))
        th = _random_thetas(N * T, g)
        theta, theta_inv = a.place(th), a.place(_inverse(th))
        outs = [ops.warp_affine(probs, theta)]
        for mode in ("avg_pool", "minentropy_pool"):
            pooled, mask, aligned = ops.warp_pool(probs, theta, theta_inv, T, mode, want_aligned=True)
            outs += [pooled, mask, aligned, ops.warp_back(pooled, mask, theta_inv, T)]
        outs += list(ops.warp_pool(probs, None, None, T, "avg_pool"))
        return outs
    _sweep(monkeypatch, case)


# ---- pointwise / BN / pool -----------------------------------------------------------------------------------------------------
def _bn(a, C, g):
    """What ops.bn_train_forward reads of an nn.BatchNorm2d, on placed tensors; the running statistics are written."""
    return NS(weight=a.place(torch.rand(C, generator=g) + 0.5), bias=a.place(torch.randn(C, generator=g)),
              running_mean=a.place(torch.randn(C, generator=g), inplace=True), running_var=a.place(torch.rand(C, generator=g) + 0.5, inplace=True),
              num_batches_tracked=a.place(torch.tensor(3), inplace=True), momentum=0.1, eps=1e-5, track_running_stats=True)


@pytest.mark.parametrize("H,W", [(7, 9), (4, 8), (1, 1)])
def test_pointwise_and_batch_norm(monkeypatch, H, W):
    from dasac_hip import ops
    N, C = 2, 5

    def case(a):
        g = _gen(H * W)
        z, res, dy = (a.place(torch.randn(N, C, H, W, generator=g)) for _ in range(3))
        bn = _bn(a, C, g)
        y, stats = ops.bn_train_forward(z, bn, res=res, relu=True)              # dasac_bn_stats, finalize, dasac_bn_apply with res and relu
        dz, dg, db = ops.bn_train_backward(ops.relu_mask(dy, y), z, stats, bn.weight)
        outs = [y, stats[0], stats[1], bn.running_mean, bn.running_var, bn.num_batches_tracked, dz, dg, db]
        outs.append(ops.scale_planes(z, a.place(torch.rand(N, C, generator=g))))
        outs += [ops.add(z, res), ops.relu_mask(dy, z), ops.channel_sums(z)]
        outs += list(ops.bn_fold(bn.weight, bn.bias, a.place(torch.randn(C, generator=g)), a.place(torch.rand(C, generator=g) + 0.1), 1e-5,
                                 a.place(torch.randn(C, generator=g))))
        dot, sum_dz = a.place(torch.randn(3, C, generator=g)), a.place(torch.randn(C, generator=g))
        outs += list(ops.bn_param_grads(dot, sum_dz, stats[0], stats[1], a.place(torch.rand(C, generator=g)), a.place(torch.randn(C, generator=g)),
                                        want_bias=True))
        labels = torch.randint(0, 19, (N, H, W), generator=g)
        labels[torch.rand(N, H, W, generator=g) < 0.3] = -1
        labels = a.place(labels, inplace=True)                                   # rewritten in place (sac.py:337-338)
        outs += [ops.label_pad_mask(labels), labels]
        torch.manual_seed(11)
        outs.append(ops.dropout_planes(N, C * H * W, 0.3, z.device))
        return outs
    _sweep(monkeypatch, case)


POOLS = [(3, 2, 1), (2, 2, 0), (3, 1, 1), (5, 3, 2)]


@pytest.mark.parametrize("k,s,p", POOLS, ids=["k{}s{}p{}".format(*c) for c in POOLS])
@pytest.mark.parametrize("H,W", [(9, 13), (8, 12)])
def test_max_pool(monkeypatch, H, W, k, s, p):
    from dasac_hip import ops
    N, C = 2, 5

    def case(a):
        g = _gen(H + k)
        x = a.place(torch.randn(N, C, H, W, generator=g))
        y, arg = ops.maxpool_fwd(x, k, s, p, True)
        dy = a.place(torch.randn(y.shape, generator=g))
        return [y, arg] + [ops.maxpool_bwd(dy, y, arg, (H, W), k, s, p, relu_mask) for relu_mask in (False, True)]
    _sweep(monkeypatch, case)


# ---- convolutions --------------------------------------------------------------------------------------------------------------
CONV_NAMES = ["1x1_quad_ragged", "1x1_s2", "3x3_qtap_w5_d3", "3x3_d2_fast_ragged", "3x3_d1_c19", "7x7_s2_stem"]


def _conv_case(name):
    from test_gpu_conv import CASES
    return next(c for c in CASES if c[0] == name)


def _conv_operands(a, case, seed=0):
    from test_gpu_conv import _make
    from dasac_hip import ops
    _, cin, cout, br, stride, (N, H, W) = case
    spec = ops.ConvSpec(cin, cout, br, stride)
    OH, OW = spec.out_hw(H, W)
    x, ws = _make(case, seed)
    g = _gen(seed + 1)
    o = NS(spec=spec, N=N, H=H, W=W, OH=OH, OW=OW, x=a.place(x), ws=[a.place(w) for w in ws])
    o.dz = a.place(torch.randn(N, cout, OH, OW, generator=g))
    o.scale, o.shift = a.place(torch.rand(cout, generator=g) + 0.5), a.place(torch.randn(cout, generator=g))
    o.res_out = a.place(torch.randn(N, cout, OH, OW, generator=g))
    o.res_in, o.act_in = a.place(torch.randn(N, cin, H, W, generator=g)), a.place(torch.randn(N, cin, H, W, generator=g))
    return o


@pytest.mark.parametrize("name", CONV_NAMES)
def test_conv_forward_dgrad_wgrad(monkeypatch, name):
    from dasac_hip import ops
    case = _conv_case(name)
    cin, cout, stride = case[1], case[2], case[4]

    def case_fn(a):
        o = _conv_operands(a, case)
        spec = o.spec
        outs = [ops.conv_forward(spec, o.x, o.ws), ops.conv_forward(spec, o.x, o.ws, o.scale, o.shift, o.res_out, relu=True)]
        bits = None
        if ops.bits_ok(cout, cin):                                           # the ReLU pattern as bits, then consumed by a data gradient
            order = ops.gemm_order(spec, False)
            y = a.torch.empty((o.N, cout, o.OH, o.OW), dtype=torch.float32, device=o.x.device)
            bits = ops.ReluBits(o.N, cout, o.OH, o.OW, o.x.device)
            ops.conv_gemm(o.x, ops.conv_pack(spec, o.ws, False, o.scale, order=order), ops.conv_table(spec, o.H, o.W, False, o.x.device, order),
                          y, (o.OH, o.OW), stride, cout, spec.K, 1, o.shift, o.res_out, None, True, bits_out=bits)
            outs += [y, bits]
        if name != "7x7_s2_stem":                                            # (no data gradient of the strided stem, as in test_gpu_conv.py)
            if stride == 1:
                outs.append(ops.conv_dgrad(spec, o.dz, o.ws, (o.H, o.W), scale=o.scale, res=o.res_in, mask=o.act_in))
            else:                                                            # strided 1x1: accumulates IN PLACE on res
                res = a.place(torch.randn(o.N, cin, o.H, o.W, generator=_gen(9)), inplace=True)
                outs.append(ops.conv_dgrad(spec, o.dz, o.ws, (o.H, o.W), scale=o.scale, res=res, mask=o.act_in))
                outs.append(ops.conv_dgrad(spec, o.dz, o.ws, (o.H, o.W)))
            if stride == 1 and ops.bits_ok(cin, cout):
                # the pattern of a [N, cin, H, W] activation, recorded by an identity-shaped producer: here simply random words
                mb = ops.ReluBits(o.N, cin, o.H, o.W, o.x.device)
                mb.words = a.place(torch.randint(-2 ** 31, 2 ** 31, (mb.words.numel(),), generator=_gen(5)).to(torch.int32))
                outs.append(ops.conv_dgrad(spec, o.dz, o.ws, (o.H, o.W), scale=o.scale, res=o.res_in, mask=mb))
        dot = a.torch.empty((ops.dot_rows(spec), cout), dtype=torch.float32, device=o.x.device)
        sum_dz = a.torch.empty(cout, dtype=torch.float32, device=o.x.device)
        dws = [a.torch.empty_like(w) for w in o.ws]
        got = ops.conv_wgrad(spec, o.dz, o.x, o.ws, scale=o.scale, dot=dot, sum_dz=sum_dz, outs=dws)
        assert all(x_ is y_ for x_, y_ in zip(got, dws))
        return outs + dws + [dot, sum_dz] + ops.conv_wgrad(spec, o.dz, o.x, o.ws)
    _sweep(monkeypatch, case_fn)


def test_conv_statistics_epilogue_feeds_batch_norm(monkeypatch):
    """conv_gemm(stats=...) on 1x1_quad_ragged, and train-mode BN forward / backward from those tile statistics (the second
    statistics source of ops.bn_train_forward)."""
    from dasac_hip import ops
    case = _conv_case("1x1_quad_ragged")
    cin, cout = case[1], case[2]

    def case_fn(a):
        o = _conv_operands(a, case, 2)
        spec = o.spec
        assert ops.stats_ok(cout, cin)
        order = ops.gemm_order(spec, False)
        z = a.torch.empty((o.N, cout, o.OH, o.OW), dtype=torch.float32, device=o.x.device)
        tiles = ops.tile_stats_buffer(o.N, cout, o.OH, o.OW, o.x.device)
        ops.conv_gemm(o.x, ops.conv_pack(spec, o.ws, False, None, order=order), ops.conv_table(spec, o.H, o.W, False, o.x.device, order), z,
                      (o.OH, o.OW), 1, cout, spec.K, 1, o.shift, stats=tiles)
        bn = _bn(a, cout, _gen(3))
        y, stats = ops.bn_train_forward(z, bn, res=o.res_out, relu=True, tile_stats=tiles)
        dz, dg, db = ops.bn_train_backward(ops.relu_mask(o.dz, y), z, stats, bn.weight)
        return [z, tiles, y, stats[0], stats[1], bn.running_mean, bn.running_var, bn.num_batches_tracked, dz, dg, db]
    _sweep(monkeypatch, case_fn)


def test_conv_bf16x3(monkeypatch):
    from dasac_hip import ops
    from test_gpu_bf16x3 import CASES
    cin, cout, br, stride, H, W = next(c for c in CASES if (c[0], c[1], c[4], c[5]) == (64, 76, 23, 27))
    monkeypatch.setattr(ops, "PRECISION", "bf16x3")

    def case_fn(a):
        o = _conv_operands(a, ("x3", cin, cout, br, stride, (2, H, W)))
        outs = [ops.conv_forward(o.spec, o.x, o.ws, o.scale, o.shift, o.res_out, relu=True)]
        outs.append(ops.conv_dgrad(o.spec, o.dz, o.ws, (o.H, o.W), scale=o.scale, res=o.res_in, mask=o.act_in))
        packed = ops.conv_pack(o.spec, o.ws, False, o.scale)                  # dasac_conv_pack_x3 in place on a shifted operand
        assert packed.dasac_x3
        return outs + [packed] + ops.conv_wgrad(o.spec, o.dz, o.x, o.ws, scale=o.scale)
    _sweep(monkeypatch, case_fn)


def test_expanded_conv(monkeypatch):
    from dasac_hip import ops
    from test_gpu_expanded_conv import CASES, _inputs
    case = next(c for c in CASES if c[0].startswith("c96_seven_cout5"))
    _, cin, cout, branches, (N, H, W), _ = case
    assert (N, H, W) == (3, 9, 13)

    def case_fn(a):
        ex = ops.ExpandedConv(ops.ConvSpec(cin, cout, branches, 1))
        x, ws, bs, dout, res = _inputs(cin, cout, branches, (N, H, W))
        x, ws, dout, res, bias = a.place(x), [a.place(w) for w in ws], a.place(dout), a.place(res), a.place(sum(bs))
        packed_f, packed_t = ex.pack(ws, False), ex.pack(ws, True)
        table_f, table_t = ops.conv_table(ex.spec1, H, W, False, x.device), ops.conv_table(ex.spec1, H, W, True, x.device)
        out = ex.forward(x, packed_f, table_f, bias)
        d = ex.scatter(dout)
        dws = ex.wgrad(d, x, ws, table_f)
        return [packed_f, packed_t, out, d, ex.dgrad(d, packed_t, table_t, (H, W), res=res, mask=x)] + dws
    _sweep(monkeypatch, case_fn)


# ---- Winograd ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transposed", [False, True], ids=["forward", "transposed"])
@pytest.mark.parametrize("shape", [(2, 32, 128, 9, 7, 4), (1, 32, 128, 11, 13, 2)], ids=lambda s: "x".join(map(str, s)))
def test_winograd_conv(monkeypatch, shape, transposed):
    from dasac_hip import ops
    N, Cin, Cout, H, W, d = shape
    spec = ops.ConvSpec(Cin, Cout, [(3, 3, d, d)])
    C, M = (Cout, Cin) if transposed else (Cin, Cout)

    def case(a):
        g = _gen(sum(shape))
        w = a.place(torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5)
        x, shift, scale = a.place(torch.randn(N, C, H, W, generator=g)), a.place(torch.randn(M, generator=g)), a.place(torch.rand(Cout, generator=g) + 0.5)
        u = ops.winograd_filter(spec, w, transposed, scale)
        dev = x.device
        bits = ops.ReluBits(N, M, H, W, dev)
        y = ops.winograd_conv(x, u, a.torch.empty((N, M, H, W), dtype=torch.float32, device=dev), d, shift, relu=True, bits_out=bits)
        masked = ops.winograd_conv(x, u, a.torch.empty((N, M, H, W), dtype=torch.float32, device=dev), d, mask_bits=bits)
        return [u, y, bits, masked]
    _sweep(monkeypatch, case)


def test_winograd_weight_gradient(monkeypatch):
    from dasac_hip import ops
    N, Cin, Cout, H, W, d = 2, 128, 256, 11, 9, 1
    spec = ops.ConvSpec(Cin, Cout, [(3, 3, d, d)])

    def case(a):
        g = _gen(7)
        x, dz = a.place(torch.randn(N, Cin, H, W, generator=g)), a.place(torch.randn(N, Cout, H, W, generator=g))
        w, scale = a.place(torch.randn(Cout, Cin, 3, 3, generator=g)), a.place(torch.rand(Cout, generator=g) + 0.5)
        dev = x.device
        dot = a.torch.empty((ops.dot_rows(spec), Cout), dtype=torch.float32, device=dev)
        sums = a.torch.empty(Cout, dtype=torch.float32, device=dev)
        return [ops.winograd_wgrad(spec, dz, x, w, scale=scale, dot=dot, sum_dz=sums), dot, sums]
    _sweep(monkeypatch, case)


# ---- optimisers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_fused_optimisers(monkeypatch, kind):
    """Two steps over parameters of 1, 4097 and 64*3*7*7 elements: p and grad placed by the test, the state allocated through the
    stand-in (`empty_like` / `zeros_like` in dasac_hip.optim); row tables and chunk lists are uploads of host arrays and stay
    aligned."""
    from dasac_hip import optim

    def case(a):
        g = _gen(13)
        params = [torch.nn.Parameter(a.place(torch.randn(s, generator=g), inplace=True)) for s in ((1,), (4097,), (64, 3, 7, 7))]
        groups = [dict(params=params[:2], lr=0.01, weight_decay=5e-4), dict(params=params[2:], lr=0.1, weight_decay=0.0)]
        opt = optim.FusedAdam(groups, betas=(0.5, 0.999)) if kind == "adam" else optim.FusedSGD(groups, momentum=0.9, nesterov=True)
        for _ in range(2):
            for p in params:
                p.grad = a.place(torch.randn(p.shape, generator=g))
            opt.step()
        state = [opt.state[p][k] for p in params for k in (("exp_avg", "exp_avg_sq") if kind == "adam" else ("momentum_buffer",))]
        return [p.detach() for p in params] + state
    _sweep(monkeypatch, case)


# ---- byte pipelines: all 16 byte phases ------------------------------------------------------------------------------------------
BYTE_PHASES = range(16)


def test_source_crops_resize_and_make_crops(monkeypatch):
    import crops
    from test_gpu_crops import _fresh
    gen = np.random.RandomState(5)
    imgs = [_fresh(gen, 180, 300), _fresh(gen, 200, 310), _fresh(gen, 150, 280)]
    sc = crops.SourceCrops((120, 200), scale_range=(0.5, 2.0), blur=True, jitter=0.5, seed=21, want_u8=True)
    draws = []
    while not (any(d["blur"] for d in draws) and any(d["jitter"] for d in draws)):
        draws = [sc.sample(i.shape[:2]) for i, _ in imgs]

    def case(a):
        # device images: `pack` gathers them into flat device buffers through the stand-in; resize, the in-place photometric step
        # on the scaled bytes and make_crops follow
        return list(sc.make([a.place(torch.from_numpy(i)) for i, _ in imgs], [a.place(torch.from_numpy(x)) for _, x in imgs], params=draws))
    _sweep(monkeypatch, case, BYTE_PHASES)


def _view_image(H, W, seed):
    gen = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([(127 + 100 * np.sin(xx / (4.0 + c) + yy / 7.0) + gen.randint(-20, 21, (H, W))).clip(0, 255) for c in range(3)], 0).astype(np.uint8)
    lab = gen.randint(0, 19, ((H + 7) // 8, (W + 7) // 8)).repeat(8, 0).repeat(8, 1)[:H, :W].astype(np.uint8)
    msk = (gen.rand(H, W) < 0.1).astype(np.uint8)
    return torch.from_numpy(img), torch.from_numpy(lab), torch.from_numpy(msk)


def test_target_views_make_and_augment(monkeypatch):
    import views
    hw, seed = (64, 96), 3
    tv = views.TargetViews(hw, 4, zoom_range=(0.5, 1.0), seed=seed, blur=(.1, 2.), jitter=0.4, jitter_p=0.75, grey_p=0.3)
    vs, photo = tv.sample(), tv.sample_photometric()
    img, lab, msk = _view_image(hw[0], hw[1], seed)

    def case(a):
        f1, gt, f2, theta, theta_inv, u8 = tv.make(a.place(img), a.place(lab), a.place(msk), views=vs, photo=photo, want_u8=True)
        return [f1, gt, f2, u8]
    _sweep(monkeypatch, case, BYTE_PHASES)


@pytest.mark.parametrize("hw,seed", [((5, 3), 4), ((37, 53), 1)], ids=["5x3", "37x53"])
def test_target_views_photometric_path(monkeypatch, hw, seed):
    """dasac_view_photometric on fresh views, as test_gpu_photometric.py feeds it: blur, jitter and greyscale rows, with labels."""
    import views
    H, W = hw
    nv = 4
    tv = views.TargetViews(hw, nv, seed=seed, blur=(.1, 2.), jitter=0.4, jitter_p=0.75, grey_p=0.3)
    photo = tv.sample_photometric()
    gen = np.random.RandomState(seed)
    u8 = torch.from_numpy(gen.randint(0, 256, (nv, 3, H, W)).astype(np.uint8))
    gt = torch.from_numpy(gen.randint(0, 19, (nv, H, W)).astype(np.int64))

    def case(a):
        return list(tv.augment(a.place(u8), a.place(gt), photo, want_u8=True))
    _sweep(monkeypatch, case, BYTE_PHASES)


@pytest.mark.parametrize("B,H,W,size,target", [(3, 5, 3, (9, 130), False), (2, 33, 49, (1, 7), True)], ids=["3x5x3", "2x33x49"])
def test_visualise_panels_and_grid(monkeypatch, B, H, W, size, target):
    import visualise as V
    from test_gpu_visualise import random_case
    image, gt, outs, image2 = random_case(B, H, W, 7 * H + W + B, target)

    def case(a):
        d_outs = {k: a.place(v) for k, v in outs.items()}
        strip, rows = V.render(a.place(image), a.place(gt), d_outs, im_size=size, image2=None if image2 is None else a.place(image2), want_u8=True)
        return [strip, rows, V.to_grid(strip)]
    _sweep(monkeypatch, case, BYTE_PHASES)


@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8], ids=["int64", "uint8"])
def test_label_nodes(monkeypatch, dtype):
    from dasac_hip import ops
    from test_gpu_class_features import NODE_SHAPES, RADII, label_maps
    size, nodes_hw = min(NODE_SHAPES, key=lambda s: s[0][0] * s[0][1])
    lab = torch.from_numpy(label_maps(size, 19, dtype))

    def case(a):
        dev = a.place(lab)
        return [ops.label_nodes(dev, nodes_hw, 19, r) for r in RADII]
    _sweep(monkeypatch, case, BYTE_PHASES)


# ---- descriptor tables one element off -------------------------------------------------------------------------------------------
def _filled(shape, dtype=torch.float32):
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(-1).view(torch.uint8).fill_(SENTINEL)
    return t


def _untouched(t):
    return bool((t.reshape(-1).view(torch.uint8) == SENTINEL).all())


def _one_off(t):
    """A copy of a device table that starts one int32 past a 256-byte boundary, inside a live allocation: were the call to
    launch after all, it would read what the aligned table holds."""
    raw = t.contiguous().view(-1).view(torch.uint8)
    big = torch.zeros(raw.numel() + 256, dtype=torch.uint8, device=t.device)
    view = big[4:4 + raw.numel()]
    view.copy_(raw)
    assert view.data_ptr() % 256 == 4
    return view


def _refused(entry, call, outputs):
    """call(shifted: bool) -> return code.  One element off: DASAC_EINVAL naming the alignment, nothing written; aligned: accepted."""
    from dasac_hip import lib as L
    lib = L.load()
    rc = call(True)
    err = lib.dasac_last_error()
    torch.cuda.synchronize()
    assert rc == -1 and b"misaligned" in err, (entry, rc, err)                        # DASAC_EINVAL
    for i, t in enumerate(outputs):
        assert _untouched(t), "{}: output {} was written by the refused call".format(entry, i)
    rc = call(False)
    torch.cuda.synchronize()
    assert rc == 0, (entry, lib.dasac_last_error())
    assert not outputs or not all(_untouched(t) for t in outputs), entry


def test_conv_entries_refuse_a_table_one_element_off():
    from dasac_hip import ops
    L = ops.L
    lib, s = L.load(), L.stream_ptr()
    N, cin, cout, H, W = 2, 128, 128, 5, 7
    spec = ops.ConvSpec(cin, cout, [(1, 1, 1, 0)], 1)
    g = _gen(1)
    x, dz = torch.randn(N, cin, H, W, generator=g).cuda(), torch.randn(N, cout, H, W, generator=g).cuda()
    w = torch.randn(cout, cin, 1, 1, generator=g).cuda()
    table = ops.conv_table(spec, H, W, False, x.device)
    packed = ops.conv_pack(spec, [w], False)
    off = _one_off(table)
    tp = lambda shifted: off.data_ptr() if shifted else table.data_ptr()
    cols = [torch.tensor(c, dtype=torch.int32) for c in zip(*spec.branches)]
    fresh = _filled(tuple(table.shape) + (2,), torch.int32).view(-1)                   # room for the table at either start
    _refused("dasac_conv_table", lambda sh: lib.dasac_conv_table(cols[0].data_ptr(), cols[1].data_ptr(), cols[2].data_ptr(), cols[3].data_ptr(), 1,
                                                                 cin, H, W, 0, 0, fresh.data_ptr() + (4 if sh else 0), s), [fresh])
    geom = (N, cin, H, W, H, W, 1, cout, spec.K, H, W, 1)
    out = _filled((N, cout, H, W))
    _refused("dasac_conv_gemm", lambda sh: lib.dasac_conv_gemm(x.data_ptr(), packed.data_ptr(), tp(sh), out.data_ptr(), *geom, None, None, None,
                                                               None, None, 0, 0, 0, 1, None, 0, s), [out])
    out, stats = _filled((N, cout, H, W)), _filled(tuple(ops.tile_stats_buffer(N, cout, H, W, x.device).shape))
    _refused("dasac_conv_gemm_stats", lambda sh: lib.dasac_conv_gemm_stats(x.data_ptr(), packed.data_ptr(), tp(sh), out.data_ptr(), *geom, None,
                                                                           None, 0, 0, 0, 1, None, 0, stats.data_ptr(), s), [out, stats])
    packed_x3 = packed.clone()
    L.check(lib.dasac_conv_pack_x3(packed_x3.data_ptr(), cout, spec.K, packed_x3.data_ptr(), s), "dasac_conv_pack_x3")
    out = _filled((N, cout, H, W))
    _refused("dasac_conv_gemm_x3", lambda sh: lib.dasac_conv_gemm_x3(x.data_ptr(), packed_x3.data_ptr(), tp(sh), out.data_ptr(), *geom, None, None,
                                                                     None, None, None, 0, 0, 0, 1, None, 0, s), [out])
    out = _filled((N, cout, H, W))
    _refused("dasac_conv_gemm_batched", lambda sh: lib.dasac_conv_gemm_batched(x.data_ptr(), packed.data_ptr(), tp(sh), out.data_ptr(), *geom,
                                                                               1, 0, 0, 0, s), [out])
    need = lib.dasac_conv_wgrad_workspace(N, H, W, cout, spec.K)
    for entry in ("dasac_conv_wgrad", "dasac_conv_wgrad_x3"):
        ws = _filled((need,), torch.uint8)
        _refused(entry, lambda sh: getattr(lib, entry)(dz.data_ptr(), x.data_ptr(), tp(sh), N, cin, H, W, H, W, 1, cout, spec.K, ws.data_ptr(),
                                                       need, s), [ws])


def test_refresh_and_teacher_entries_refuse_tables_one_element_off():
    from dasac_hip import ops
    L = ops.L
    lib, s = L.load(), L.stream_ptr()
    g = _gen(2)
    C, cin, cout = 5, 8, 40
    gamma, beta, mean, var = (torch.rand(C, generator=g).cuda() + 0.5 for _ in range(4))
    fold_outs = tuple(_filled((C,)) for _ in range(3))
    w = torch.randn(cout, cin, 1, 1, generator=g).cuda()
    Kpad, Mpad = lib.dasac_conv_kpad(cin), lib.dasac_conv_mpad(cout)
    packed = _filled((Kpad, Mpad))
    t = ops.build_refresh_tables([(gamma, beta, mean, var, None, fold_outs, 1e-5, C)], [(w, None, packed, cout, cin, 1, Mpad, Kpad, 0, 0)], w.device)
    for entry, jobs, chunks, n, outs in (("dasac_bn_fold_multi", t["fold"], t["fold_chunks"], t["n_fold_chunks"], list(fold_outs)),
                                         ("dasac_conv_pack_multi", t["pack"], t["pack_chunks"], t["n_pack_chunks"], [packed])):
        for which in ("jobs", "chunks"):
            for o in outs:
                o.view(-1).view(torch.uint8).fill_(SENTINEL)
            j_off, c_off = _one_off(jobs), _one_off(chunks)
            _refused("{} ({})".format(entry, which), lambda sh: getattr(lib, entry)(
                (j_off if sh and which == "jobs" else jobs).data_ptr(), (c_off if sh and which == "chunks" else chunks).data_ptr(), n, s), outs)
    fast, slow = [torch.randn(n, generator=g).cuda() for n in (3, 4097)], [torch.randn(n, generator=g).cuda() for n in (3, 4097)]
    plan = ops.EmaPlan(fast, slow)
    before = [t_.clone() for t_ in slow]
    for which in ("pairs", "chunks", "sq"):
        out = _filled((1,))
        p_off, c_off = _one_off(plan.pairs), _one_off(plan.chunks)
        sq_off = torch.zeros(plan.sq.numel() * 8 + 256, dtype=torch.uint8, device="cuda")[4:4 + plan.sq.numel() * 8]
        _refused("dasac_ema_update ({})".format(which), lambda sh: lib.dasac_ema_update(
            (p_off if sh and which == "pairs" else plan.pairs).data_ptr(), plan.n_tensors, (c_off if sh and which == "chunks" else plan.chunks).data_ptr(),
            plan.n_chunks, 0.99, 0, (sq_off if sh and which == "sq" else plan.sq).data_ptr(), out.data_ptr(), s), [out])
    assert all(torch.equal(a_, b_) for a_, b_ in zip(slow, before))                    # update = 0 throughout


def test_optimiser_entries_refuse_tables_one_element_off():
    from dasac_hip import lib as L
    lib, s = L.load(), L.stream_ptr()
    g = _gen(3)
    sizes = (3, 4097)
    chunk = lib.dasac_ema_chunk_elems()
    chunks = torch.tensor([(i, j) for i, n in enumerate(sizes) for j in range((n + chunk - 1) // chunk)], dtype=torch.int32).cuda()
    nc = chunks.shape[0]
    lr, wd = (ctypes.c_float * 1)(0.1), (ctypes.c_float * 1)(1e-4)
    lrp, wdp = ctypes.cast(lr, ctypes.c_void_p), ctypes.cast(wd, ctypes.c_void_p)

    def tensors(k):
        return [[torch.randn(n, generator=g).cuda() for n in sizes] for _ in range(k)]

    def both(entry, rows, untouched, call):
        """Each of the row table and the chunk list one int32 off in turn; `untouched`: the tensors a launch would have written."""
        rows = torch.from_numpy(rows).cuda()
        r_off, c_off = _one_off(rows), _one_off(chunks)
        for which in ("tensors", "chunks"):
            before = [t_.clone() for t_ in untouched]
            rc = call((r_off if which == "tensors" else rows).data_ptr(), (c_off if which == "chunks" else chunks).data_ptr())
            err = lib.dasac_last_error()
            torch.cuda.synchronize()
            assert rc == -1 and b"misaligned" in err, (entry, which, rc, err)
            assert all(torch.equal(a_, b_) for a_, b_ in zip(untouched, before)), (entry, which)
        before = [t_.clone() for t_ in untouched]
        rc = call(rows.data_ptr(), chunks.data_ptr())
        torch.cuda.synchronize()
        assert rc == 0, (entry, lib.dasac_last_error())
        return before

    ctl = torch.zeros(4, dtype=torch.float32, device="cuda")
    ctl[1] = 1.0
    # SGD rows {p, g, g2, buf, n, group} (48 bytes)
    for entry in ("dasac_sgd_step", "dasac_sgd_nesterov_step", "dasac_sgd_step_ctl", "dasac_sgd_nesterov_step_ctl"):
        p, gr, buf = tensors(3)
        rows = np.asarray([(a_.data_ptr(), b_.data_ptr(), 0, c_.data_ptr(), a_.numel(), 0) for a_, b_, c_ in zip(p, gr, buf)], dtype=np.int64)
        tail = (ctl.data_ptr(), 0, 0, s) if entry.endswith("_ctl") else (s,)
        before = both(entry, rows, p + buf, lambda t_, c_: getattr(lib, entry)(t_, len(sizes), c_, nc, lrp, wdp, 1, 0.9, 1, *tail))
        assert not any(torch.equal(a_, b_) for a_, b_ in zip(p, before))               # the aligned call did step
    # Adam rows {p, g, g2, m, v, n, group, step_size, bc2_sqrt} (64 bytes)
    for entry in ("dasac_adam_step", "dasac_adam_step_ctl"):
        p, gr, m, v = tensors(4)
        v = [t_.abs() for t_ in v]
        rows = np.zeros((len(sizes), 8), dtype=np.int64)
        rows[:, :7] = [(a_.data_ptr(), b_.data_ptr(), 0, c_.data_ptr(), d_.data_ptr(), a_.numel(), 0) for a_, b_, c_, d_ in zip(p, gr, m, v)]
        rows.view(np.float32)[:, 14:16] = (0.01, 0.5)
        tail = (ctl.data_ptr(), 0, 0, s) if entry.endswith("_ctl") else (s,)
        before = both(entry, rows, p + m + v, lambda t_, c_: getattr(lib, entry)(t_, len(sizes), c_, nc, wdp, 1, 0.5, 0.999, 1e-8, *tail))
        assert not any(torch.equal(a_, b_) for a_, b_ in zip(p, before))
    # dasac_grad_norm over the 48-byte rows: writes the control block
    p, gr, buf = tensors(3)
    rows = np.asarray([(a_.data_ptr(), b_.data_ptr(), 0, c_.data_ptr(), a_.numel(), 0) for a_, b_, c_ in zip(p, gr, buf)], dtype=np.int64)
    norm_ctl = torch.zeros(4, dtype=torch.float32, device="cuda")
    ws = torch.zeros(lib.dasac_grad_norm_workspace(nc), dtype=torch.uint8, device="cuda")
    both("dasac_grad_norm", rows, [norm_ctl, ws], lambda t_, c_: lib.dasac_grad_norm(t_, 48, len(sizes), c_, nc, 1.0, ws.data_ptr(), ws.numel(),
                                                                                    norm_ctl.data_ptr(), None, s))
    want = float(torch.cat([t_.double().view(-1) for t_ in gr]).pow(2).sum().sqrt())
    assert abs(float(norm_ctl[0]) - want) <= 1e-6 * want
