"""Reference interpreter for `dasac_hip.engine.Plan` objects and a catalogue of small synthetic plans (a helper of
test_engine_plans_cpu.py and test_gpu_engine_plans.py, not a conftest).

`run_reference` evaluates a plan with plain torch functions on the CPU, in any dtype, and lets autograd differentiate it: it
reads the plan's STRUCTURE (the op objects' fields and the modules' tensors) and never calls Engine, _BackwardPass or an ops.*
function.  `PLANS` is a list of (name, build); every plan is a few convolutions over a 2 x 3 x (9..17)^2 image and isolates
branch combinations of engine.py that the three shipped networks do not contain; `features` (name -> the slots / op indices it
lives at) says which, so that a test can assert that the plan really has them and that a pass really took them.

Channel counts and the engine's kernel choices: a ReLU pattern is recorded / applied as bits, and a train-mode BN reads tile
statistics from the GEMM epilogue, when the GEMM's output rows pad to the 128-row tile (dasac_conv_mpad: more than 64 channels) and
the gathered channel count is a multiple of 16.  80 and 96 satisfy both, 24 / 40 (padded to 32 / 64, no multiple of 16) neither,
48 only the second."""
import collections

import torch
import torch.nn as nn
import torch.nn.functional as F

from dasac_hip import engine as E

SEEDS = (1, 2)            # the seeds both test modules use; test_engine_plans_cpu.py checks the preconditions for exactly these


# ---------------------------------------------------------------------------------------------------------------
# the kernel-choice rules of csrc/conv_gemm.hip and csrc/conv_wgrad.hip, restated on the host (test_engine_plans_cpu.py compares them with the library)
# ---------------------------------------------------------------------------------------------------------------
def mpad(M):
    return (M + 127) // 128 * 128 if M > 64 else (64 if M > 32 else 32)


def bits_ok(M, Cx):
    """An output of M channels over Cx gathered channels has the bit-mask (and the tile-statistics) GEMM variant."""
    return mpad(M) % 128 == 0 and Cx % 16 == 0


stats_ok = bits_ok


# ---------------------------------------------------------------------------------------------------------------
# reference interpreter
# ---------------------------------------------------------------------------------------------------------------
Reference = collections.namedtuple("Reference", "acts grad_at params pre_bn")
Reference.__doc__ = """acts[slot]: the slot's activation (retain_grad).  grad_at[slot]: the tensor whose .grad is what the engine calls
the slot's gradient -- the one w.r.t. the op output with the producer's ReLU pattern applied, i.e. w.r.t. the pre-activation of a
ReLU conv.  params: copies of the parameters in the order of Engine.params.  pre_bn[op index]: the raw conv output (retain_grad) in
front of a train-mode BN."""


class RecordingRelu:
    """ReLU that keeps its pre-activations, in call order = the plan order of the ReLU convs."""

    def __init__(self):
        self.z = []

    def __call__(self, z):
        self.z.append(z.detach())
        return torch.relu(z)


def relu_slots(plan):
    """Slots closed by a ReLU, in the order the `relu` callable of run_reference is called."""
    return [op.dst for op in plan.ops if op.kind == "conv" and op.relu]


def run_reference(plan, x, dtype, relu=None):
    relu = torch.relu if relu is None else relu

    def copy(t):
        return t.detach().cpu().clone().to(dtype)

    acts = {0: copy(x)}
    grad_at, params, pre_bn = {}, [], {}
    for i, op in enumerate(plan.ops):
        xin = acts[op.src]
        if op.kind == "conv":
            ws = [copy(c.weight).requires_grad_(True) for c in op.convs]
            bs = [copy(c.bias).requires_grad_(True) if c.bias is not None else None for c in op.convs]
            bn = [] if op.bn is None else [copy(op.bn.weight).requires_grad_(True), copy(op.bn.bias).requires_grad_(True)]
            params += ws + [b for b in bs if b is not None] + bn
            z = None
            for c, w, b in zip(op.convs, ws, bs):
                t = F.conv2d(xin, w, b, stride=c.stride, padding=c.padding, dilation=c.dilation)
                z = t if z is None else z + t
            if op.bn is not None and op.bn.training:
                z.retain_grad()
                pre_bn[i] = z
                z = F.batch_norm(z, None, None, bn[0], bn[1], True, 0.0, op.bn.eps)
            elif op.bn is not None:
                z = F.batch_norm(z, copy(op.bn.running_mean), copy(op.bn.running_var), bn[0], bn[1], False, 0.0, op.bn.eps)
            if op.res is not None:
                z = z + acts[op.res]
            if op.relu:
                z.retain_grad()
                grad_at[op.dst] = z
                z = relu(z)
            out = z
        elif op.kind == "pool":
            out = F.max_pool2d(xin, op.k, op.s, op.p, ceil_mode=op.ceil)
        elif op.kind == "up2add":
            out = F.interpolate(xin, scale_factor=2, mode="bilinear", align_corners=True) + acts[op.skip]
        elif op.kind == "drop":
            m = op.module
            # (eval mode: the same values as a node of its own, so that the gradient of this slot is not also its source's)
            out = xin * copy(m.keep_mask)[:, :, None, None] if (m.training and m.p > 0) else xin.view_as(xin)
        else:
            raise ValueError("unknown op kind {!r}".format(op.kind))
        out.retain_grad()
        acts[op.dst] = out
        grad_at.setdefault(op.dst, out)
    return Reference(acts, grad_at, params, pre_bn)


def param_roles(plan):
    """(op index, role) of every parameter in the order of Engine.params; role: "w", "b", "gamma" or "beta"."""
    roles = []
    for i, op in enumerate(plan.ops):
        if op.kind == "conv":
            w, b, bn = op.owner_groups()
            roles += [(i, "w")] * len(w) + [(i, "b")] * len(b) + [(i, r) for r, _ in zip(("gamma", "beta"), bn)]
    return roles


def zero_by_construction(plan):
    """Indices of the conv biases in front of a train-mode BN: the batch mean takes the bias out again, so their gradient is
    exactly zero in exact arithmetic and pure round-off in any floating-point one."""
    return [j for j, (i, r) in enumerate(param_roles(plan)) if r == "b" and plan.ops[i].bn is not None and plan.ops[i].bn.training]


def need_sets(plan):
    """name -> need list (one flag per parameter): the subsets of `_param_grads` that "everything trainable" never takes."""
    roles = param_roles(plan)
    first = lambda role: next(j for j, (_, r) in enumerate(roles) if r == role)
    return collections.OrderedDict([
        ("all", [True] * len(roles)),
        ("weights", [r == "w" for _, r in roles]),
        ("bn_affine", [r in ("gamma", "beta") for _, r in roles]),
        ("biases", [r == "b" for _, r in roles]),
        ("first_two_ops_frozen", [i >= 2 for i, _ in roles]),
        ("one_bias", [j == first("b") for j in range(len(roles))]),
        ("one_gamma", [j == first("gamma") for j in range(len(roles))]),
    ])


NEED_SETS = ("res_conv_first_bits", "strided_pair_bits")      # frozen BN, train-mode BN


# ---------------------------------------------------------------------------------------------------------------
# plan catalogue
# ---------------------------------------------------------------------------------------------------------------
class _Builder:
    """Modules with He-initialised weights and randomised BN vectors, as in the Winograd engine test."""

    def __init__(self, seed):
        self.gen = torch.Generator().manual_seed(seed)
        self.P = E.Plan()
        self.features = {}

    def randn(self, *shape):
        return torch.randn(*shape, generator=self.gen)

    def conv_module(self, cin, cout, k=1, stride=1, dil=1, pad=None, bias=False):
        pad = (dil * (k - 1) // 2) if pad is None else pad
        c = nn.Conv2d(cin, cout, k, stride=stride, padding=pad, dilation=dil, bias=bias)
        with torch.no_grad():
            c.weight.copy_(self.randn(*c.weight.shape) * (2.0 / (cin * k * k)) ** 0.5)
            if bias:
                c.bias.copy_(self.randn(cout) * 0.2)
        return c

    def bn_module(self, ch, train=False):
        bn = nn.BatchNorm2d(ch)
        with torch.no_grad():
            bn.weight.copy_(torch.rand(ch, generator=self.gen) + 0.5)
            bn.bias.copy_(self.randn(ch) * 0.2)
            bn.running_mean.copy_(self.randn(ch) * 0.2)
            bn.running_var.copy_(torch.rand(ch, generator=self.gen) + 0.5)
        return bn.train(train)

    def conv(self, src, cin, cout, k=1, stride=1, dil=1, pad=None, bias=False, bn=None, relu=False, res=None):
        """bn: None, "frozen" or "train"."""
        bnm = None if bn is None else self.bn_module(cout, bn == "train")
        return self.P.conv(src, self.conv_module(cin, cout, k, stride, dil, pad, bias), bnm, relu, res)

    def conv_sum(self, src, cin, cout, dils, bias=True):
        return self.P.conv_sum(src, [self.conv_module(cin, cout, 3, dil=d, bias=bias) for d in dils])

    def dropout(self, src, shape, train):
        m = nn.Dropout2d(0.5).train(train)
        if train:
            keep = (torch.rand(*shape, generator=self.gen) < 0.5).float()
            keep[0, 0], keep[-1, -1] = 0.0, 1.0                    # at least one plane dropped, one kept
            m.keep_mask = keep / (1.0 - m.p)
        return self.P.dropout2d(src, m)

    def op_index(self, slot):
        return next(i for i, op in enumerate(self.P.ops) if op.dst == slot)

    def finish(self, out, x_shape, out_shape):
        plan = self.P.finish(out)
        return plan, self.randn(*x_shape), self.randn(*out_shape), self.features


def _stem(b, c0, bn="frozen", bias=False):
    """From the image: 3x3 stride 2 (slot 0 gets no data gradient)."""
    s = b.conv(0, 3, c0, 3, stride=2, pad=1, bias=bias, bn=bn, relu=True)
    b.features["conv:image_s2"] = dict(op=b.op_index(s))
    return s


def _residual(seed, c0, c, join_last, n=2, hw=(17, 13)):
    """A ReLU slot with three consumers: two convs and a residual.  join_last False: the stride-1 conv is the first consumer in
    plan order = the last to arrive in the backward pass: its data-gradient epilogue adds the other two gradients (res=) and
    applies the pattern (bits for c = 80, the fp32 activation for c = 40).  join_last True: the residual consumer comes first in
    plan order, so `join` arrives last and runs relu_mask(add(cur, t), acts)."""
    b = _Builder(seed)
    bits = bits_ok(c, c0) and bits_ok(c, c)
    s1 = _stem(b, c0)                                                      # frozen BN, no conv bias
    s2 = b.conv(s1, c0, c, bias=True, bn="frozen", relu=True)              # the slot; frozen BN with a conv bias
    b.features["bn:frozen_nobias"] = dict(op=b.op_index(s1))
    b.features["bn:frozen_bias"] = dict(op=b.op_index(s2))
    b.features["conv:1x1"] = dict(op=b.op_index(s2))
    if not join_last:
        s3 = b.conv(s2, c, c, 3, dil=2, bn="frozen", relu=True)
        s4 = b.conv(s2, c, c, bias=True)                                   # no BN, with a bias
        s5 = b.conv(s3, c, c, bn="frozen", relu=True, res=s2)
        out = b.conv(s5, c, c, res=s4)                                     # no BN, no bias
        b.features["order:conv_first"] = dict(slot=s2, bits=bits)
        b.features["nobn:bias"] = dict(op=b.op_index(s4))
        b.features["nobn:nobias"] = dict(op=b.op_index(out))
    else:
        s3 = b.conv(s1, c0, c, bn="frozen")
        s4 = b.conv(s3, c, c, bn="frozen", relu=True, res=s2)              # the residual consumer: first in plan order
        s5 = b.conv(s2, c, c, 3, dil=2, bn="frozen", relu=True)
        s6 = b.conv(s2, c, c, bias=True)
        s7 = b.conv(s5, c, c, res=s4)
        out = b.conv(s7, c, c, res=s6)
        b.features["order:join_last"] = dict(slot=s2, could_use_bits=bits)
        s3 = s5
    b.features["conv:dilated"] = dict(op=b.op_index(s3))
    oh, ow = (hw[0] + 1) // 2, (hw[1] + 1) // 2
    return b.finish(out, (n, 3) + hw, (n, c, oh, ow))


def _strided_pair(seed, c0, c):
    """ResNet's strided block: the block input (a ReLU slot) is read by two stride-2 1x1 convs.  The second one's data gradient
    is scattered into a zero-filled tensor, the first one's in place on top of it, then relu_mask applies the pattern.  The last
    two convs run a train-mode BN (tile statistics from the GEMM for c = 80, a statistics pass for c = 40); the last one has a
    conv bias, a residual and a ReLU."""
    b = _Builder(seed)
    s1 = _stem(b, c0)
    s2 = b.conv(s1, c0, c, stride=2, bn="frozen", relu=True)
    s3 = b.conv(s1, c0, c, stride=2, bias=True, bn="frozen")
    s4 = b.conv(s2, c, c, 3, bn="train", relu=True)
    out = b.conv(s4, c, c, bias=True, bn="train", relu=True, res=s3)
    b.features["order:strided_pair"] = dict(slot=s1)
    b.features["bn:train_stats" if stats_ok(c, c) else "bn:train_nostats"] = dict(op=b.op_index(out))
    return b.finish(out, (2, 3, 17, 13), (2, c, 5, 4))


def _mixed_bits(seed):
    """Bits on one side only.  Slot A (48 -> 80) records bits, but its first consumer 80 -> 40 gathers 40 channels in its data
    gradient and takes the fp32 activation (with res= from the residual consumer).  Slot B (40 -> 80) cannot record bits although
    its consumer 80 -> 80 could use them."""
    b = _Builder(seed)
    s1 = _stem(b, 48, bn=None, bias=True)
    a = b.conv(s1, 48, 80, bn="frozen", relu=True)
    s3 = b.conv(a, 80, 40, 3, relu=True)
    bb = b.conv(s3, 40, 80, bn="frozen", relu=True)
    out = b.conv(bb, 80, 80, bn="frozen", res=a)
    b.features["bits:recorded_consumer_fp32"] = dict(slot=a)
    b.features["bits:producer_cannot"] = dict(slot=bb)
    b.features["nobn:bias"] = dict(op=b.op_index(s1))
    b.features["nobn:nobias"] = dict(op=b.op_index(s3))
    return b.finish(out, (2, 3, 15, 11), (2, 80, 8, 6))


def _aspp(seed, c0, c, expanded_first):
    """Four dilated 3x3 branches into 8 channels (the tap-expanded form) next to a plain 1x1 conv on one ReLU slot.
    expanded_first: the expanded conv arrives last in the backward pass: ex.dgrad(res=g, mask=pattern)."""
    b = _Builder(seed)
    s1 = _stem(b, c0)
    s2 = b.conv(s1, c0, c, bn="frozen", relu=True)
    if expanded_first:
        ex = b.conv_sum(s2, c, 8, (1, 2, 3, 4))
        s4 = b.conv(s2, c, 8, bias=True)
        out = b.conv(s4, 8, 8, res=ex)
        b.features["conv:expanded_first"] = dict(slot=s2, op=b.op_index(ex), bits=bits_ok(c, c0) and bits_ok(c, 36 * 8))
    else:
        s3 = b.conv(s2, c, 8, bias=True)
        ex = b.conv_sum(s2, c, 8, (1, 2, 3, 4))
        out = b.conv(s3, 8, 8, res=ex)
        b.features["conv:expanded_second"] = dict(slot=s2, op=b.op_index(ex), plain=b.op_index(s3))
    return b.finish(out, (2, 3, 13, 17), (2, 8, 7, 9))


def _sum40(seed):
    """conv_sum of two branches into 40 channels: too wide for the expanded form, so one GEMM over both branches' taps, the sum of
    the two biases as its shift (Engine.fold with bn None) and one channel-sums vector fanned out to both bias gradients."""
    b = _Builder(seed)
    s1 = _stem(b, 24)
    s2 = b.conv_sum(s1, 24, 40, (1, 2))
    out = b.conv(s2, 40, 8, bias=True)
    b.features["conv:sum40"] = dict(op=b.op_index(s2))
    return b.finish(out, (2, 3, 11, 9), (2, 8, 6, 5))


def _pools(seed):
    b = _Builder(seed)
    s1 = _stem(b, 24)                                       # 17 x 15 -> 9 x 8
    s2 = b.P.maxpool(s1, 3, 2, 1, ceil_mode=True)           # behind a ReLU conv -> 5 x 5
    s3 = b.conv(s2, 24, 40, 3, bias=True)
    s4 = b.P.maxpool(s3, 2, 2)                              # behind a conv without ReLU -> 2 x 2
    s5 = b.conv(s4, 40, 40, bn="frozen", relu=True)
    s6 = b.P.maxpool(s5, 3, 1, 1)
    out = b.conv(s6, 40, 8)
    b.features["pool:k3s2p1_ceil_relu"] = dict(op=b.op_index(s2))
    b.features["pool:k2s2_norelu"] = dict(op=b.op_index(s4))
    b.features["pool:k3s1p1"] = dict(op=b.op_index(s6))
    return b.finish(out, (2, 3, 17, 15), (2, 8, 2, 2))


def _fcn(seed):
    """FCN-8s in small: fc6 - dropout - fc7 - dropout - score, two chained up2_add over the pool scores.  The first dropout trains
    with a pinned mask, the second is in eval mode and returns its input tensor itself; the skip of the second up2_add is a ReLU
    slot that a conv reads as well -- later in plan order, so the up2_add's `join` applies the pattern."""
    b = _Builder(seed)
    s1 = b.conv(0, 3, 24, 3, stride=2, pad=0, bn="frozen", relu=True)        # 17 x 17 -> 8 x 8
    s2 = b.P.maxpool(s1, 2, 2)                                               # 4 x 4
    s3 = b.conv(s2, 24, 40, 3, bias=True, relu=True)
    s4 = b.P.maxpool(s3, 2, 2)                                               # 2 x 2
    s5 = b.conv(s4, 40, 40, bias=True, relu=True)
    s6 = b.dropout(s5, (2, 40), train=True)
    s7 = b.conv(s6, 40, 40, bias=True, relu=True)
    s8 = b.dropout(s7, (2, 40), train=False)
    s9 = b.conv(s8, 40, 8, bias=True)
    s10 = b.conv(s2, 24, 8, bias=True)
    s11 = b.P.up2_add(s9, s10)                                               # 4 x 4
    s12 = b.conv(0, 3, 8, 3, stride=2, pad=0, bias=True, relu=True)          # 8 x 8, the busy ReLU skip
    s13 = b.P.up2_add(s11, s12)
    s14 = b.conv(s12, 8, 8)
    out = b.conv(s13, 8, 8, res=s14)
    b.features["up2add:chain"] = dict(ops=(b.op_index(s11), b.op_index(s13)))
    b.features["up2add:busy_relu_skip"] = dict(slot=s12, op=b.op_index(s13))
    b.features["drop:train_pinned"] = dict(op=b.op_index(s6))
    b.features["drop:eval_alias"] = dict(op=b.op_index(s8))
    return b.finish(out, (2, 3, 17, 17), (2, 8, 8, 8))


PLANS = [
    ("res_conv_first_bits", lambda seed: _residual(seed, 48, 80, False)),
    ("res_conv_first_fp32", lambda seed: _residual(seed, 24, 40, False, hw=(15, 11))),
    ("res_join_last_bits", lambda seed: _residual(seed, 48, 96, True, hw=(13, 17))),
    ("res_join_last_fp32_n1", lambda seed: _residual(seed, 24, 40, True, n=1, hw=(17, 15))),
    ("strided_pair_bits", lambda seed: _strided_pair(seed, 48, 80)),
    ("strided_pair_fp32", lambda seed: _strided_pair(seed, 24, 40)),
    ("mixed_bits", _mixed_bits),
    ("aspp_first_bits", lambda seed: _aspp(seed, 48, 80, True)),
    ("aspp_first_fp32", lambda seed: _aspp(seed, 24, 40, True)),
    ("aspp_second", lambda seed: _aspp(seed, 48, 80, False)),
    ("sum40", _sum40),
    ("pools", _pools),
    ("fcn", _fcn),
]

# every feature the plans have to contain between them (both test modules assert the union)
FEATURES = (
    "order:conv_first", "order:join_last", "order:strided_pair", "bits:recorded_consumer_fp32", "bits:producer_cannot",
    "conv:image_s2", "conv:1x1", "conv:dilated", "conv:expanded_first", "conv:expanded_second", "conv:sum40",
    "bn:frozen_bias", "bn:frozen_nobias", "nobn:bias", "nobn:nobias", "bn:train_stats", "bn:train_nostats",
    "pool:k3s2p1_ceil_relu", "pool:k2s2_norelu", "pool:k3s1p1",
    "up2add:chain", "up2add:busy_relu_skip", "drop:train_pinned", "drop:eval_alias",
)


def build(name, seed):
    return dict(PLANS)[name](seed)


def modules(plan):
    out = []
    for op in plan.ops:
        if op.kind == "conv":
            out += op.convs + ([op.bn] if op.bn is not None else [])
        elif op.kind == "drop":
            out.append(op.module)
    return out


def to_device(plan, device):
    """Moves the plan's modules (Parameter objects stay the same) and the pinned dropout masks."""
    for m in modules(plan):
        m.to(device)
        if getattr(m, "keep_mask", None) is not None:
            m.keep_mask = m.keep_mask.to(device)
    return plan


# ---------------------------------------------------------------------------------------------------------------
# the float64 / ATen-fp32 runs both test modules share (computed once per plan and seed, never modified)
# ---------------------------------------------------------------------------------------------------------------
def backward(ref, plan, grad_out):
    out = ref.acts[plan.output]
    out.backward(grad_out.detach().cpu().to(out.dtype))
    return ref


_free = {}


def free_runs(name, seed):
    """(plan, x, grad_out, features, rec64, ref64, rec32, ref32): the free-running float64 and ATen float32 passes (each with its
    own ReLU pattern) of PLANS[name] at `seed`, backward included; cached."""
    key = (name, seed)
    if key not in _free:
        plan, x, gout, feats = build(name, seed)
        rec64, rec32 = RecordingRelu(), RecordingRelu()
        ref64 = backward(run_reference(plan, x, torch.float64, rec64), plan, gout)
        ref32 = backward(run_reference(plan, x, torch.float32, rec32), plan, gout)
        _free[key] = (plan, x, gout, feats, rec64, ref64, rec32, ref32)
    return _free[key]


def masked_run(plan, x, grad_out, masks):
    """The float64 pass (backward included) under a given ReLU pattern (CPU bool masks, in the order of relu_slots)."""
    from oracle.nets_ref import MaskedRelu
    return backward(run_reference(plan, x, torch.float64, MaskedRelu(masks)), plan, grad_out)


_aten = {}


def aten_errors(name, seed):
    """rel_err(ATen fp32, float64 under ATen's own ReLU pattern) of every activation ("a", slot), slot gradient ("g", slot) and
    parameter gradient ("p", index): the yardstick's right-hand side; cached."""
    from conftest import rel_err
    key = (name, seed)
    if key not in _aten:
        plan, x, gout, feats, rec64, ref64, rec32, ref32 = free_runs(name, seed)
        r64 = masked_run(plan, x, gout, [z > 0 for z in rec32.z])
        errs = {}
        for op in plan.ops:
            errs["a", op.dst] = rel_err(ref32.acts[op.dst], r64.acts[op.dst])
            errs["g", op.dst] = rel_err(ref32.grad_at[op.dst].grad, r64.grad_at[op.dst].grad)
        for j, (p32, p64) in enumerate(zip(ref32.params, r64.params)):
            errs["p", j] = rel_err(p32.grad, p64.grad)
            errs["p_abs", j] = float((p32.grad.double() - p64.grad).abs().max())
        _aten[key] = errs
    return _aten[key]


def flip_budget(plan, z64, masks, who):
    """The condition of test_resnet101_gradients_fp64_arbitration: an fp32 pattern differs from the float64 one on at most 1e-4 of
    the ReLU units, and every such unit has |z64| <= 1e-5 of its layer's max."""
    total = flips = 0
    worst = 0.0
    assert len(z64) == len(masks)
    for z, m in zip(z64, masks):
        d = (z > 0) != m.cpu()
        total += z.numel()
        flips += int(d.sum())
        if d.any():
            worst = max(worst, float(z[d].abs().max() / z.abs().max()))
    print("{}: {} ReLU units, {} flipped against float64 (worst |z|/max {:.2e})".format(who, total, flips, worst))
    assert flips <= 1e-4 * total and worst <= 1e-5, (who, flips, total, worst)
