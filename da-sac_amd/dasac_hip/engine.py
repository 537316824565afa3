"""Fused forward/backward executor for the segmentation backbones.

A network (`models.deeplabv2`, `models.fcn`) describes itself once as a flat *plan* of fused ops
over numbered activation slots; this module runs the plan forward and -- hand-written, no autograd
tape inside the backbone -- backward, calling only the C-ABI kernels of libdasac_hip.so:

  ConvOp   implicit-GEMM convolution with the frozen-BN scale/shift (or bias), residual add and ReLU
           in the epilogue ("ABN": conv+BN+ReLU fused).  Several branches (ASPP) are one contraction.
           Backward: channel sums (d beta), split-K weight-gradient GEMM (+ the d gamma dot term),
           data-gradient GEMM whose epilogue accumulates into the producer's gradient and applies the
           producer's ReLU mask -- so no stand-alone elementwise pass exists in the backbone.
  PoolOp   max pooling with the ReLU backward of its producer folded into the gradient routing.
  Up2AddOp FCN-8s skip fusion: up_x2(a) + b.          ScaleOp: Dropout2d with an explicit mask.

The whole plan is exposed to PyTorch as ONE autograd.Function (inputs: image + all parameters), so
DistributedDataParallel sees ordinary parameter gradients.

`Engine.probe` (None by default; `driver.activation_probe` attaches one) turns a forward into a probed one: every activation
is kept until the end of the pass and one dasac_activation_stats call reduces them per channel and sample segment.
"""
import torch

from . import ops
from . import lib as L


class ConvOp:
    kind = "conv"

    def __init__(self, src, dst, convs, bn, relu, res):
        c0 = convs[0]
        self.src, self.dst, self.res, self.relu = src, dst, res, bool(relu)
        self.convs, self.bn = list(convs), bn
        assert all(c.stride == c0.stride and c.in_channels == c0.in_channels and c.out_channels == c0.out_channels
                   and c.groups == 1 for c in convs)
        assert c0.stride[0] == c0.stride[1]
        branches = []
        for c in convs:
            assert c.dilation[0] == c.dilation[1] and c.padding[0] == c.padding[1]
            branches.append((c.kernel_size[0], c.kernel_size[1], c.dilation[0], c.padding[0]))
        self.spec = ops.ConvSpec(c0.in_channels, c0.out_channels, branches, c0.stride[0])
        self.has_bias = c0.bias is not None
        assert bn is None or len(convs) == 1
        # few output channels x many taps (ASPP): evaluate as dense 1x1 GEMMs over taps*Cp channels
        self.expanded = ops.ExpandedConv(self.spec) if (len(convs) > 1 and c0.out_channels <= 32 and c0.stride[0] == 1) else None

    def owner_groups(self):
        """(module, attribute) of every parameter in three groups: weights, biases, BN affine (gamma, beta)."""
        return ([(c, "weight") for c in self.convs],
                [(c, "bias") for c in self.convs] if self.has_bias else [],
                [(self.bn, "weight"), (self.bn, "bias")] if self.bn is not None else [])

    def owners(self):
        """(module, attribute) of every parameter, in the order of params()."""
        w, b, bn = self.owner_groups()
        return w + b + bn

    def name_index_groups(self):
        """Names the three groups of `pidx` (the engine's index of every parameter, in the order of owners())."""
        it = iter(self.pidx)
        self.w_idx, self.b_idx, self.bn_idx = ([next(it) for _ in group] for group in self.owner_groups())

    def params(self):
        return [getattr(m, a) for m, a in self.owners()]

    def geometry(self):
        return tuple((c.kernel_size, c.dilation, c.padding, c.stride, c.bias is not None) for c in self.convs)

    @property
    def frozen_bn(self):
        return self.bn is not None and not self.bn.training

    @property
    def refreshable(self):
        """Single-branch, non-expanded: the whole-network refresh (Engine.refresh) rebuilds its fold and its packs."""
        return self.expanded is None and len(self.convs) == 1

    def inputs(self):
        return [self.src] + ([self.res] if self.res is not None else [])

    def tensors(self, c, h, w):
        """(channels, height, width) of every tensor a forward over a [c, h, w] input creates; the output last."""
        oh, ow = self.spec.out_hw(h, w)
        return ([(self.expanded.E, oh, ow)] if self.expanded is not None else []) + [(self.spec.cout, oh, ow)]

    def forward(self, eng, i, saved, keep):
        acts, spec = saved["acts"], self.spec
        xin = acts[self.src]
        Nb, _, H, W = xin.shape
        if self.expanded is not None:
            _, bias_sum, _ = eng.fold(self)
            return self.expanded.forward(xin, eng.packed(self, False), eng.table(self, H, W, False, xin.device), bias_sum)
        OH, OW = spec.out_hw(H, W)
        out = torch.empty((Nb, spec.cout, OH, OW), dtype=torch.float32, device=xin.device)
        res = None if self.res is None else acts[self.res]
        if self.bn is not None and self.bn.training:
            # batch-statistics BN (baseline / AdaBN mode): raw conv, then stats -> normalise(+res)(+ReLU)
            cb = self.convs[0].bias.detach() if self.has_bias else None
            # the GEMM epilogue leaves the per-tile channel sums / sums of squares next to z: no statistics pass over z
            ts = ops.tile_stats_buffer(Nb, spec.cout, OH, OW, xin.device) if ops.stats_ok(spec.cout, spec.cin) else None
            z = ops.conv_gemm(xin, eng.packed(self, False, None), eng.table(self, H, W, False, xin.device), out, (OH, OW),
                              spec.stride, spec.cout, spec.K, 1, cb, None, None, False, stats=ts)
            out, stats = ops.bn_train_forward(z, self.bn, res, self.relu, tile_stats=ts)
            if keep:
                saved["aux"][i] = (z, stats)
            return out
        scale, shift, _ = eng.fold(self)
        bits = None
        if keep and self.relu and eng._bits_wanted[self.dst] and ops.bits_ok(spec.cout, spec.cin):
            bits = ops.ReluBits(Nb, spec.cout, OH, OW, xin.device)
            saved["bits"][self.dst] = bits
        form = ops.winograd_form(spec, False, Nb, H, W, keep) if res is None else None
        if form is not None:
            # wide dilated 3x3: F(4x4,3x3) on a route of ops.WINOGRAD4_ROUTES (no-grad passes of layer4's and layer3's conv2 on maps of two
            # whole 4x4 tiles per phase), else F(2x2,3x3) (layer4 conv2), around one batched launch of the 1x1 point GEMMs
            return form.conv(xin, eng.winograd_filter(self, False, scale, form), out, spec.branches[0][2], shift, self.relu, bits_out=bits)
        return ops.conv_gemm(xin, eng.packed(self, False, scale), eng.table(self, H, W, False, xin.device), out, (OH, OW),
                             spec.stride, spec.cout, spec.K, 1, shift, res, None, self.relu, bits_out=bits)

    def backward(self, eng, bp, i, dz):
        """(a) parameter gradients, (b) data gradient into g[src], masked with the producer's ReLU pattern by the last consumer,
        (c) residual hand-off and sink.done.  The expanded conv differs in the `ops` calls of (a) and (b) only."""
        spec, ex = self.spec, self.expanded
        xin = bp.acts[self.src]
        H, W = xin.shape[2:]
        dy_out = dz                       # gradient w.r.t. the op output (what a residual input receives)
        if ex is not None:
            d = ex.scatter(dz)
            self._param_grads_expanded(eng, bp, d, dz, xin)
        else:
            dz, scale = self._param_grads(eng, bp, i, dz, xin)
        if self.src != 0:
            relu = bp.arrive(self.src)
            if ex is not None:
                mask = bp.relu_pattern(self.src, spec.cin, ex.E) if relu else None
                bp.g[self.src] = ex.dgrad(d, eng.packed(self, True), eng.table(self, H, W, True, dz.device), (H, W),
                                          res=bp.g.get(self.src), mask=mask)
            else:
                mask = (bp.relu_pattern(self.src, spec.cin, spec.cout) if spec.stride == 1 else bp.acts[self.src]) if relu else None
                OH, OW = dz.shape[2:]
                wino_ok = bp.g.get(self.src) is None and (mask is None or isinstance(mask, ops.ReluBits))
                form = ops.winograd_form(spec, True, dz.shape[0], OH, OW, True) if wino_ok else None
                if form is not None:
                    dx = torch.empty((dz.shape[0], spec.cin, H, W), dtype=torch.float32, device=dz.device)
                    bp.g[self.src] = form.conv(dz, eng.winograd_filter(self, True, scale, form), dx, spec.branches[0][2], mask_bits=mask)
                else:
                    bp.g[self.src] = ops.conv_dgrad(spec, dz, None, (H, W), scale=scale, res=bp.g.get(self.src), mask=mask,
                                                    table=eng.table(self, OH, OW, True, dz.device),
                                                    packed=eng.packed(self, True, scale))
        if self.res is not None:
            bp.join(self.res, dy_out)
        if bp.sink is not None:
            bp.sink.done([j for j in self.pidx if bp.need[j]])

    def _param_grads_expanded(self, eng, bp, d, dz, xin):
        need = bp.need
        if any(need[j] for j in self.w_idx):
            bp.store(self.w_idx, self.expanded.wgrad(d, xin, [c.weight.detach() for c in self.convs],
                                                     eng.table(self, xin.shape[2], xin.shape[3], False, xin.device),
                                                     outs=[bp.dest(j) for j in self.w_idx]))
        if any(need[j] for j in self.b_idx):
            bp.fan_out(self.b_idx, ops.channel_sums(dz, out=bp.sums_dest(self.b_idx, True, self.spec.cout, dz.device)))

    def _param_grads(self, eng, bp, i, dz, xin):
        """Returns (gradient w.r.t. the conv output, the frozen BN's scale or None): what the data gradient starts from."""
        spec, need, grads = self.spec, bp.need, bp.grads
        w_idx, b_idx, bn_idx = self.w_idx, self.b_idx, self.bn_idx
        train_bn = i in bp.aux
        want_bias = any(need[j] for j in b_idx)
        want_bn = any(need[j] for j in bn_idx)
        if train_bn:
            z, stats = bp.aux.pop(i)
            dz, dg, db = ops.bn_train_backward(dz, z, stats, self.bn.weight.detach(), want_params=want_bn,
                                               outs=(bp.dest(bn_idx[0]), bp.dest(bn_idx[1])) if want_bn else (None, None))
            del z
            if want_bn:
                bp.store(bn_idx, (dg, db))
            scale, invstd, want_bn = None, None, False        # what is left of BN below is the frozen one's
        else:
            scale, _, invstd = eng.fold(self)
        bias_is_sums = train_bn or self.bn is None            # the bias gradient IS the channel sums of dz
        sums, dot = None, None
        if any(need[j] for j in w_idx) or want_bn:
            if want_bn:
                dot = bp.dot_slice(spec, dz.device)
            if want_bn or want_bias:      # channel sums ride along with the wgrad kernel
                sums = bp.sums_dest(b_idx, want_bias and bias_is_sums, spec.cout, dz.device)
            form = ops.winograd_wgrad_form(spec, xin.shape[0], xin.shape[2], xin.shape[3])
            if form is not None:
                # wide dilated 3x3 (conv2 of layer3 and layer4): the adjoint of the forward's Winograd form, 2.25 x fewer multiplies as
                # F(2x2,3x3), 1.71 x fewer again as F(4x4,3x3) on maps of at least two whole 4x4-output tiles per phase
                bp.store(w_idx, [form.wgrad(spec, dz, xin, self.convs[0].weight.detach(), scale=scale, dot=dot, sum_dz=sums,
                                            out=bp.dest(w_idx[0]))])
            else:
                bp.store(w_idx, ops.conv_wgrad(spec, dz, xin, [c.weight.detach() for c in self.convs], scale=scale, dot=dot,
                                               table=eng.table(self, xin.shape[2], xin.shape[3], False, xin.device, wgrad=True),
                                               sum_dz=sums, outs=[bp.dest(j) for j in w_idx]))
        elif want_bias:
            sums = ops.channel_sums(dz, out=bp.sums_dest(b_idx, bias_is_sums, spec.cout, dz.device))
        if bias_is_sums:
            if want_bias:
                bp.fan_out(b_idx, sums)
        elif want_bn or want_bias:
            cb = self.convs[0].bias.detach() if self.has_bias else None
            dg, db, dcb = ops.bn_param_grads(dot, sums, self.bn.running_mean, invstd, scale, cb,
                                             want_gamma=want_bn, want_beta=want_bn, want_bias=want_bias,
                                             outs=(bp.dest(bn_idx[0]) if want_bn else None, bp.dest(bn_idx[1]) if want_bn else None,
                                                   bp.dest(b_idx[0]) if want_bias else None))
            if want_bn:
                bp.store(bn_idx, (dg, db))
            if want_bias:
                grads[b_idx[0]] = dcb
        return dz, scale


class PoolOp:
    kind = "pool"
    relu = False

    def __init__(self, src, dst, k, s, p, ceil_mode):
        self.src, self.dst, self.k, self.s, self.p, self.ceil = src, dst, k, s, p, bool(ceil_mode)

    def params(self):
        return []

    def inputs(self):
        return [self.src]

    def tensors(self, c, h, w):
        return [(c, ops.pool_out(h, self.k, self.s, self.p, self.ceil), ops.pool_out(w, self.k, self.s, self.p, self.ceil))]

    def forward(self, eng, i, saved, keep):
        out, arg = ops.maxpool_fwd(saved["acts"][self.src], self.k, self.s, self.p, self.ceil)
        if keep:
            saved["aux"][i] = arg
        return out

    def backward(self, eng, bp, i, dz):
        assert eng.consumers[self.src] == 1
        bp.g[self.src] = ops.maxpool_bwd(dz, bp.acts[self.dst], bp.aux[i], bp.acts[self.src].shape[2:], self.k, self.s, self.p,
                                         relu_mask=bp.arrive(self.src))


class Up2AddOp:
    kind = "up2add"
    relu = False

    def __init__(self, src, skip, dst):
        self.src, self.skip, self.dst = src, skip, dst

    def params(self):
        return []

    def inputs(self):
        return [self.src, self.skip]

    def tensors(self, c, h, w):
        return [(c, 2 * h, 2 * w)]

    def forward(self, eng, i, saved, keep):
        xin = saved["acts"][self.src]
        up, _, _ = ops.upsample_softmax(xin, (2 * xin.shape[2], 2 * xin.shape[3]))
        return ops.add(up, saved["acts"][self.skip], out=up)

    def backward(self, eng, bp, i, dz):
        bp.join(self.skip, dz)
        bp.join(self.src, ops.upsample_bwd(dz, bp.acts[self.src].shape[2:]))


class ScaleOp:
    """Dropout2d(p) in train mode: y = x * keep/(1-p) per (n, c) plane."""
    kind = "drop"
    relu = False

    def __init__(self, src, dst, module):
        self.src, self.dst, self.module = src, dst, module

    def params(self):
        return []

    def inputs(self):
        return [self.src]

    def tensors(self, c, h, w):
        return [(c, h, w)]

    def forward(self, eng, i, saved, keep):
        xin, m = saved["acts"][self.src], self.module
        if not (m.training and m.p > 0):
            return xin
        # ATen feature dropout (fcn.py:52,56): per (n, c) plane noise = bernoulli(1-p)/(1-p).  A test can pin
        # the draw by setting `module.keep_mask` ([B,C], already divided by 1-p) -- parity needs equal masks.
        keep_mask = getattr(m, "keep_mask", None)
        if keep_mask is None:
            keep_mask = ops.dropout_planes(xin.shape[0], xin.shape[1], m.p, xin.device)
        assert tuple(keep_mask.shape) == tuple(xin.shape[:2]) and keep_mask.is_cuda
        if keep:
            saved["aux"][i] = keep_mask
        return ops.scale_planes(xin, keep_mask)

    def backward(self, eng, bp, i, dz):
        m = bp.aux.get(i)
        bp.join(self.src, dz if m is None else ops.scale_planes(dz, m))


class Plan:
    """Builder used by the model classes."""

    def __init__(self):
        self.ops, self.n_slots, self.output = [], 1, None     # slot 0 = input image

    def _new(self):
        self.n_slots += 1
        return self.n_slots - 1

    def conv(self, src, conv, bn=None, relu=False, res=None):
        dst = self._new()
        self.ops.append(ConvOp(src, dst, [conv], bn, relu, res))
        return dst

    def conv_sum(self, src, convs):
        dst = self._new()
        self.ops.append(ConvOp(src, dst, list(convs), None, False, None))
        return dst

    def maxpool(self, src, k, s, p=0, ceil_mode=False):
        dst = self._new()
        self.ops.append(PoolOp(src, dst, k, s, p, ceil_mode))
        return dst

    def up2_add(self, src, skip):
        dst = self._new()
        self.ops.append(Up2AddOp(src, skip, dst))
        return dst

    def dropout2d(self, src, module):
        dst = self._new()
        self.ops.append(ScaleOp(src, dst, module))
        return dst

    def finish(self, output):
        self.output = output
        return self


def _ver(t):
    return (t.data_ptr(), t._version)


_tensor_data = torch.Tensor.data          # the C-level `data` descriptor of every tensor


class TrackedParameter(torch.nn.Parameter):
    """The class an Engine gives the parameters of its plan (`p.__class__`: the objects, their storage and every reference to
    them stay what they are; isinstance(p, nn.Parameter) holds; pickling and state_dict give plain tensors / Parameters).

    `p.data` is an alias of p with a version counter of its own, so `p.data.mul_(...)` -- the in-place update of much older
    PyTorch code -- moves nothing that `_ver` reads and the cached packs and folds would outlive the values they were made from.
    Here reading or assigning `p.data` moves p's own counter: whoever asks for the alias is taken to write through it.  A reader
    costs one rebuild of that layer's caches, nothing else.  Not seen: a write through an alias taken BEFORE the last forward and
    kept, or through a raw pointer -- `ops.bump_versions` after those."""

    @property
    def data(self):
        torch.autograd.graph.increment_version(self)
        return _tensor_data.__get__(self, type(self))

    @data.setter
    def data(self, value):
        _tensor_data.__set__(self, value)
        torch.autograd.graph.increment_version(self)


def _keep_multi_tensor_optimisers():
    """torch.optim takes its multi-tensor (foreach / fused) implementations only for the tensor classes on this list (Tensor and
    nn.Parameter), by exact type; a class that behaves like them registers itself there (as torch's own DTensor does).  Without
    it torch.optim.Adam / SGD fall back to one launch series per parameter -- slower, and rounded differently."""
    from torch.optim.optimizer import _foreach_supported_types as types
    if TrackedParameter not in types:
        types.append(TrackedParameter)


_keep_multi_tensor_optimisers()


def _fold_key(op):
    """What a cached fold of `op` was computed from: the frozen BN's vectors (and the conv bias), or the branch biases."""
    if op.bn is None:
        return tuple(_ver(c.bias) for c in op.convs)
    bn, cb = op.bn, (op.convs[0].bias if op.has_bias else None)
    return (_ver(bn.weight), _ver(bn.bias), _ver(bn.running_mean), _ver(bn.running_var), None if cb is None else _ver(cb))


def _pack_key(op, scale):
    """What a cached packed operand of `op` was computed from: the weights, the scale folded into them, the arithmetic."""
    return tuple(_ver(c.weight) for c in op.convs) + ((_ver(scale),) if scale is not None else ()) + (ops.PRECISION,)


def _copy_into(out, src):
    """A second parameter that receives the same gradient (the bias of every ASPP branch): its own tensor."""
    if out is None:
        return src.clone()
    out.view(-1).copy_(src.view(-1))
    return out


class _BackwardPass:
    """State of one Engine.backward, shared by the ops' backward methods: activation gradients `g` by slot, the consumers of
    each slot still `pending`, the parameter gradients and where they are written."""

    def __init__(self, eng, saved, grad_out, need, sink):
        self.eng, self.need, self.sink = eng, need, sink
        self.acts, self.aux, self.bits = saved["acts"], saved["aux"], saved.get("bits", {})
        self.grads = [None] * len(eng.params)
        g_out, out_op = grad_out.contiguous(), eng.producer[eng.plan.output]
        if out_op is not None and out_op.relu:
            # nobody consumes the plan's output inside the plan: a ReLU that closes it is differentiated here
            g_out = ops.relu_mask(g_out, self.acts[eng.plan.output])
        self.g = {eng.plan.output: g_out}
        # the d-gamma dot terms of all frozen-BN convs are slices of ONE vector: [dot_rows, cout] partial rows per layer, every
        # element written by the weight-gradient finish and added in a fixed order by bn_param_grads (no atomics, no fill)
        self.dot_pool, self.dot_used = None, 0
        self.dot_total = sum(ops.dot_rows(op.spec) * op.spec.cout for op in eng._convs if op.bn is not None and op.expanded is None)
        self.pending = list(eng.consumers)
        self.pending[eng.plan.output] = 0

    def dest(self, j):
        return self.sink.alloc(j) if (self.sink is not None and self.need[j]) else None

    def store(self, idx, tensors):
        for j, t in zip(idx, tensors):
            if self.need[j]:
                self.grads[j] = t

    def sums_dest(self, b_idx, is_bias_grad, cout, device):
        """Per-channel sums of dz: they ARE the bias gradient of a conv without (or with batch-statistics) BN -- then they
        are written straight to that gradient's destination -- and an intermediate of bn_param_grads otherwise."""
        wanted = [j for j in b_idx if self.need[j]]
        out = self.dest(wanted[0]) if (is_bias_grad and wanted) else None
        return torch.empty(cout, dtype=torch.float32, device=device) if out is None else out.view(cout)

    def fan_out(self, b_idx, sums):
        """Every branch bias sees the same gradient."""
        wanted = [j for j in b_idx if self.need[j]]
        for n_, j in enumerate(wanted):
            self.grads[j] = sums if n_ == 0 else _copy_into(self.dest(j), sums)

    def dot_slice(self, spec, device):
        if self.dot_pool is None:
            self.dot_pool = torch.empty(self.dot_total, dtype=torch.float32, device=device)
        rows = ops.dot_rows(spec)
        dot = self.dot_pool[self.dot_used:self.dot_used + rows * spec.cout].view(rows, spec.cout)
        self.dot_used += rows * spec.cout
        return dot

    def relu_pattern(self, slot, M, Cx):
        """What the data-gradient epilogue (output M channels, gathering Cx) masks with: the producer's bit mask when the
        forward recorded one and this GEMM has the bit-mask variant, else the producer's fp32 output."""
        b = self.bits.get(slot)
        return b if (b is not None and ops.bits_ok(M, Cx)) else self.acts[slot]

    def arrive(self, slot):
        """One more consumer of `slot` delivers its gradient.  True when it is the last one and the slot's producer ends in
        a ReLU: that consumer applies the pattern."""
        self.pending[slot] -= 1
        p = self.eng.producer[slot]
        return self.pending[slot] == 0 and p is not None and p.relu

    def join(self, slot, t):
        """A pass-through consumer (residual / skip) hands its gradient to `slot`."""
        relu = self.arrive(slot)
        cur = self.g.get(slot)
        t = t if cur is None else ops.add(cur, t)
        self.g[slot] = ops.relu_mask(t, self.acts[slot]) if relu else t


class Engine:
    """Executes a Plan.  Keeps per-layer caches of gather tables (by spatial size) and of packed
    weights / folded BN vectors (invalidated by the parameters' version counters)."""

    def __init__(self, plan):
        self.plan = plan
        self.params = []
        for op in plan.ops:
            op.pidx = list(range(len(self.params), len(self.params) + len(op.params())))
            self.params += op.params()
        for p in self.params:
            if type(p) is torch.nn.Parameter:      # (another subclass keeps its class: its `.data` writes need bump_versions)
                p.__class__ = TrackedParameter
        self._convs =[op for op in plan.ops if isinstance(op, ConvOp)]      # the ops that own parameters and caches
        self._owners, self._geometry = [], []
        for op in self._convs:
            op.name_index_groups()
            self._owners += op.owners()
            self._geometry.append((op, op.geometry()))
        self.consumers = [0] * plan.n_slots
        self.producer = [None] * plan.n_slots
        self.last_use = [0] * plan.n_slots
        first_consumer = {}
        for i, op in enumerate(plan.ops):
            self.producer[op.dst] = op
            for s in op.inputs():
                self.consumers[s] += 1
                self.last_use[s] = i
                first_consumer.setdefault(s, op)
        self.last_use[plan.output] = len(plan.ops)
        self._check_supported()
        self._tables, self._packs, self._folds = {}, {}, {}
        self._refresh, self._fold_bufs = {}, {}
        self.probe, self._layouts = None, {}      # activation tables: off unless a probe is attached (Engine.forward)
        self.tap = None                           # (op index, sink): hands ONE activation of a forward to the sink (Engine.forward)
        # A ReLU conv's pattern is recorded as bits when the backward pass will apply it in a stride-1 data-gradient epilogue:
        # the mask is applied by the consumer that finishes LAST in backward order = the slot's FIRST consumer in plan order.
        self._bits_wanted = [False] * plan.n_slots
        for op in self._convs:
            if first_consumer[op.src] is op and op.spec.stride == 1 and op.src != 0:
                self._bits_wanted[op.src] = True

    def _check_supported(self):
        """Refuses, before any kernel runs, the plan shapes the backward pass has no code for."""
        plan = self.plan

        def refuse(i, op, why):
            raise ValueError("dasac_hip engine: op {} ({} {} -> slot {}) {}".format(
                i, op.kind, "slots {}".format(op.inputs()) if len(op.inputs()) > 1 else "slot {}".format(op.src), op.dst, why))

        live = {plan.output}
        for i in range(len(plan.ops) - 1, -1, -1):
            op = plan.ops[i]
            if op.dst not in live:
                refuse(i, op, "never reaches the plan's output (slot {}): the backward pass would wait for its gradient".format(plan.output))
            live.update(op.inputs())
        for i, op in enumerate(plan.ops):
            if isinstance(op, PoolOp) and self.consumers[op.src] != 1:
                refuse(i, op, "is a pool whose source has {} consumers: the pool's backward writes its source's gradient "
                              "alone".format(self.consumers[op.src]))
            if isinstance(op, ConvOp) and op.spec.stride != 1 and op.src != 0 and \
                    (op.spec.taps != 1 or op.spec.branches[0][3] != 0):
                refuse(i, op, "is a stride-{} conv with {} taps (padding {}) that does not read the input image: the strided "
                              "data gradient exists for unpadded 1x1 convs only".format(op.spec.stride, op.spec.taps, op.spec.branches[0][3]))

    def stale(self):
        """True when a module no longer holds the Parameter objects (or conv geometry) this engine captured:
        `load_state_dict(assign=True)`, `m.weight = nn.Parameter(...)`, parametrizations, edited dilation/padding.
        In-place updates (optimisers, copy_, `p.data.mul_`: TrackedParameter) are NOT stale -- the caches follow the version
        counters.  A write through a raw pointer, or into a BN buffer's `.data`, moves no counter: `ops.bump_versions` after it."""
        return any(getattr(m, a) is not p for (m, a), p in zip(self._owners, self.params)) or \
            any(op.geometry() != geo for op, geo in self._geometry)

    # ---------------------------------------------------------------- caches
    def table(self, op, h, w, transposed, device, wgrad=False):
        """Gather table (of the 1x1 GEMM over the expanded channels for an expanded conv); the forward / data-gradient GEMMs
        may use the chunk-major K order, the weight gradient always the tap-major one."""
        spec = op.spec if op.expanded is None else op.expanded.spec1
        order = 0 if wgrad else ops.gemm_order(spec, transposed)
        key = (id(op), h, w, transposed, device.index, order)
        t = self._tables.get(key)
        if t is None:
            t = ops.conv_table(spec, h, w, transposed, device, order)
            self._tables[key] = t
        return t

    @staticmethod
    def _cached(store, slot, key, build, *args):
        """store[slot] = (key, value, args): the value when its key still holds, else build(old value or None, *args) --
        a rebuild writes into the old buffer.  `args` stay alive with the entry (a scale vector's address is part of its key)."""
        ent = store.get(slot)
        if ent is None or ent[0] != key:
            ent = store[slot] = (key, build(None if ent is None else ent[1], *args), args)
        return ent[1]

    def fold(self, op):
        """(scale, shift, invstd) of the frozen BN (plus conv bias), or (None, bias_sum, None)."""
        if op.bn is None and (not op.has_bias or len(op.convs) == 1):
            return None, (op.convs[0].bias.detach() if op.has_bias else None), None
        return self._cached(self._folds, id(op), _fold_key(op), self._build_fold, op)

    @staticmethod
    def _build_fold(old, op):
        if op.bn is None:
            acc = op.convs[0].bias.detach()
            for c in op.convs[1:]:
                acc = ops.add(acc, c.bias.detach())
            return None, acc, None
        bn = op.bn
        return ops.bn_fold(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps,
                           op.convs[0].bias.detach() if op.has_bias else None)

    def packed(self, op, transposed, scale=None):
        """Packed weight operand of the forward (transposed: the data-gradient) GEMM, `scale` folded in."""
        return self._cached(self._packs, (id(op), transposed), _pack_key(op, scale), self._build_pack, op, transposed, scale)

    @staticmethod
    def _build_pack(old, op, transposed, scale):
        weights = [c.weight.detach() for c in op.convs]
        if op.expanded is not None:
            return op.expanded.pack(weights, transposed, out=old)
        return ops.conv_pack(op.spec, weights, transposed, scale, out=old, order=ops.gemm_order(op.spec, transposed))

    def winograd_filter(self, op, transposed, scale, form):
        """Transformed filter (the packed point matrices of `form`, ops.F2 or ops.F4) of a conv routed to the Winograd path: cached
        like `packed`, on the same key -- rebuilt when the weights or the folded scale change, so a teacher's stays put between EMA
        updates.  The two forms have slots of their own (a layer may run both, on maps of different sizes)."""
        return self._cached(self._packs, (id(op), transposed, form.name), _pack_key(op, scale), self._build_winograd_filter, op, transposed,
                            scale, form)

    @staticmethod
    def _build_winograd_filter(old, op, transposed, scale, form):
        return form.filter(op.spec, op.convs[0].weight.detach(), transposed, scale, out=old)

    def largest_tensor_bytes(self, Nb, H, W):
        """Bytes of the largest activation (or expanded-conv intermediate) a pass over an [Nb, *, H, W] input creates.  The conv
        kernels address tensors through buffer descriptors with unsigned 32-bit byte offsets: every one of them has to stay below 4 GiB
        (4 GiB - 4 KiB; rounds 1-4: 2 GiB)."""
        shapes = {0: (None, H, W)}
        biggest = 0
        for op in self.plan.ops:
            made = op.tensors(*shapes[op.src])
            shapes[op.dst] = made[-1]
            biggest = max([biggest] + [Nb * (c or 1) * h * w * 4 for c, h, w in made])
        return biggest

    # ---------------------------------------------------------------- whole-network refresh of folds / packs
    def _refresh_plan(self, device, transposed):
        """Device job tables for `ops.refresh_network`: one fold job per frozen-BN conv, one pack job per (conv, layout) for
        every single-branch, non-expanded conv.  Output buffers are persistent (their pointers sit in the tables)."""
        # batch-statistics BN layers (baseline / AdaBN mode) fold nothing into the weights: their convs are packed un-scaled
        bn_mode = tuple(bool(op.bn is not None and op.bn.training) for op in self._convs)
        key = (device.index, bool(transposed), bn_mode)
        plan = self._refresh.get(key)
        if plan is not None and plan["ptrs"] == self._refresh_ptrs():
            return plan
        lib = L.load()
        fold_jobs, pack_jobs, fold_ops, pack_slots = [], [], [], []
        for op in self._convs:
            if not op.refreshable:
                continue
            scale = None
            if op.frozen_bn:
                ent = self._fold_bufs.get(id(op))
                if ent is None:
                    C = op.spec.cout
                    ent = tuple(torch.empty(C, dtype=torch.float32, device=device) for _ in range(3))
                    self._fold_bufs[id(op)] = ent
                scale = ent[0]
                cb = op.convs[0].bias if op.has_bias else None
                fold_jobs.append((op.bn.weight, op.bn.bias, op.bn.running_mean, op.bn.running_var, cb, ent, op.bn.eps, op.spec.cout))
                fold_ops.append(op)
            for tr in ((False, True) if transposed else (False,)):
                M = op.spec.cin if tr else op.spec.cout
                K = op.spec.Kt if tr else op.spec.K
                slot = (id(op), tr)
                old = self._packs.get(slot)
                shape = (lib.dasac_conv_kpad(K), lib.dasac_conv_mpad(M))
                buf = old[1] if (old is not None and tuple(old[1].shape) == shape and not getattr(old[1], "dasac_x3", False)) else \
                    torch.empty(shape, dtype=torch.float32, device=device)
                buf.dasac_x3 = False
                pack_jobs.append((op.convs[0].weight, scale, buf, op.spec.cout, op.spec.cin, op.spec.taps, shape[1], shape[0], int(tr),
                                  ops.gemm_order(op.spec, tr)))
                pack_slots.append((slot, op, buf, scale))
        plan = {"ptrs": self._refresh_ptrs(), "fold_ops": fold_ops, "pack_slots": pack_slots,
                "tables": ops.build_refresh_tables(fold_jobs, pack_jobs, device)}
        self._refresh[key] = plan
        return plan

    def _refresh_ptrs(self):
        out = []
        for op in self._convs:
            out += [p.data_ptr() for p in op.params()]
            if op.bn is not None:
                out += [op.bn.running_mean.data_ptr(), op.bn.running_var.data_ptr()]
        return tuple(out)

    def refresh(self, device, transposed):
        """After an optimiser / EMA step every folded BN vector and every packed weight operand of the network is stale at
        once: rebuild them ALL in two launches (dasac_bn_fold_multi, dasac_conv_pack_multi) instead of one small launch per
        layer and layout as they are first used (~310 launches per student step).  Only when the whole network is stale and
        runs fp32 -- partial invalidations and the split-bf16 operands keep the per-layer path.  Convolutions in front of a
        batch-statistics BN (round 4: cfg-2 spent 1.5 ms per step in 228 per-layer pack launches) are packed un-scaled by the
        same launch; only frozen BNs have a fold job."""
        if ops.PRECISION != "fp32":
            return
        convs = [op for op in self._convs if op.refreshable]
        if len(convs) < 8:
            return
        # stale = the cached key no longer matches the parameters' version counters
        for op in convs:                                     # all-or-nothing: the first fresh layer ends the check
            ent = self._packs.get((id(op), False))
            sc = self._folds.get(id(op)) if op.frozen_bn else None
            fresh_fold = (not op.frozen_bn) or (sc is not None and sc[0] == _fold_key(op))
            if fresh_fold and ent is not None and ent[0] == _pack_key(op, sc[1][0] if op.frozen_bn else None):
                # (the forward layout may have been refreshed alone by a no-grad pass -- AdaBN's target forward right after the
                # optimiser step: the data-gradient layout is then still stale, and one more launch beats 104 per-layer ones)
                ent_t = self._packs.get((id(op), True)) if transposed else ent
                if ent_t is not None and ent_t[0] == ent[0]:
                    return
        plan = self._refresh_plan(device, transposed)
        ops.refresh_network(plan["tables"])
        for op in plan["fold_ops"]:
            ent = self._fold_bufs[id(op)]
            ops.bump_versions([ent[0]])                      # the scale vector is part of the pack keys: it has new contents
            self._folds[id(op)] = (_fold_key(op), ent, None)
        for slot, op, buf, scale in plan["pack_slots"]:
            self._packs[slot] = (_pack_key(op, scale), buf, scale)

    # ---------------------------------------------------------------- forward
    def forward(self, x, keep):
        """Runs the plan.  keep=True retains what backward needs; returns (output, saved).

        With a `probe` attached (None by default: nothing below happens) every activation of the pass stays alive until its
        end -- on keep=False passes too, which then need the memory of a training pass instead of that of the two or three
        live slots -- and ONE dasac_activation_stats call over slot 0 (the input) and every op's output, in plan order, follows
        the last op on the launch stream.  `probe.append((table, layout, N, bounds))` receives the device table (fp64
        [n_segments, R, 6], ops.ACTIVATION_STATS_COLUMNS), the layout (`activation_layout`), the batch size and the segment
        bounds (`probe.bounds`: None, cut points, or a callable N -> bounds).  Nothing synchronises; `saved` is what it is
        without a probe.

        With a `tap` = (op index, sink) attached (None by default) `sink(tensor)` is called right after that op has produced its
        output (op index -1: with the input, before the first op; `tap_index` resolves a name).  No other activation is kept and
        `saved` is what it is without the tap."""
        L.require_gpu(x)
        self.refresh(x.device, transposed=keep)
        acts = {0: x}
        saved = {"acts": acts, "aux": {}, "bits": {}}
        probe, tap = self.probe, self.tap
        held = None if probe is None else [x]
        if tap is not None and tap[0] == -1:
            tap[1](x)
        for i, op in enumerate(self.plan.ops):
            acts[op.dst] = op.forward(self, i, saved, keep)
            if tap is not None and tap[0] == i:
                tap[1](acts[op.dst])
            if held is not None:
                held.append(acts[op.dst])
            if not keep:
                for s in op.inputs():
                    if self.last_use[s] == i and s != 0:
                        del acts[s]
        if held is not None:
            self._probe_pass(probe, held)
        return acts[self.plan.output], saved

    # ---------------------------------------------------------------- activation tables
    def activation_layout(self, shapes, names=None):
        """One entry per tensor of a probed pass -- slot 0, then every op's output in plan order -- for tensors of `shapes`
        ((C, H, W) each): dict(op (index, -1 for the input), slot, name, kind, C, H, W, relu (a ReLU closes it), row0 (its first
        table row)).  names: {conv module: name}, e.g. inverted `named_modules()`; a conv op is called by its module (the common
        dotted prefix of the branches for a multi-branch op), the other ops "pool@<slot>" / "up2add@<slot>" / "dropout@<slot>", the
        input "input".  A name that is missing or taken gets "@<slot>" appended: names are unique."""
        names = names or {}
        entries, row0, taken = [], 0, set()
        for j, (c, h, w) in enumerate(shapes):
            op = None if j == 0 else self.plan.ops[j - 1]
            slot = 0 if op is None else op.dst
            if op is None:
                name, kind = "input", "input"
            elif isinstance(op, ConvOp):
                parts = [names[m].split(".") for m in op.convs if m in names]
                common = []
                if len(parts) == len(op.convs):
                    for level in zip(*parts):
                        if any(p != level[0] for p in level):
                            break
                        common.append(level[0])
                name, kind = ".".join(common) or "conv@{}".format(slot), op.kind
            else:
                name, kind = "{}@{}".format("dropout" if op.kind == "drop" else op.kind, slot), op.kind
            if name in taken:
                name = "{}@{}".format(name, slot)
            taken.add(name)
            entries.append(dict(op=j - 1, slot=slot, name=name, kind=kind, C=int(c), H=int(h), W=int(w),
                                relu=bool(op is not None and op.relu), row0=row0))
            row0 += int(c)
        return entries

    def tap_index(self, name=None, names=None):
        """(op index for `tap`, the tensor's name).  `name`: one of the names `activation_layout` gives under `names` ({conv module:
        name}) -- "input" (index -1), a conv module's name, "pool@<slot>" ...; None: the tensor the classifier reads, i.e. the
        input of the conv that makes the coarsest scores -- from the plan's output back through the upsampled operand of every
        up2add (the 2048-channel layer4 output of the ResNet-101 DeepLab, fc7 of the VGG DeepLab, fc7 behind its Dropout2d op for FCN-8s).  An unknown name
        raises ValueError and lists the names."""
        layout = self.activation_layout([(0, 0, 0)] * (len(self.plan.ops) + 1), names)
        if name is None:
            slot = self.plan.output
            while isinstance(self.producer[slot], Up2AddOp):
                slot = self.producer[slot].src
            if self.producer[slot] is not None:
                slot = self.producer[slot].src
            entry = [e for e in layout if e["slot"] == slot][-1]
            return entry["op"], entry["name"]
        for e in layout:
            if e["name"] == name:
                return e["op"], e["name"]
        raise ValueError("no activation is called {!r}; the names are: {}".format(name, ", ".join(e["name"] for e in layout)))

    def _probe_pass(self, probe, held):
        N = held[0].shape[0]
        bounds = probe.bounds(N) if callable(probe.bounds) else probe.bounds
        shapes = tuple(tuple(t.shape[1:]) for t in held)
        plan = ops.activation_stats_plan(shapes, N, bounds)
        names = getattr(probe, "names", None)
        key = (shapes, id(names))
        ent = self._layouts.get(key)
        if ent is None:
            ent = self._layouts[key] = (names, self.activation_layout(shapes, names))      # (names held: its id stays its own)
        probe.append((plan.run(held), ent[1], N, plan.bounds))

    # ---------------------------------------------------------------- backward
    def backward(self, saved, grad_out, need, trace=None, sink=None):
        """grad_out: gradient w.r.t. the plan output.  need[i]: whether parameter i wants a gradient.
        Returns the list of parameter gradients (None where not needed).  `trace` (debug): dict that
        receives the finished activation gradient of every slot.

        `sink` (dasac_hip.parallel.GradSink or None): where parameter gradients are WRITTEN and who is told when a layer's
        are complete -- `sink.alloc(j)` returns the destination of parameter j (a slice of one flat reduction buffer),
        `sink.done(indices)` is called after each op, in backward order, so that a bucket's all-reduce can start while
        the layers below it are still being differentiated (DistributedDataParallel's overlap, train.py:104,133,232)."""
        bp = _BackwardPass(self, saved, grad_out, need, sink)
        for i in range(len(self.plan.ops) - 1, -1, -1):
            op = self.plan.ops[i]
            dz = bp.g.pop(op.dst, None)
            if dz is None:
                continue
            assert bp.pending[op.dst] == 0
            if trace is not None:
                trace[op.dst] = dz
            op.backward(self, bp, i, dz)
            bp.acts.pop(op.dst, None)      # the activation of this op's output is no longer needed
        return bp.grads


class _PlanFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, engine, sink, x, *params):
        keep = any(p.requires_grad for p in params)
        out, saved = engine.forward(x, keep)
        ctx.engine, ctx.sink = engine, sink
        ctx.saved = saved if keep else None
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.saved is None:
            raise RuntimeError("dasac_hip engine: the activations of this forward were already consumed by a backward pass "
                               "(retain_graph / a second backward through the same forward is not supported)")
        need = list(ctx.needs_input_grad[3:])
        sink = ctx.sink
        if sink is not None:
            grad_out = sink.begin(ctx.engine, need, grad_out)
        grads = ctx.engine.backward(ctx.saved, grad_out, need, sink=sink)
        if sink is not None:
            sink.finish()         # the launch stream waits for the outstanding bucket reductions: .grad is final for any consumer
        ctx.saved = None
        return (None, None, None) + tuple(grads)


def run_plan(engine, x, sink=None):
    """logits = plan(x); differentiable w.r.t. every parameter of the plan.  `sink`: see Engine.backward."""
    if torch.is_grad_enabled() and any(p.requires_grad for p in engine.params):
        return _PlanFunction.apply(engine, sink, x, *engine.params)
    out, _ = engine.forward(x, keep=False)
    return out


# --------------------------------------------------------------------------------------------------
# head functions with gradients
# --------------------------------------------------------------------------------------------------
class _Upsample(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, size):
        ctx.low = tuple(logits.shape[2:])
        up, _, _ = ops.upsample_softmax(logits, size)
        return up

    @staticmethod
    def backward(ctx, g):
        return ops.upsample_bwd(g, ctx.low), None


def upsample_bilinear(logits, size):
    """F.interpolate(logits, size, mode='bilinear', align_corners=True) (deeplabv2.py:217).  The result remembers the
    low-resolution tensor it came from, so that a loss on it can send its gradient straight there (`_CELossLow`)."""
    up = _Upsample.apply(logits, tuple(int(s) for s in size))
    up._dasac_low = (logits, up._version)      # valid only while `up` still holds U(logits): see _ce
    return up


class _SplitBatch(torch.autograd.Function):
    """x [B, ...] -> (x[:n], x[n:]) as two contiguous tensors sharing x's storage; backward writes the two gradients side by
    side into one buffer (a missing one is zero)."""

    @staticmethod
    def forward(ctx, x, n):
        ctx.n, ctx.shape = int(n), tuple(x.shape)
        return x.narrow(0, 0, ctx.n), x.narrow(0, ctx.n, x.shape[0] - ctx.n)

    @staticmethod
    def backward(ctx, ga, gb):
        ref = ga if ga is not None else gb
        g = torch.empty(ctx.shape, dtype=ref.dtype, device=ref.device)
        for part, grad in ((g.narrow(0, 0, ctx.n), ga), (g.narrow(0, ctx.n, ctx.shape[0] - ctx.n), gb)):
            if grad is None:
                part.zero_()
            else:
                part.copy_(grad)
        return g, None


def split_batch(x, n):
    return _SplitBatch.apply(x, n)


class _CELoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits_up, labels, class_weight, conf):
        loss, _, _ = ops.ce_loss(logits_up, labels, class_weight, conf)
        ctx.save_for_backward(logits_up, labels, class_weight, conf)
        return loss

    @staticmethod
    def backward(ctx, g):
        logits_up, labels, class_weight, conf = ctx.saved_tensors
        _, dl, _ = ops.ce_loss(logits_up, labels, class_weight, conf, want_grad=True, gscale=g.contiguous())
        return dl, None, None, None


class _CELossLow(torch.autograd.Function):
    """The same loss value as _CELoss, differentiated w.r.t. the LOW-resolution logits that `logits_up` was upsampled from:
    backward is one pass over logits_up (dasac_ce_loss_bwd_low) -- the full-resolution gradient (359.5 MB at 8 x 769^2)
    is never written or read back.  `logits_up` enters detached; its own autograd edge (for other consumers) is untouched."""

    @staticmethod
    def forward(ctx, logits_low, logits_up, labels, class_weight, conf):
        loss, _, _ = ops.ce_loss(logits_up, labels, class_weight, conf)
        ctx.save_for_backward(logits_up, labels, class_weight, conf)
        ctx.low_hw = tuple(logits_low.shape[2:])
        return loss

    @staticmethod
    def backward(ctx, g):
        logits_up, labels, class_weight, conf = ctx.saved_tensors
        return ops.ce_loss_bwd_low(logits_up, labels, ctx.low_hw, class_weight, conf, gscale=g.contiguous()), None, None, None, None


def _ce(logits_up, labels, class_weight, conf):
    low, version = getattr(logits_up, "_dasac_low", None) or (None, None)
    # The shortcut sends the loss gradient straight to the low-resolution logits, past `logits_up`'s own autograd edge.
    # It is taken only while that is indistinguishable from the long way round: `logits_up` was not edited in place since
    # it was upsampled (version counter) and nobody observes its gradient (retain_grad / tensor hooks).  Otherwise the
    # loss is differentiated w.r.t. logits_up itself and autograd continues through the upsampling's own backward.
    watched = logits_up.retains_grad or bool(getattr(logits_up, "_backward_hooks", None))
    if low is not None and version == logits_up._version and not watched and low.requires_grad and torch.is_grad_enabled() \
            and tuple(low.shape[:2]) == tuple(logits_up.shape[:2]):
        return _CELossLow.apply(low, logits_up.detach(), labels, class_weight, conf)
    return _CELoss.apply(logits_up, labels, class_weight, conf)


def ce_mean_all_pixels(logits_up, labels):
    """criterion(logits_up, y).mean().view(1) with CrossEntropyLoss(ignore_index=255, reduction='none')
    (deeplabv2.py:223-224): the mean runs over ALL pixels, ignored ones included."""
    return _ce(logits_up, labels, None, None)


def focal_ce(logits_up, labels, class_weight, conf=None):
    """sac.py:119-149 loss value ([1]); conf given -> `_focal_ce_conf` broadcast form."""
    return _ce(logits_up, labels, class_weight, conf)
