"""dasac_hip.engine on the small synthetic plans of tests/plan_ref.py against its float64 reference interpreter: every slot
activation, every slot gradient and every parameter gradient, per plan, under the yardstick of tests/fp64_yardstick.py
    err(HIP vs fp64 under the HIP ReLU pattern) <= 2 * err(ATen fp32 vs fp64 under ATen's pattern) + 1e-6        per tensor;
the same through autograd for the `need` subsets; the kernels each plan's `features` name were really launched; keep=False,
the error paths, determinism and a single-process GradSink.  The preconditions (features present, ReLU flip budget of the
reference, pool gaps, non-trivial gradients) are test_engine_plans_cpu.py's."""
import collections
import inspect

import pytest
import torch

import plan_ref as R
from conftest import rel_err
from fp64_yardstick import FLOOR, _report

pytestmark = pytest.mark.gpu

NAMES = [n for n, _ in R.PLANS]
CASES = [(n, s) for n in NAMES for s in R.SEEDS]
U32 = 2.0 ** -24


def _engine(name, seed):
    from dasac_hip import engine as E
    from dasac_hip import ops
    assert ops.PRECISION == "fp32" and ops.ALGORITHM == "auto"
    plan, x, gout, feats = R.build(name, seed)
    R.to_device(plan, "cuda")
    return E.Engine(plan), x.cuda(), gout.cuda(), feats


# ------------------------------------------------------------------------------------------------ which kernels ran
def _ptr(t):
    return None if t is None else t.data_ptr()


def _mask_kind(m):
    from dasac_hip import ops
    return None if m is None else ("bits" if isinstance(m, ops.ReluBits) else "fp32")


_SUMMARY = {
    "conv_gemm": lambda a: dict(M=a["M"], K=a["K"], stride=a["stride"], ostride=a["ostride"], shift=a["shift"] is not None,
                                res=a["res"] is not None, mask=_mask_kind(a["mask"]), bits_out=a["bits_out"] is not None,
                                stats=a["stats"] is not None),
    "conv_wgrad": lambda a: dict(cin=a["spec"].cin, cout=a["spec"].cout, dot=a["dot"] is not None, sums=a["sum_dz"] is not None),
    "relu_mask": lambda a: dict(y=_ptr(a["y"])),
    "add": lambda a: dict(n=a["a"].numel()),
    "channel_sums": lambda a: dict(C=a["x"].shape[1]),
    "bn_param_grads": lambda a: dict(C=a["sum_dz"].numel(), dot=a["dot"] is not None, gamma=a["want_gamma"], bias=a["want_bias"]),
    "bn_train_forward": lambda a: dict(C=a["z"].shape[1], stats=a["tile_stats"] is not None, res=a["res"] is not None, relu=a["relu"]),
    "bn_train_backward": lambda a: dict(C=a["z"].shape[1], params=a["want_params"]),
    "maxpool_bwd": lambda a: dict(k=a["k"], s=a["s"], p=a["p"], relu=bool(a["relu_mask"])),
    "scale_planes": lambda a: dict(m=_ptr(a["plane_scale"])),
    "upsample_bwd": lambda a: dict(),
}


class Recorder:
    """Wraps the ops.* functions whose choice engine.py makes and keeps (name, summary of the arguments) per call."""

    def __init__(self, monkeypatch):
        from dasac_hip import ops
        self.events = []
        for name, summary in _SUMMARY.items():
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name), summary))

    def _wrap(self, name, fn, summary):
        sig = inspect.signature(fn)

        def wrapped(*args, **kw):
            b = sig.bind(*args, **kw)
            b.apply_defaults()
            self.events.append((name, summary(b.arguments)))
            return fn(*args, **kw)
        return wrapped

    def mark(self):
        return len(self.events)

    def find(self, name, start=0, stop=None, **want):
        """Indices of the calls of `name` in events[start:stop] whose summary has all of `want`."""
        ev = self.events[start:stop]
        return [start + i for i, (n, s) in enumerate(ev) if n == name and all(s[k] == v for k, v in want.items())]


def _consumers(eng, slot):
    return [op for op in eng.plan.ops if slot in op.inputs()]


def check_exercised(eng, rec, fwd_end, acts, bits_slots, grads, name, at):
    """True when the pass recorded in `rec` (forward = events[:fwd_end]) took the path feature `name` stands for."""
    ops_ = eng.plan.ops
    op = ops_[at["op"]] if "op" in at else None
    slot = at.get("slot")
    F_ = lambda fn, **w: rec.find(fn, 0, fwd_end, **w)             # calls of the forward / of the backward pass
    B_ = lambda fn, **w: rec.find(fn, fwd_end, None, **w)
    masked_here = lambda s: B_("relu_mask", y=acts[s].data_ptr())

    def add_then_mask(s):
        return any(rec.events[i - 1] == ("add", dict(n=acts[s].numel())) for i in masked_here(s))

    if slot is not None:
        cons, C = _consumers(eng, slot), eng.producer[slot].spec.cout
    if name == "order:conv_first":
        kind = "bits" if at["bits"] else "fp32"
        return (slot in bits_slots) == at["bits"] and not masked_here(slot) \
            and len(B_("conv_gemm", M=C, K=cons[0].spec.Kt, res=True, mask=kind, ostride=1)) == 1 \
            and len(B_("conv_gemm", M=C, K=cons[1].spec.Kt, res=True, mask=None)) == 1
    if name == "order:join_last":
        # the two convs deliver unmasked (the second one adds to the first one's gradient), `join` adds and masks
        return slot not in bits_slots and add_then_mask(slot) and len(masked_here(slot)) == 1 \
            and len(B_("conv_gemm", M=C, K=cons[1].spec.Kt, res=True, mask=None)) == 1
    if name == "order:strided_pair":
        first, second = B_("conv_gemm", M=C, ostride=2, res=False, mask=None), B_("conv_gemm", M=C, ostride=2, res=True, mask=None)
        m = masked_here(slot)
        return len(first) == len(second) == len(m) == 1 and first[0] < second[0] < m[0]
    if name == "bits:recorded_consumer_fp32":
        return slot in bits_slots and len(B_("conv_gemm", M=C, K=cons[0].spec.Kt, res=True, mask="fp32")) == 1
    if name == "bits:producer_cannot":
        return slot not in bits_slots and len(B_("conv_gemm", M=C, K=cons[0].spec.Kt, res=False, mask="fp32")) == 1
    if name == "conv:image_s2":
        return len(F_("conv_gemm", M=op.spec.cout, K=27, stride=2)) >= 1 and not B_("conv_gemm", M=3)
    if name in ("conv:1x1", "conv:dilated"):
        return len(F_("conv_gemm", M=op.spec.cout, K=op.spec.K, stride=1)) >= 1
    if name == "conv:expanded_first":
        E_ = op.expanded.E
        return len(F_("conv_gemm", M=E_, K=C)) == 1 and (slot in bits_slots) == at["bits"] \
            and len(B_("conv_gemm", M=C, K=E_, res=True, mask="bits" if at["bits"] else "fp32")) == 1
    if name == "conv:expanded_second":
        E_ = op.expanded.E
        ex, plain = B_("conv_gemm", M=C, K=E_, res=False, mask=None), B_("conv_gemm", M=C, K=ops_[at["plain"]].spec.Kt, res=True, mask="fp32")
        return len(ex) == len(plain) == 1 and ex[0] < plain[0] and slot in bits_slots
    if name == "conv:sum40":
        gb = [grads[j] for j in op.b_idx]
        return len(F_("add", n=40)) == 1 and len(F_("conv_gemm", M=40, K=op.spec.K, shift=True)) == 1 and len(gb) == 2 \
            and torch.equal(gb[0], gb[1]) and gb[0].data_ptr() != gb[1].data_ptr() and len(B_("conv_wgrad", cout=40, sums=True)) == 1
    if name in ("bn:frozen_bias", "bn:frozen_nobias"):
        return len(B_("bn_param_grads", C=op.spec.cout, dot=True, gamma=True, bias=name == "bn:frozen_bias")) >= 1
    if name in ("nobn:bias", "nobn:nobias"):
        return len(F_("conv_gemm", M=op.spec.cout, K=op.spec.K, shift=name == "nobn:bias")) >= 1
    if name in ("bn:train_stats", "bn:train_nostats"):
        st = name == "bn:train_stats"
        return len(F_("conv_gemm", M=op.spec.cout, K=op.spec.K, stats=st, shift=True)) == 1 \
            and len(F_("bn_train_forward", C=op.spec.cout, stats=st, res=True, relu=True)) == 1 \
            and len(B_("bn_train_backward", C=op.spec.cout, params=True)) == 2
    if name.startswith("pool:"):
        return len(B_("maxpool_bwd", k=op.k, s=op.s, p=op.p, relu=eng.producer[op.src].relu)) == 1
    if name == "up2add:chain":
        return len(B_("upsample_bwd")) == 2
    if name == "up2add:busy_relu_skip":
        return add_then_mask(slot)
    if name == "drop:train_pinned":
        m = op.module.keep_mask.data_ptr()
        return len(F_("scale_planes", m=m)) == 1 and len(B_("scale_planes", m=m)) == 1
    if name == "drop:eval_alias":
        return acts[op.dst] is acts[op.src] and bool(masked_here(op.src))
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ the yardstick
def _hip_reference(eng, name, seed, acts):
    """(float64 reference under the HIP ReLU pattern, ATen's errors); asserts the flip budget of the HIP pattern."""
    plan, x, gout, feats, rec64, ref64, rec32, ref32 = R.free_runs(name, seed)
    masks = [(acts[s] > 0).cpu() for s in R.relu_slots(eng.plan)]
    R.flip_budget(plan, rec64.z, masks, "{} seed {}: HIP".format(name, seed))
    return R.masked_run(plan, x, gout, masks), R.aten_errors(name, seed)


def _ratio(got, r64, err_aten):
    return rel_err(got, r64) / (2.0 * err_aten + FLOOR)


def _param_ratios(eng, ref, aten, grads, wanted):
    """Ratios of the wanted parameter gradients.  The conv bias in front of a batch-statistics BN has an exactly zero gradient (the
    batch mean removes the bias); what any implementation returns is the round-off of sum(dz) over a channel, a sum that cancels.
    Such a tensor has no scale of its own, so its bound is absolute: twice ATen's absolute error plus 8 units of fp32 round-off of
    the largest per-channel sum of |dz| (the forward error of a float32 sum of terms that carry a few ulp each)."""
    roles, zero = R.param_roles(eng.plan), R.zero_by_construction(eng.plan)
    out = collections.OrderedDict()
    for j in reversed(range(len(grads))):
        if not wanted[j]:
            continue
        i, role = roles[j]
        key = "p{}:{}@op{}".format(j, role, i)
        if j in zero:
            room = 8 * U32 * float(ref.pre_bn[i].grad.abs().sum((0, 2, 3)).max())
            out[key] = float((grads[j].double().cpu() - ref.params[j].grad).abs().max()) / (2.0 * aten["p_abs", j] + room)
        else:
            out[key] = _ratio(grads[j], ref.params[j].grad, aten["p", j])
    return out


WORST = {}


@pytest.mark.parametrize("name,seed", CASES)
def test_plan_forward_and_backward_against_float64(name, seed, monkeypatch):
    from dasac_hip import engine as E
    eng, x, gout, feats = _engine(name, seed)
    rec = Recorder(monkeypatch)
    out, saved = eng.forward(x, keep=True)
    fwd_end = rec.mark()
    acts, bits_slots = dict(saved["acts"]), set(saved["bits"])
    trace = {}
    grads = E.Engine.backward(eng, saved, gout, [True] * len(eng.params), trace=trace)
    torch.cuda.synchronize()
    assert sorted(trace) == sorted(op.dst for op in eng.plan.ops) and all(g is not None for g in grads)

    ref, aten = _hip_reference(eng, name, seed, acts)
    ratios = collections.OrderedDict()
    for op in eng.plan.ops:                                            # forward order: the first activation that is off
        ratios["act{}".format(op.dst)] = _ratio(acts[op.dst], ref.acts[op.dst], aten["a", op.dst])
    for op in reversed(eng.plan.ops):                                  # backward order: the first slot gradient that is off
        ratios["grad{}".format(op.dst)] = _ratio(trace[op.dst], ref.grad_at[op.dst].grad, aten["g", op.dst])
    ratios.update(_param_ratios(eng, ref, aten, grads, [True] * len(grads)))
    WORST[name] = max(WORST.get(name, 0.0), max(ratios.values()))
    print("worst ratio of {} so far: {:.3g}".format(name, WORST[name]))
    _report("engine plan", "{} seed {}".format(name, seed), ratios)

    for f, at in feats.items():                                        # every case takes the path its feature names
        assert check_exercised(eng, rec, fwd_end, acts, bits_slots, grads, f, at), (name, f, at, rec.events)


def _set_need(eng, need):
    for p, n in zip(eng.params, need):
        p.requires_grad_(bool(n))
        p.grad = None


@pytest.mark.parametrize("name", R.NEED_SETS)
def test_need_subsets_through_autograd(name, monkeypatch):
    from dasac_hip import engine as E
    seed = R.SEEDS[0]
    eng, x, gout, feats = _engine(name, seed)
    _, saved = eng.forward(x, keep=True)
    ref, aten = _hip_reference(eng, name, seed, saved["acts"])
    del saved
    rec = Recorder(monkeypatch)
    train = name == "strided_pair_bits"
    for label, need in R.need_sets(eng.plan).items():
        _set_need(eng, need)
        start = rec.mark()
        E.run_plan(eng, x).backward(gout)
        torch.cuda.synchronize()
        for p, n in zip(eng.params, need):
            assert (p.grad is not None) == n, (name, label)
        _report("engine plan need={}".format(label), name, _param_ratios(eng, ref, aten, [p.grad for p in eng.params], need))
        # the branch of _param_grads the subset stands for
        wg = rec.find("conv_wgrad", start)
        n_conv = len(eng._convs)
        if label == "weights":
            assert len(wg) == n_conv and not rec.find("bn_param_grads", start) and not rec.find("channel_sums", start)
            assert not rec.find("conv_wgrad", start, dot=True) and not rec.find("conv_wgrad", start, sums=True)
            assert not rec.find("bn_train_backward", start, params=True)
        elif label == "bn_affine":
            frozen = [op for op in eng._convs if op.frozen_bn]
            # the weight-gradient kernel runs for its dot rows although no weight is wanted
            assert len(wg) == len(frozen) == len(rec.find("conv_wgrad", start, dot=True, sums=True))
            assert len(rec.find("bn_param_grads", start, dot=True, gamma=True, bias=False)) == len(frozen)
            assert len(rec.find("bn_train_backward", start, params=True)) == (2 if train else 0)
        elif label in ("biases", "one_bias"):
            with_bias = [op for op in eng._convs if op.has_bias]
            n = len(with_bias) if label == "biases" else 1
            assert not wg and len(rec.find("channel_sums", start)) == n
            n_frozen = sum(op.frozen_bn for op in with_bias) if label == "biases" else 1
            assert len(rec.find("bn_param_grads", start, dot=False, gamma=False, bias=True)) == n_frozen == len(rec.find("bn_param_grads", start))
        elif label == "one_gamma":
            assert len(wg) == 1 == len(rec.find("bn_param_grads", start, dot=True, gamma=True, bias=False)) and not rec.find("channel_sums", start)
        elif label == "first_two_ops_frozen":
            assert len(wg) == n_conv - 2
        # Engine.backward itself: None where not needed, the autograd gradient elsewhere
        _, saved = eng.forward(x, keep=True)
        direct = E.Engine.backward(eng, saved, gout, need)
        for p, n, g in zip(eng.params, need, direct):
            assert (g is not None) == n and (g is None or torch.equal(g.view(torch.int32), p.grad.view(torch.int32))), (name, label)
    _set_need(eng, [True] * len(eng.params))


# ------------------------------------------------------------------------------------------------ keep=False, errors, determinism
@pytest.mark.parametrize("name", NAMES)
def test_keep_false_gives_the_same_output_and_frees_the_rest(name):
    eng, x, gout, feats = _engine(name, R.SEEDS[0])
    out_keep, saved_keep = eng.forward(x, keep=True)
    out, saved = eng.forward(x, keep=False)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), out_keep.view(torch.int32))
    assert sorted(saved["acts"]) == [0, eng.plan.output] and not saved["aux"] and not saved["bits"]
    assert saved["acts"][eng.plan.output] is out and saved["acts"][0] is x
    if "drop:eval_alias" in feats:
        # the alias of the eval-mode dropout was deleted as a slot of its own; its consumer had read the live tensor before
        op = eng.plan.ops[feats["drop:eval_alias"]["op"]]
        assert saved_keep["acts"][op.dst] is saved_keep["acts"][op.src] and op.dst not in saved["acts"]


def test_a_second_backward_through_one_forward_raises():
    from dasac_hip import engine as E
    eng, x, gout, feats = _engine("res_conv_first_fp32", R.SEEDS[0])
    out = E.run_plan(eng, x)
    out.backward(gout, retain_graph=True)
    with pytest.raises(RuntimeError, match="already consumed by a backward pass"):
        out.backward(gout)


def _forward_ratio(eng, x):
    """(HIP output, float64 output, yardstick ratio) against the float64 reference of the modules AS THEY ARE NOW (under the
    HIP pattern); the yardstick's other side is the ATen fp32 run of the same modules."""
    from oracle.nets_ref import MaskedRelu
    plan, x_cpu = eng.plan, x.cpu()
    out, saved = eng.forward(x, keep=True)
    masks = [(saved["acts"][s] > 0).cpu() for s in R.relu_slots(plan)]
    r64 = R.run_reference(plan, x_cpu, torch.float64, MaskedRelu(masks))
    rec32 = R.RecordingRelu()
    r32 = R.run_reference(plan, x_cpu, torch.float32, rec32)
    r64a = R.run_reference(plan, x_cpu, torch.float64, MaskedRelu([z > 0 for z in rec32.z]))
    o = plan.output
    return out, r64.acts[o].detach(), _ratio(out, r64.acts[o].detach(), rel_err(r32.acts[o].detach(), r64a.acts[o].detach()))


@pytest.mark.parametrize("how", ["data_mul_", "no_grad_mul_"])
@pytest.mark.parametrize("name", ["res_conv_first_bits", "aspp_first_bits", "sum40"])
def test_forward_after_an_in_place_parameter_update(name, how):
    """Warm caches (folded BN vectors, packed weights, expanded packs, summed biases), then every parameter is scaled in place by
    a factor in [0.75, 1.25] -- through `p.data.mul_` and, next to it, through `p.mul_` under no_grad (what torch.optim does) --
    and the next forward has to be the updated network's.

    The engine's caches are keyed on (data_ptr, _version) of the parameters, and `p.data` is an alias with a version counter of
    its own: on plain nn.Parameters the `data_mul_` cases returned a mix of the old network's packs and folds and the live biases
    (yardstick ratio of the output 2.28e+05 / 1.91e+05 / 1.60e+05 for the three plans, bound 1, against 0.22 / 0.17 / 0.19 after
    the no_grad `p.mul_`).  engine.TrackedParameter, the class an Engine gives its parameters, moves p's counter when `p.data` is
    read or assigned."""
    seed = R.SEEDS[0]
    eng, x, gout, feats = _engine(name, seed)
    _, before, r0 = _forward_ratio(eng, x)
    gen = torch.Generator().manual_seed(7)
    for p in eng.params:
        f = (0.75 + 0.5 * torch.rand(p.shape, generator=gen)).cuda()
        if how == "data_mul_":
            p.data.mul_(f)
        else:
            with torch.no_grad():
                p.mul_(f)
    out, after, r1 = _forward_ratio(eng, x)
    moved = rel_err(after, before)
    print("in-place update ({}) of {}: reference output moved by {:.3g}; ratio before {:.3g}, after {:.3g}; "
          "HIP output vs the OLD reference {:.3g}".format(how, name, moved, r0, r1, rel_err(out, before)))
    assert moved > 1e-2
    _report("engine plan after {}".format(how), name, {"before": r0, "after": r1})


def _bn_state(eng):
    return [b for op in eng._convs if op.bn is not None for b in (op.bn.running_mean, op.bn.running_var, op.bn.num_batches_tracked)]


@pytest.mark.parametrize("name", NAMES)
def test_two_runs_from_one_state_are_bit_identical(name):
    from dasac_hip import engine as E
    eng, x, gout, feats = _engine(name, R.SEEDS[0])
    state = [b.clone() for b in _bn_state(eng)]
    runs = []
    for _ in range(2):
        with torch.no_grad():
            for b, s in zip(_bn_state(eng), state):
                b.copy_(s)
        _set_need(eng, [True] * len(eng.params))
        out = E.run_plan(eng, x)
        out.backward(gout)
        runs.append([out.detach().clone()] + [p.grad.clone() for p in eng.params])
    torch.cuda.synchronize()
    for a, b in zip(*runs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------------------ single-process GradSink
@pytest.mark.parametrize("label", ["all", "bn_affine", "first_two_ops_frozen"])
@pytest.mark.parametrize("name", R.NEED_SETS)
def test_single_process_grad_sink_writes_only_the_parameters_slices(name, label):
    from dasac_hip import engine as E
    from dasac_hip import parallel

    class NanSink(parallel.GradSink):
        def begin(self, engine, need, grad_out):
            grad_out = super().begin(engine, need, grad_out)
            self._flat.fill_(float("nan"))
            self.seen = self._flat
            return grad_out

    eng, x, gout, feats = _engine(name, R.SEEDS[0])
    need = R.need_sets(eng.plan)[label]
    _set_need(eng, need)
    E.run_plan(eng, x).backward(gout)
    plain = [None if p.grad is None else p.grad.clone() for p in eng.params]
    _set_need(eng, need)
    sink = NanSink(bucket_bytes=1 << 10)
    assert sink.world() == 1
    E.run_plan(eng, x, sink=sink).backward(gout)
    torch.cuda.synchronize()
    flat = sink.seen.cpu()
    assert len(sink._buckets) >= 2 and sink._launches == [1] * len(sink._buckets) and sink.launched == 0
    covered = torch.zeros(flat.numel(), dtype=torch.bool)
    for j, (p, n) in enumerate(zip(eng.params, need)):
        assert (p.grad is not None) == n == (j in sink._offsets) == (plain[j] is not None)
        if not n:
            assert sink.alloc(j) is None                                   # no slice of its own
            continue
        assert torch.equal(p.grad.view(torch.int32), plain[j].view(torch.int32)), (name, label, j)
        o = sink._offsets[j]
        assert o % parallel._ALIGN == 0 and not covered[o:o + p.numel()].any()
        covered[o:o + p.numel()] = True
        assert torch.equal(flat[o:o + p.numel()].view(torch.int32), plain[j].cpu().view(-1).view(torch.int32))       # written in place
    assert flat.numel() == sink._total and bool(torch.isnan(flat[~covered]).all()) and not torch.isnan(flat[covered]).any()
    assert int((~covered).sum()) > 0                                       # there were alignment gaps to leave alone
    _set_need(eng, [True] * len(eng.params))
