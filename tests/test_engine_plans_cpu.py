"""Preconditions of test_gpu_engine_plans.py, checked without a GPU from the reference interpreter (tests/plan_ref.py) alone: every
plan contains the features it lists, the float64 reference is well-conditioned for the seeds the GPU test uses (ReLU flip budget,
pool gaps, no all-zero gradient), and Engine refuses the plan shapes its backward pass has no code for at construction."""
import pytest
import torch
import torch.nn as nn

import plan_ref as R
from dasac_hip import engine as E
from dasac_hip import lib as L

NAMES = [n for n, _ in R.PLANS]
CASES = [(n, s) for n in NAMES for s in R.SEEDS]


def test_host_rules_restate_the_library():
    lib = L.load()
    for M in (3, 8, 24, 32, 33, 40, 48, 64, 65, 80, 96, 128, 129, 288):
        assert R.mpad(M) == lib.dasac_conv_mpad(M)
        for Cx in (3, 8, 16, 24, 40, 48, 80, 96, 288):
            assert R.bits_ok(M, Cx) == bool(lib.dasac_conv_gemm_bits_ok(M, Cx)) == bool(lib.dasac_conv_gemm_stats_ok(M, Cx))
    assert all(R.bits_ok(c, c) for c in (80, 96)) and not any(R.bits_ok(c, c) for c in (24, 40, 48))


def _consumers(eng, slot):
    """Ops that read `slot`, in plan order."""
    return [op for op in eng.plan.ops if slot in op.inputs()]


def _channels(eng, slot):
    return eng.producer[slot].spec.cout


def check_feature(eng, name, at):
    """True when the plan of `eng` has feature `name` at the slots / ops `at` names (read from the engine's own tables)."""
    ops_ = eng.plan.ops
    op = ops_[at["op"]] if "op" in at else None
    slot = at.get("slot")
    if slot is not None:
        prod, cons = eng.producer[slot], _consumers(eng, slot)
        assert prod.relu and eng.consumers[slot] == len(cons)
        C = _channels(eng, slot)
        prod_bits = R.bits_ok(prod.spec.cout, prod.spec.cin) and prod.expanded is None and not (prod.bn is not None and prod.bn.training)
    if name == "order:conv_first":
        first = cons[0]
        return len(cons) == 3 and first.kind == "conv" and first.src == slot and first.spec.stride == 1 and cons[1].src == slot \
            and cons[2].res == slot and eng._bits_wanted[slot] and prod_bits == at["bits"] and R.bits_ok(C, first.spec.cout) == at["bits"]
    if name == "order:join_last":
        return len(cons) == 3 and cons[0].res == slot and cons[0].src != slot and all(c.src == slot for c in cons[1:]) \
            and not eng._bits_wanted[slot] and prod_bits == at["could_use_bits"]
    if name == "order:strided_pair":
        return len(cons) == 2 and all(c.kind == "conv" and c.src == slot and c.spec.stride == 2 and c.spec.taps == 1 for c in cons) \
            and not eng._bits_wanted[slot]
    if name == "bits:recorded_consumer_fp32":
        return eng._bits_wanted[slot] and prod_bits and not R.bits_ok(C, cons[0].spec.cout) and cons[0].src == slot and len(cons) == 2 \
            and cons[1].res == slot
    if name == "bits:producer_cannot":
        return eng._bits_wanted[slot] and not prod_bits and R.bits_ok(C, cons[0].spec.cout) and len(cons) == 1
    if name == "conv:image_s2":
        return op.src == 0 and op.spec.stride == 2 and op.spec.branches == [(3, 3, 1, 1)]
    if name == "conv:1x1":
        return op.spec.branches == [(1, 1, 1, 0)] and op.spec.stride == 1
    if name == "conv:dilated":
        kh, kw, d, p = op.spec.branches[0]
        return (kh, kw) == (3, 3) and d > 1 and p == d and len(op.spec.branches) == 1
    if name == "conv:expanded_first":
        return op.expanded is not None and len(op.convs) == 4 and op.spec.cout == 8 and cons[0] is op and len(cons) == 2 \
            and cons[1].expanded is None and (prod_bits and R.bits_ok(C, op.expanded.E)) == at["bits"] and eng._bits_wanted[slot]
    if name == "conv:expanded_second":
        return op.expanded is not None and len(op.convs) == 4 and cons[1] is op and cons[0] is ops_[at["plain"]] and len(cons) == 2 \
            and cons[0].expanded is None
    if name == "conv:sum40":
        return op.expanded is None and len(op.convs) == 2 and op.spec.cout == 40 and op.has_bias and op.bn is None
    if name in ("bn:frozen_bias", "bn:frozen_nobias"):
        return op.frozen_bn and op.has_bias == (name == "bn:frozen_bias")
    if name in ("nobn:bias", "nobn:nobias"):
        return op.bn is None and len(op.convs) == 1 and op.has_bias == (name == "nobn:bias")
    if name in ("bn:train_stats", "bn:train_nostats"):
        return op.bn is not None and op.bn.training and op.has_bias and op.relu and op.res is not None \
            and R.stats_ok(op.spec.cout, op.spec.cin) == (name == "bn:train_stats")
    if name == "pool:k3s2p1_ceil_relu":
        return (op.k, op.s, op.p, op.ceil) == (3, 2, 1, True) and eng.producer[op.src].relu
    if name == "pool:k2s2_norelu":
        return (op.k, op.s, op.p, op.ceil) == (2, 2, 0, False) and eng.producer[op.src].kind == "conv" and not eng.producer[op.src].relu
    if name == "pool:k3s1p1":
        return (op.k, op.s, op.p) == (3, 1, 1)
    if name == "up2add:chain":
        a, b = (ops_[i] for i in at["ops"])
        return a.kind == b.kind == "up2add" and b.src == a.dst
    if name == "up2add:busy_relu_skip":
        return op.kind == "up2add" and op.skip == slot and len(cons) == 2 and cons[0] is op and cons[1].kind == "conv"
    if name == "drop:train_pinned":
        m = op.module
        return op.kind == "drop" and m.training and m.p > 0 and bool((m.keep_mask == 0).any()) and bool((m.keep_mask > 0).any())
    if name == "drop:eval_alias":
        return op.kind == "drop" and not op.module.training
    raise KeyError(name)


@pytest.mark.parametrize("name", NAMES)
def test_every_listed_feature_is_in_the_plan(name):
    plan, x, gout, feats = R.build(name, R.SEEDS[0])
    eng = E.Engine(plan)
    assert feats and set(feats) <= set(R.FEATURES)
    for f, at in feats.items():
        assert check_feature(eng, f, at), (name, f, at)
    assert len(eng.params) == len(R.param_roles(plan)) == sum(len(op.params()) for op in plan.ops)


def test_the_catalogue_covers_every_feature_and_the_shape_rules():
    have, widths, batch = set(), [], []
    variants = set()
    for name, build in R.PLANS:
        plan, x, gout, feats = build(R.SEEDS[0])
        have |= set(feats)
        for f, at in feats.items():
            if "bits" in at:
                variants.add((f, at["bits"]))
        N, C, H, W = x.shape
        assert C == 3 and H % 2 == 1 and W % 2 == 1 and 9 <= H <= 17 and 9 <= W <= 17, (name, x.shape)
        widths.append(W)
        batch.append(N)
        for op in plan.ops:
            if op.kind == "conv":
                assert {op.spec.cin, op.spec.cout} <= {3, 8, 24, 40, 48, 80, 96}, (name, op.spec.cin, op.spec.cout)
                assert op.spec.cin * op.spec.cout < 512 * 512                  # no Winograd route
    assert have == set(R.FEATURES), set(R.FEATURES) ^ have
    assert min(widths) < 16 and sorted(set(batch)) == [1, 2] and batch.count(1) == 1
    # both channel choices of the consumer orders
    assert {("order:conv_first", True), ("order:conv_first", False), ("conv:expanded_first", True), ("conv:expanded_first", False)} <= variants
    assert set(R.NEED_SETS) <= set(NAMES)


@pytest.mark.parametrize("name", R.NEED_SETS)
def test_need_sets_are_distinct_proper_subsets(name):
    plan = R.build(name, R.SEEDS[0])[0]
    sets = R.need_sets(plan)
    assert list(sets) == ["all", "weights", "bn_affine", "biases", "first_two_ops_frozen", "one_bias", "one_gamma"]
    assert all(sets["all"]) and len({tuple(v) for v in sets.values()}) == len(sets)
    for k, v in sets.items():
        assert any(v) and (k == "all" or not all(v)), k
    assert sum(sets["one_bias"]) == sum(sets["one_gamma"]) == 1
    train = [op.bn.training for op in plan.ops if op.kind == "conv" and op.bn is not None]
    assert any(train) == (name == "strided_pair_bits")
    # the single bias of the train-mode plan is not one of the biases whose gradient is zero by construction
    assert not any(sets["one_bias"][j] for j in R.zero_by_construction(plan))


@pytest.mark.parametrize("name,seed", CASES)
def test_relu_flip_budget_of_aten_fp32(name, seed):
    plan, x, gout, feats, rec64, ref64, rec32, ref32 = R.free_runs(name, seed)
    assert len(rec64.z) == len(R.relu_slots(plan)) > 0
    R.flip_budget(plan, rec64.z, [z > 0 for z in rec32.z], "{} seed {}: ATen fp32".format(name, seed))


@pytest.mark.parametrize("name,seed", CASES)
def test_pool_windows_have_one_clear_maximum(name, seed):
    """In every pool window whose float64 maximum is positive (behind a ReLU conv the others are all-zero windows that receive no
    gradient; behind any other op: every window) the two largest values are further apart than 1e-5 of the tensor's max."""
    plan, x, gout, feats, rec64, ref64, rec32, ref32 = R.free_runs(name, seed)
    eng_producer = {op.dst: op for op in plan.ops}
    for op in plan.ops:
        if op.kind != "pool":
            continue
        a = ref64.acts[op.src].detach()
        N, C, H, W = a.shape
        OH, OW = ref64.acts[op.dst].shape[2:]
        # windows as columns; padding and the ceil-mode overhang count as -inf
        ph, pw = (OH - 1) * op.s + op.k - H - op.p, (OW - 1) * op.s + op.k - W - op.p
        padded = torch.nn.functional.pad(a, (op.p, max(pw, 0), op.p, max(ph, 0)), value=float("-inf"))
        cols = torch.nn.functional.unfold(padded.reshape(N * C, 1, *padded.shape[2:]), op.k, stride=op.s)[:, :, :OH * OW]
        assert cols.shape[2] == OH * OW
        top = cols.topk(2, dim=1).values
        assert torch.equal(top[:, 0].reshape(N, C, OH, OW), ref64.acts[op.dst].detach())
        relu_src = eng_producer[op.src].relu
        judged = top[:, 0] > 0 if relu_src else torch.ones_like(top[:, 0], dtype=torch.bool)
        gap = (top[:, 0] - top[:, 1])[judged]
        assert judged.any() and float(gap.min()) > 1e-5 * float(a.abs().max()), (name, seed, op.src, float(gap.min()))


@pytest.mark.parametrize("name,seed", CASES)
def test_reference_gradients_are_not_trivial(name, seed):
    plan, x, gout, feats, rec64, ref64, rec32, ref32 = R.free_runs(name, seed)
    zero = R.zero_by_construction(plan)
    roles = R.param_roles(plan)
    for j, p in enumerate(ref64.params):
        assert p.grad is not None and tuple(p.grad.shape) == tuple(p.shape)
        if j in zero:
            # the bias in front of a batch-statistics BN: round-off of a sum that cancels, nothing else
            dz = ref64.pre_bn[roles[j][0]].grad
            assert float(p.grad.abs().max()) <= 1e-12 * float(dz.abs().sum((0, 2, 3)).max())
        else:
            assert float(p.grad.abs().max()) > 0, (name, seed, j, roles[j])
    for op in plan.ops:
        g = ref64.grad_at[op.dst].grad
        assert g is not None and float(g.abs().max()) > 0, (name, seed, op.dst)
    for op in plan.ops:
        if op.kind == "drop" and op.module.training:
            dropped = op.module.keep_mask == 0
            assert dropped.any() and float(ref64.acts[op.dst].detach()[dropped].abs().max()) == 0.0
            assert float(ref64.acts[op.src].detach()[dropped].abs().max()) > 0         # planes that had something to lose


def test_reference_matches_module_forward():
    """The interpreter against the modules themselves (nn.Conv2d / nn.BatchNorm2d called directly) on a plan without branches."""
    plan, x, gout, feats = R.build("pools", 1)
    ref = R.run_reference(plan, x, torch.float32)
    y = x
    with torch.no_grad():
        for op in plan.ops:
            if op.kind == "conv":
                y = op.convs[0](y)
                y = op.bn(y) if op.bn is not None else y
                y = torch.relu(y) if op.relu else y
            else:
                y = nn.functional.max_pool2d(y, op.k, op.s, op.p, ceil_mode=op.ceil)
    assert torch.equal(y, ref.acts[plan.output].detach())


def test_engine_parameters_move_their_version_counter_on_data_access():
    """Engine gives its parameters the class TrackedParameter: the same objects, still nn.Parameters for modules, optimisers,
    deepcopy and state_dict, whose `.data` (an alias with a version counter of its own) moves the parameter's own counter when it
    is read or assigned -- the cache keys of the engine follow `p.data.mul_(...)`."""
    import copy
    plan, x, gout, feats = R.build("sum40", 1)
    before = [p for op in plan.ops for p in op.params()]
    plain = nn.Parameter(torch.ones(3))
    v = plain._version
    plain.data.mul_(2.0)
    assert plain._version == v                                  # what the class is there for
    eng = E.Engine(plan)
    assert len(eng.params) == len(before) and all(a is b for a, b in zip(eng.params, before)) and not eng.stale()
    conv = plan.ops[0].convs[0]
    for p in eng.params:
        assert type(p) is E.TrackedParameter and isinstance(p, nn.Parameter) and p.requires_grad and p.is_leaf
        key, values = E._ver(p), p.detach().clone()
        p.data.mul_(2.0)
        assert E._ver(p) != key and torch.equal(p.detach(), 2.0 * values)
        key = E._ver(p)
        p.data = values.clone()
        assert E._ver(p) != key and torch.equal(p.detach(), values)
    assert [n for n, _ in conv.named_parameters()] == ["weight"] and type(conv.state_dict()["weight"]) is torch.Tensor
    twin = copy.deepcopy(conv)
    assert torch.equal(twin.weight, conv.weight) and twin.weight is not conv.weight and twin.weight.requires_grad
    conv.double()
    assert conv.weight is eng.params[0] and conv.weight.dtype == torch.float64
    y = conv(x.double()).sum()
    y.backward()
    assert conv.weight.grad is not None
    opt = torch.optim.SGD([conv.weight], lr=0.1)
    key = E._ver(conv.weight)
    opt.step()
    assert E._ver(conv.weight) != key
    E.Engine(plan)                                              # a second engine over the same modules keeps the class
    # torch.optim chooses its multi-tensor implementations by exact type: the class is on its list, next to nn.Parameter
    from torch.optim.optimizer import _foreach_supported_types
    assert E.TrackedParameter in _foreach_supported_types and nn.Parameter in _foreach_supported_types


# ------------------------------------------------------------------------------------------------ unsupported plans
def _conv(cin, cout, k=1, **kw):
    return nn.Conv2d(cin, cout, k, **kw)


def test_engine_refuses_a_pool_whose_source_has_a_second_consumer():
    P = E.Plan()
    s1 = P.conv(0, _conv(3, 8, 3, padding=1), relu=True)
    s2 = P.maxpool(s1, 3, 1, 1)
    s3 = P.conv(s1, _conv(8, 8))
    out = P.conv(s2, _conv(8, 8), res=s3)
    with pytest.raises(ValueError, match=r"op 1 \(pool slot 1 -> slot 2\).*2 consumers"):
        E.Engine(P.finish(out))


def test_engine_refuses_a_strided_multi_tap_conv_off_the_image():
    P = E.Plan()
    s1 = P.conv(0, _conv(3, 8, 3, stride=2, padding=1), relu=True)         # from the image: fine
    out = P.conv(s1, _conv(8, 8, 3, stride=2, padding=1))
    with pytest.raises(ValueError, match=r"op 1 \(conv slot 1 -> slot 2\).*stride-2 conv with 9 taps"):
        E.Engine(P.finish(out))
    P = E.Plan()
    E.Engine(P.finish(P.conv(0, _conv(3, 8, 3, stride=2, padding=1))))     # the same conv on slot 0 is supported
    P = E.Plan()
    s1 = P.conv(0, _conv(3, 8, 3, padding=1), relu=True)
    E.Engine(P.finish(P.conv(s1, _conv(8, 8, 1, stride=2))))               # and so is a strided 1x1 anywhere


def test_engine_refuses_an_op_that_never_reaches_the_output():
    P = E.Plan()
    s1 = P.conv(0, _conv(3, 8, 3, padding=1), relu=True)
    s2 = P.conv(s1, _conv(8, 8))
    P.conv(s2, _conv(8, 8))                                                # a dead end that reads the output slot
    with pytest.raises(ValueError, match=r"op 2 \(conv slot 2 -> slot 3\) never reaches the plan's output \(slot 2\)"):
        E.Engine(P.finish(s2))
    P = E.Plan()
    s1 = P.conv(0, _conv(3, 8, 3, padding=1), relu=True)
    s2 = P.conv(s1, _conv(8, 8), relu=True)
    P.maxpool(s2, 2, 2)                                                    # a dead branch in the middle: slot 2 would wait for it
    with pytest.raises(ValueError, match=r"op 2 \(pool slot 2 -> slot 3\) never reaches"):
        E.Engine(P.finish(P.conv(s2, _conv(8, 8))))


def test_the_shipped_networks_are_still_accepted():
    import models
    crit = nn.CrossEntropyLoss(ignore_index=255, reduction="none")
    for cls in (models.DeepLabV2_ResNet101, models.DeepLabV2_VGG16, models.VGG16_FCN8s):
        eng = E.Engine(cls(num_classes=19, criterion=crit)._plan())
        assert len(eng.params) > 0 and eng.consumers[eng.plan.output] == 0
