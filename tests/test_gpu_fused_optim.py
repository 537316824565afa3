"""The other two optimisers of the reference's factory (base_trainer.py:47-73) on the HIP path: FusedSGD(nesterov=True)
(dasac_sgd_nesterov_step) and FusedAdam (dasac_adam_step), and `driver.make_optimizer(..., fused="all")`.

Tolerances.  Nesterov: the project's bound for the same-operation-order SGD kernel, 1e-6 rel (tests/test_gpu_optim.py).
Adam: no number of ours -- torch.optim.Adam on the device (fp32) and the fused optimiser are both compared with the same
Adam written in fp64 torch ops on fp64 copies; with e_ref = rel_err(torch fp32, fp64) per tensor the fused result must keep
rel_err(fused, fp64) <= 2 * e_ref + 1e-7 (2: one differently contracted multiply-add per element; 1e-7: about one fp32 ulp,
for tensors on which torch happens to be exact).  Measured values: profiles/fused_optim.md."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

from oracle import nets_ref as N
from conftest import rel_err
from test_gpu_models import CRIT, model_cfg

pytestmark = pytest.mark.gpu

SHAPES = [(64, 3, 7, 7), (64,), (5000,), (19, 2048, 3, 3), (1,), (4097,)]      # 1 element; 4097 = one chunk + 1; 85.5 chunks
LATE = 5                                                                     # gets its first gradient one step later
ZERO = 2                                                                     # Adam scenario: its gradient is exactly 0 (wd 0)


def make_params(seed, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    return g, [nn.Parameter(torch.randn(s, generator=g).cuda()) for s in shapes]


def clones(ps, dtype=torch.float32):
    return [nn.Parameter(p.detach().clone().to(dtype)) for p in ps]


def three_groups(ps, decay=True):
    wd = 5e-4 if decay else 0.0
    return [{"params": ps[:2], "lr": 2.5e-4, "weight_decay": wd}, {"params": ps[2:4], "lr": 5e-3, "weight_decay": 0.0},
            {"params": ps[4:], "lr": 2.5e-3, "weight_decay": wd}]


def versions(opt, ps, keys):
    return {id(t): t._version for p in ps for t in [p] + [opt.state.get(p, {}).get(k) for k in keys] if t is not None}


def assert_versions_advanced(opt, ps, keys, before):
    """Every tensor step() wrote through a raw pointer -- the parameters that had a gradient and their state -- has a newer
    autograd version (a state tensor created by this step counts as new)."""
    for p in ps:
        if p.grad is not None:
            for t in [p] + [opt.state[p][k] for k in keys]:
                assert t._version > before.get(id(t), -1)


def test_fused_nesterov_sgd_matches_torch_sgd():
    from dasac_hip.optim import FusedSGD
    g, pa = make_params(3)
    pb = clones(pa)
    oa = FusedSGD(three_groups(pa), momentum=0.9, nesterov=True)
    ob = torch.optim.SGD(three_groups(pb), momentum=0.9, nesterov=True)
    assert all(gr["nesterov"] is True for gr in oa.param_groups)
    for it in range(4):
        for i, (a, b) in enumerate(zip(pa, pb)):
            if it == 0 and i == LATE:
                continue
            gr = torch.randn(a.shape, generator=g).cuda()
            a.grad, b.grad = gr.clone(), gr.clone()
        if it == 2:
            for o in (oa, ob):
                o.param_groups[1]["lr"] = 1e-3               # schedules poke param_groups
        v0 = versions(oa, pa, ("momentum_buffer",))
        oa.step()
        ob.step()
        assert_versions_advanced(oa, pa, ("momentum_buffer",), v0)                   # engine caches key on this
        for a, b in zip(pa, pb):
            assert rel_err(a, b) < 1e-6
            if b in ob.state and "momentum_buffer" in ob.state[b]:
                assert rel_err(oa.state[a]["momentum_buffer"], ob.state[b]["momentum_buffer"]) < 1e-6
    sd = copy.deepcopy(oa.state_dict())
    assert set(sd["state"][0]) == {"momentum_buffer"} and sd["param_groups"][0]["nesterov"] is True
    ob.load_state_dict(sd)                                   # layout-compatible with torch.optim.SGD
    assert ob.param_groups[0]["nesterov"] is True
    for a, b in zip(pa, pb):
        gr = torch.randn(a.shape, generator=g).cuda()
        a.grad, b.grad = gr.clone(), gr.clone()
    oa.step()
    ob.step()                                                # torch continues from the fused optimiser's buffers
    for a, b in zip(pa, pb):
        assert rel_err(a, b) < 1e-6


def test_nesterov_keeps_torchs_conditions_and_refuses_mixed_groups():
    from dasac_hip.optim import FusedSGD
    _, pa = make_params(1, [(8,), (8,)])
    with pytest.raises(ValueError):
        FusedSGD(pa, momentum=0.0, nesterov=True)
    with pytest.raises(NotImplementedError):
        FusedSGD(pa, momentum=0.9, nesterov=True, dampening=0.1)
    opt = FusedSGD([{"params": pa[:1]}, {"params": pa[1:], "nesterov": False}], lr=0.1, momentum=0.9, nesterov=True)
    before = [p.detach().clone() for p in pa]
    for p in pa:
        p.grad = torch.ones_like(p)
    with pytest.raises(NotImplementedError):
        opt.step()
    assert all(torch.equal(p, b) for p, b in zip(pa, before))


class Fp64Adam:
    """torch.optim.Adam's rule (L2 weight decay in the gradient, no amsgrad) in fp64 torch ops."""

    def __init__(self, groups, betas, eps=1e-8):
        self.groups, self.betas, self.eps, self.state = groups, betas, eps, {}

    @torch.no_grad()
    def step(self):
        b1, b2 = self.betas
        for gr in self.groups:
            for p in gr["params"]:
                if p.grad is None:
                    continue
                st = self.state.setdefault(p, {"step": 0, "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)})
                st["step"] += 1
                g = p.grad.to(torch.float64)
                if gr["weight_decay"] != 0:
                    g = g + gr["weight_decay"] * p
                st["exp_avg"] = st["exp_avg"] + (1 - b1) * (g - st["exp_avg"])
                st["exp_avg_sq"] = st["exp_avg_sq"] * b2 + (1 - b2) * g * g
                step_size = gr["lr"] / (1 - b1 ** st["step"])
                denom = st["exp_avg_sq"].sqrt() / (1 - b2 ** st["step"]) ** 0.5 + self.eps
                p -= step_size * st["exp_avg"] / denom


def within_reference_error(tag, opt_x, px, opt_b, pb, ref, pc, report):
    """rel_err(x, fp64) <= 2 * rel_err(torch fp32, fp64) + 1e-7 for every parameter and state tensor; returns bit equality."""
    same = True
    for i, (x, b, c) in enumerate(zip(px, pb, pc)):
        trio = [("param", x, b, c)]
        if c in ref.state:
            trio += [(k, opt_x.state[x][k], opt_b.state[b][k], ref.state[c][k]) for k in ("exp_avg", "exp_avg_sq")]
            assert float(opt_x.state[x]["step"]) == float(opt_b.state[b]["step"]) == ref.state[c]["step"]
        for name, tx, tb, tc in trio:
            assert torch.isfinite(tx).all()
            e_x, e_ref = rel_err(tx, tc), rel_err(tb, tc)
            report.append((tag, i, name, e_x, e_ref))
            same = same and torch.equal(tx, tb)
            assert e_x <= 2 * e_ref + 1e-7, (tag, i, name, e_x, e_ref)
    return same


def feed(g, it, *param_lists):
    for i, ps in enumerate(zip(*param_lists)):
        if it == 0 and i == LATE:
            continue
        gr = torch.zeros(ps[0].shape) if i == ZERO else torch.randn(ps[0].shape, generator=g)
        for p in ps:
            p.grad = gr.to(device="cuda", dtype=p.dtype)


def print_report(title, report, same):
    """Largest error per kind of tensor over all tensors and steps, and the entry closest to (or furthest over) the bound."""
    for tag in sorted({r[0].split(" ")[0] for r in report}):
        for name in ("param", "exp_avg", "exp_avg_sq"):
            rows = [r for r in report if r[0].split(" ")[0] == tag and r[2] == name]
            tight = max(rows, key=lambda r: r[3] - (2 * r[4] + 1e-7))
            print("{}: {:<13} {:<10} max rel_err vs fp64: fused {:.3e}  torch fp32 {:.3e};  nearest the bound: {} tensor {} fused {:.3e} "
                  "torch {:.3e}".format(title, tag, name, max(r[3] for r in rows), max(r[4] for r in rows), tight[0], tight[1], tight[3], tight[4]))
    print("{}: bit-identical to torch.optim.Adam on every tensor and step: {}".format(title, same))


@pytest.mark.parametrize("decay", [True, False])
@pytest.mark.parametrize("beta1", [0.5, 0.9])            # ATen's lerp switches formula at weight 0.5: both branches
def test_fused_adam_matches_torch_adam_within_torchs_own_fp32_error(beta1, decay):
    from dasac_hip.optim import FusedAdam
    g, pa = make_params(3)
    pb, pc = clones(pa), clones(pa, torch.float64)
    betas = (beta1, 0.999)
    oa, ob = FusedAdam(three_groups(pa, decay), betas=betas), torch.optim.Adam(three_groups(pb, decay), betas=betas)
    ref = Fp64Adam(three_groups(pc, decay), betas)
    assert set(oa.param_groups[0]) == set(ob.param_groups[0])
    start, report, same = pa[ZERO].detach().clone(), [], True
    for it in range(7):
        feed(g, it, pa, pb, pc)
        if it == 2:
            for o in (oa, ob):
                o.param_groups[1]["lr"] = 1e-3               # schedules poke param_groups
            ref.groups[1]["lr"] = 1e-3
        v0 = versions(oa, pa, ("exp_avg", "exp_avg_sq"))
        oa.step()
        ob.step()
        ref.step()
        assert_versions_advanced(oa, pa, ("exp_avg", "exp_avg_sq"), v0)              # engine caches key on this
        same = within_reference_error("step %d" % it, oa, pa, ob, pb, ref, pc, report) and same
    print_report("adam beta1={} wd={}".format(beta1, decay), report, same)
    assert float(oa.state[pa[LATE]]["step"]) == 6 and float(oa.state[pa[0]]["step"]) == 7
    assert torch.is_tensor(oa.state[pa[0]]["step"]) and set(oa.state[pa[0]]) == set(ob.state[pb[0]])
    # an exactly-zero gradient without weight decay: 0 / (0 + eps) stays 0, nothing moves, no NaN
    assert torch.equal(pa[ZERO], start) and not oa.state[pa[ZERO]]["exp_avg"].any() and not oa.state[pa[ZERO]]["exp_avg_sq"].any()


def stash_scenario(make):
    g, pa = make_params(5, [(64, 3, 7, 7), (64,), (5000,), (4097,)])
    pb = clones(pa)
    groups = lambda ps: [{"params": ps[:2], "lr": 2.5e-4, "weight_decay": 5e-4}, {"params": ps[2:], "lr": 5e-3, "weight_decay": 0.0}]
    oa, ob = make(groups(pa)), make(groups(pb))
    for it in range(3):
        g1 = [torch.randn(a.shape, generator=g).cuda() for a in pa]
        g2 = [torch.randn(a.shape, generator=g).cuda() for a in pa]
        oa.zero_grad()                                       # as driver.sac_train_iteration does before the source backward
        for i, a in enumerate(pa):
            if i != 3:
                a.grad = g1[i].clone()
        oa.stash_grads()
        assert all(a.grad is None for a in pa)
        for i, (a, b) in enumerate(zip(pa, pb)):
            if i != 2:
                a.grad = g2[i].clone()                       # parameter 2: source pass only; parameter 3: target pass only
            b.grad = g1[i].clone() if i != 3 else None
            if i != 2:
                if b.grad is None:
                    b.grad = g2[i].clone()
                else:
                    b.grad += g2[i]                          # what AccumulateGrad does
        full = oa.full_grads()
        assert all(torch.equal(full[a], b.grad) for a, b in zip(pa, pb))
        oa.step()
        ob.step()
        for a, b in zip(pa, pb):
            assert torch.equal(a, b) and set(oa.state[a]) == set(ob.state[b]) and len(oa.state[a]) >= 1
            for k in oa.state[a]:
                assert torch.equal(oa.state[a][k], ob.state[b][k]), k
    pa[0].grad = torch.ones_like(pa[0])
    oa.stash_grads()
    oa.zero_grad()
    before = pa[0].detach().clone()
    oa.step()                                                # nothing stashed, no gradient: no update
    assert torch.equal(pa[0], before)


@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_stashed_gradients_sum_inside_the_new_updates_bit_for_bit(kind):
    from dasac_hip.optim import FusedAdam, FusedSGD
    stash_scenario((lambda gs: FusedAdam(gs, betas=(0.5, 0.999))) if kind == "adam" else (lambda gs: FusedSGD(gs, momentum=0.9, nesterov=True)))


def test_adam_state_dict_round_trips_with_torch_adam_in_both_directions():
    """Three steps, then a checkpoint of each optimiser continues in the OTHER class over cloned parameters for three more:
    all four trajectories stay within the bound of the Adam test, the step counts (the late parameter's smaller one included)
    survive."""
    from dasac_hip.optim import FusedAdam
    g, pa = make_params(7)
    pb, pc = clones(pa), clones(pa, torch.float64)
    betas = (0.5, 0.999)
    oa, ob = FusedAdam(three_groups(pa), betas=betas), torch.optim.Adam(three_groups(pb), betas=betas)
    ref = Fp64Adam(three_groups(pc), betas)
    report = []
    for it in range(3):
        feed(g, it, pa, pb, pc)
        for o in (oa, ob, ref):
            o.step()
        within_reference_error("fused", oa, pa, ob, pb, ref, pc, report)
    pd, pe = clones(pa), clones(pb)
    od, oe = torch.optim.Adam(three_groups(pd), betas=(0.9, 0.99)), FusedAdam(three_groups(pe), betas=(0.9, 0.99))
    od.load_state_dict(copy.deepcopy(oa.state_dict()))       # fused -> torch (deepcopy: what a saved checkpoint is)
    oe.load_state_dict(copy.deepcopy(ob.state_dict()))       # torch -> fused
    for o, ps in ((od, pd), (oe, pe)):
        assert o.param_groups[0]["betas"] == betas
        assert [float(o.state[p]["step"]) for p in ps] == [3, 3, 3, 3, 3, 2]
        assert torch.is_tensor(o.state[ps[0]]["step"])
    for it in range(3, 6):
        feed(g, it, pa, pb, pc, pd, pe)
        for o in (oa, ob, ref, od, oe):
            o.step()
        within_reference_error("fused", oa, pa, ob, pb, ref, pc, report)
        within_reference_error("fused->torch", od, pd, ob, pb, ref, pc, report)
        within_reference_error("torch->fused", oe, pe, ob, pb, ref, pc, report)
    print_report("adam round trip", report, "-")
    for o, ps in ((oa, pa), (od, pd), (oe, pe)):
        assert [float(o.state[p]["step"]) for p in ps] == [6, 6, 6, 6, 6, 5]


@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_refusals_come_before_any_launch(kind):
    from dasac_hip.optim import FusedAdam, FusedSGD
    make = (lambda gs, **kw: FusedAdam(gs, lr=0.1, **kw)) if kind == "adam" else (lambda gs, **kw: FusedSGD(gs, lr=0.1, momentum=0.9, nesterov=True, **kw))
    _, pa = make_params(2, [(33,)] * 9)
    with pytest.raises(ValueError):
        make([{"params": [p]} for p in pa])                  # more than 8 groups
    bad = {"non-contiguous": nn.Parameter(torch.randn(8, 6).cuda().t()), "fp16": nn.Parameter(torch.randn(16).cuda().half())}
    for what, p in bad.items():
        assert not (p.is_contiguous() and p.dtype == torch.float32)
        good = nn.Parameter(torch.randn(5000).cuda())
        opt = make([good, p])
        good.grad, p.grad = torch.ones_like(good), torch.ones_like(p)
        before, v0 = good.detach().clone(), good._version
        with pytest.raises(TypeError):
            opt.step()
        torch.cuda.synchronize()
        assert torch.equal(good, before) and good._version == v0, what      # the valid neighbour was not updated
        assert not opt.state.get(good)                                      # and has no half-initialised state
    if kind == "adam":
        with pytest.raises(NotImplementedError):
            FusedAdam(pa[:2], amsgrad=True)
        with pytest.raises(NotImplementedError):
            FusedAdam(pa[:2], maximize=True)
        with pytest.raises(NotImplementedError):
            FusedAdam(pa[:2], capturable=True)
        with pytest.raises(NotImplementedError):
            FusedAdam([{"params": pa[:1]}, {"params": pa[1:2], "betas": (0.5, 0.999)}], betas=(0.9, 0.999))
        opt = FusedAdam([{"params": pa[:1]}, {"params": pa[1:2]}])
        opt.param_groups[1]["eps"] = 1e-6                    # poked after construction
        pa[0].grad, pa[1].grad = torch.ones_like(pa[0]), torch.ones_like(pa[1])
        before = pa[0].detach().clone()
        with pytest.raises(NotImplementedError):
            opt.step()
        assert torch.equal(pa[0], before)
        sparse = nn.Parameter(torch.randn(6, 4).cuda())
        opt = FusedAdam([sparse])
        sparse.grad = torch.ones(6, 4).cuda().to_sparse()
        with pytest.raises(TypeError):
            opt.step()


@functools.lru_cache(maxsize=None)
def rn101_state(seed):
    return N.resnet101_state(seed=seed, randomize_bn=True, he_init=True, residual_gain=0.25, aspp_gain=0.2)


@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_training_with_the_fused_optimisers_equals_torch(kind):
    """Three SAC-free training steps of the RN101 model (the scenario of test_training_with_fused_sgd_equals_torch_sgd):
    fused="all" and torch's optimiser give the same loss curve, i.e. the packed-weight / BN-fold caches see every
    raw-pointer update of the new kernels."""
    import models
    import driver
    from dasac_hip.optim import FusedAdam, FusedSGD
    cfg = model_cfg(**(dict(OPT="Adam", BETA1=0.5) if kind == "adam" else dict(OPT_NESTEROV=True)))
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 3, 41, 49, generator=g).cuda()
    y = torch.randint(0, 19, (2, 41, 49), generator=g).cuda()
    curves = []
    for fused in ("all", False):
        net = models.DeepLabV2_ResNet101(num_classes=19, criterion=CRIT, freeze_bn=True)
        net.load_state_dict(rn101_state(4), strict=True)
        net.cuda().train()
        cfg2 = copy.copy(cfg)
        cfg2.LR = 1e-3                                       # 4x the reference LR: the updates matter within 3 steps
        opt = driver.make_optimizer(net, cfg2, fused=fused)
        assert type(opt) is {("adam", "all"): FusedAdam, ("adam", False): torch.optim.Adam, ("nesterov", "all"): FusedSGD,
                             ("nesterov", False): torch.optim.SGD}[(kind, fused)]
        losses = []
        for _ in range(3):
            l, _ = net(x, y)
            opt.zero_grad()
            l["loss_ce"].mean().backward()
            opt.step()
            losses.append(float(l["loss_ce"].mean()))
        curves.append(losses)
    print("loss curves ({}): fused {}  torch {}".format(kind, *curves))
    assert curves[0][0] != curves[0][2]
    for a, b in zip(*curves):
        assert a == pytest.approx(b, rel=1e-5)


@pytest.fixture(scope="module")
def sac_net():
    import models
    import driver
    from oracle.step_ref import DEFAULT_CFG
    from types import SimpleNamespace as NS
    cfg = NS(**dict(DEFAULT_CFG, INIT_MODEL="", OPT_NESTEROV=False))
    net = models.get_model(cfg, 0, num_classes=19, criterion=CRIT)
    net.cuda().train()
    src, tgt = driver.synthetic_batches(2, 1, 2, (33, 49), "cuda", seed=5)
    return cfg, net, src, tgt


def recorded_iterations(sac_net, overrides, fused, fuse):
    """The scenario of tests/test_gpu_no_aten_compute.py with another optimiser: one warm-up iteration, then two recorded."""
    import driver
    from types import SimpleNamespace as NS
    from test_gpu_no_aten_compute import Recorder
    cfg, net, src, tgt = sac_net
    cfg = NS(**dict(vars(cfg), **overrides))
    net.backbone.load_state_dict(rn101_state(3), strict=True)
    optim = driver.make_optimizer(net, cfg, fused=fused)
    clone = lambda: (tgt[0], tgt[1].clone(), tgt[2], tgt[3], tgt[4])
    driver.sac_train_iteration(net, optim, src, clone(), 2, True, cfg.LR_TARGET, fuse_passes=fuse)
    big = []
    for update in (True, False):
        with Recorder() as rec:
            driver.sac_train_iteration(net, optim, src, clone(), 2, update, cfg.LR_TARGET, fuse_passes=fuse)
            torch.cuda.synchronize()
        big += rec.big
    return optim, big


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_one_training_iteration_with_the_fused_optimisers_runs_no_aten_arithmetic(sac_net, kind, fuse):
    overrides = dict(OPT="Adam", BETA1=0.5) if kind == "adam" else dict(OPT_NESTEROV=True)
    optim, big = recorded_iterations(sac_net, overrides, "all", fuse)
    assert hasattr(optim, "stash_grads")
    assert not big, sorted(set(big))[:12]


def test_the_recorder_does_see_torchs_adam(sac_net):
    """Control: under fused=True, OPT == "Adam" is torch.optim.Adam, whose foreach kernels are ATen arithmetic."""
    optim, big = recorded_iterations(sac_net, dict(OPT="Adam", BETA1=0.5), True, False)
    assert type(optim) is torch.optim.Adam
    assert big
