"""Global L2 gradient-norm clipping, the logged norm and non-finite step skipping inside the fused optimisers
(`max_grad_norm`, `track_grad_norm`, `skip_nonfinite`; dasac_grad_norm and the `_ctl` update entry points).

Shapes: those of tests/test_gpu_fused_optim.py (1 element; 4097 = one chunk + 1; 85.5 chunks; a parameter whose gradient is all
zero; one whose first gradient arrives a step late), three groups with their own lr / weight decay, and the gradient of the
85.5-chunk tensor handed over as a view one element (4 bytes) into a flat buffer: the norm pass and Adam then take their
scalar paths for it.

Tolerances.  None of ours: the fused result and torch's fp32 result (`p.grad = g2 + g; clip_grad_norm_; torch.optim.X.step()`)
are both compared with the same rule in fp64, and rel_err(fused, fp64) <= 2 * rel_err(torch fp32, fp64) + 1e-7 must hold for
every tensor (2: one differently rounded operation per element -- the norm is summed in double here and in fp32 there, the
coefficient differs by an ulp at most; 1e-7: about one fp32 ulp, for tensors on which torch happens to be exact).  Where the
operation order is the same the comparison is torch.equal.  Non-finite arithmetic (skip_nonfinite=False) is compared element by
element with NaNs in the same places and 1e-6 relative elsewhere: the project's bound for the same-operation-order SGD kernel
(tests/test_gpu_optim.py), a few fp32 ulps of each element."""
import pytest
import torch
import torch.nn as nn

from conftest import rel_err
from test_gpu_fused_optim import (LATE, SHAPES, ZERO, Fp64Adam, assert_versions_advanced, clones, make_params, rn101_state, sac_net,  # noqa: F401
                                  stash_scenario, three_groups, versions)

pytestmark = pytest.mark.gpu

UNALIGNED = 3                 # (19, 2048, 3, 3): its gradients are views at a 4-byte offset that is no multiple of 16
KINDS = ["sgd", "nesterov", "adam0.5", "adam0.9"]
STATE = {"sgd": ("momentum_buffer",), "nesterov": ("momentum_buffer",), "adam0.5": ("exp_avg", "exp_avg_sq"), "adam0.9": ("exp_avg", "exp_avg_sq")}


def fused(kind, groups, **kw):
    from dasac_hip.optim import FusedAdam, FusedSGD
    if kind.startswith("adam"):
        return FusedAdam(groups, betas=(float(kind[4:]), 0.999), **kw)
    return FusedSGD(groups, momentum=0.9, nesterov=kind == "nesterov", **kw)


def torch_optim(kind, groups):
    if kind.startswith("adam"):
        return torch.optim.Adam(groups, betas=(float(kind[4:]), 0.999))
    return torch.optim.SGD(groups, momentum=0.9, nesterov=kind == "nesterov")


class Fp64Sgd:
    """torch.optim.SGD's rule (momentum, dampening 0, nesterov or not, L2 weight decay in the gradient) in fp64 torch ops."""

    def __init__(self, groups, momentum, nesterov):
        self.groups, self.momentum, self.nesterov, self.state = groups, momentum, nesterov, {}

    @torch.no_grad()
    def step(self):
        for gr in self.groups:
            for p in gr["params"]:
                if p.grad is None:
                    continue
                d = p.grad.to(torch.float64)
                if gr["weight_decay"] != 0:
                    d = d + gr["weight_decay"] * p
                st = self.state.setdefault(p, {})
                st["momentum_buffer"] = d.clone() if "momentum_buffer" not in st else st["momentum_buffer"] * self.momentum + d
                p -= gr["lr"] * (d + self.momentum * st["momentum_buffer"] if self.nesterov else st["momentum_buffer"])


def fp64_optim(kind, groups):
    if kind.startswith("adam"):
        return Fp64Adam(groups, (float(kind[4:]), 0.999))
    return Fp64Sgd(groups, 0.9, kind == "nesterov")


def offset_view(t):
    """The same values as a view one element into a flat buffer: a 4-byte offset from a 16-byte aligned allocation."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:].copy_(t.reshape(-1))
    v = flat[1:].view(t.shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def draw(g, it, late=True):
    """One gradient per parameter of SHAPES on the host (None for the late parameter on step 0; all zero for ZERO)."""
    out = []
    for i, s in enumerate(SHAPES):
        if late and it == 0 and i == LATE:
            out.append(None)
        else:
            out.append(torch.zeros(s) if i == ZERO else torch.randn(s, generator=g))
    return out


def give(ps, grads, place=False):
    """p.grad = the gradient, on the device in the parameter's dtype; place: UNALIGNED's through offset_view."""
    for i, (p, gr) in enumerate(zip(ps, grads)):
        if gr is None:
            p.grad = None
            continue
        t = gr.to(device="cuda", dtype=p.dtype)
        p.grad = offset_view(t) if place and i == UNALIGNED else t


def two_pass(opt, ps, g1, g2):
    """The fused side of driver.sac_train_iteration: first-pass gradients stashed, second-pass gradients in .grad.  Parameter 0
    takes part in the second pass only, parameter 1 in the first pass only."""
    opt.zero_grad()
    give(ps, [None if i == 0 else gr for i, gr in enumerate(g1)], place=True)
    opt.stash_grads()
    give(ps, [None if i == 1 else gr for i, gr in enumerate(g2)], place=True)


def summed(g1, g2):
    """What AccumulateGrad leaves in .grad after both passes of two_pass: the fp32 sum g1 + g2 (on the host: the same rounding)."""
    out = []
    for i, (a, b) in enumerate(zip(g1, g2)):
        a, b = (None if i == 0 else a), (None if i == 1 else b)
        out.append(b if a is None else (a if b is None else a + b))
    return out


def norms_of(grads):
    """(fp64 norm, the norm torch's fp32 clip_grad_norm_ returns on the device) of one gradient per parameter."""
    have = [gr for gr in grads if gr is not None]
    exact = torch.linalg.vector_norm(torch.cat([gr.to(device="cuda", dtype=torch.float64).reshape(-1) for gr in have]))
    ps = [nn.Parameter(torch.zeros(gr.shape, device="cuda")) for gr in have]
    give(ps, have)
    return float(exact), float(torch.nn.utils.clip_grad_norm_(ps, float("inf")))


@pytest.mark.parametrize("stash", [False, True])
@pytest.mark.parametrize("kind", ["nesterov", "adam0.5"])             # the 48-byte and the 64-byte table
def test_norm_matches_fp64_within_torchs_own_fp32_error_and_repeats_bit_for_bit(kind, stash):
    g, pa = make_params(21)
    opt = fused(kind, three_groups(pa), track_grad_norm=True)
    assert opt.max_grad_norm is None and float(opt.grad_norm) == 0.0 and int(opt.skipped_steps) == 0
    before = [p.detach().clone() for p in pa]
    for it in range(2):                                                   # step 0 without the late parameter
        g1, g2 = draw(g, it), draw(g, it)
        if stash:
            two_pass(opt, pa, g1, g2)
            applied = summed(g1, g2)
        else:
            give(pa, g1, place=True)
            applied = g1
        exact, torch32 = norms_of(applied)
        first, second = opt.measure_grad_norm(), opt.measure_grad_norm()
        assert first.dtype == torch.float32 and first.dim() == 0 and first.is_cuda
        assert torch.equal(first, second)
        if it == 0:
            assert all(torch.equal(p, b) for p, b in zip(pa, before)) and not opt.state      # measuring updates nothing
        opt.step()
        stepped = opt.grad_norm
        assert stepped.dtype == torch.float32 and stepped.dim() == 0 and stepped.is_cuda
        assert torch.equal(stepped, first)
        e_x, e_ref = abs(float(first) - exact) / exact, abs(torch32 - exact) / exact
        print("norm {} stash={} step {}: fp64 {:.9e}  fused {:.9e} (rel_err {:.3e})  torch fp32 {:.9e} (rel_err {:.3e})".format(
            kind, stash, it, exact, float(first), e_x, torch32, e_ref))
        assert e_x <= 2 * e_ref + 1e-7, (e_x, e_ref)
    assert not any(torch.equal(p, b) for i, (p, b) in enumerate(zip(pa, before)) if i != ZERO)     # track_grad_norm does not clip or skip
    assert int(opt.skipped_steps) == 0


def within_reference_error(tag, keys, opt_x, px, opt_b, pb, ref, pc, report):
    """rel_err(x, fp64) <= 2 * rel_err(torch fp32, fp64) + 1e-7 for every parameter and state tensor; returns bit equality."""
    same = True
    for i, (x, b, c) in enumerate(zip(px, pb, pc)):
        trio = [("param", x, b, c)]
        if c in ref.state:
            trio += [(k, opt_x.state[x][k], opt_b.state[b][k], ref.state[c][k]) for k in keys]
        for name, tx, tb, tc in trio:
            assert torch.isfinite(tx).all()
            e_x, e_ref = rel_err(tx, tc), rel_err(tb, tc)
            report.append((tag, i, name, e_x, e_ref))
            same = same and torch.equal(tx, tb)
            assert e_x <= 2 * e_ref + 1e-7, (tag, i, name, e_x, e_ref)
    return same


def print_report(title, keys, report, same):
    for name in ("param",) + tuple(keys):
        rows = [r for r in report if r[2] == name]
        tight = max(rows, key=lambda r: r[3] - (2 * r[4] + 1e-7))
        print("{}: {:<15} max rel_err vs fp64: fused {:.3e}  torch fp32 {:.3e};  nearest the bound: {} tensor {} fused {:.3e} torch {:.3e}".format(
            title, name, max(r[3] for r in rows), max(r[4] for r in rows), tight[0], tight[1], tight[3], tight[4]))
    print("{}: bit-identical to clip_grad_norm_ + torch's optimiser on every tensor and step: {}".format(title, same))


@pytest.mark.parametrize("kind", KINDS)
def test_active_clipping_matches_clip_grad_norm_within_torchs_own_fp32_error(kind):
    g, pa = make_params(3)
    pb, pc = clones(pa), clones(pa, torch.float64)
    oa, ob, ref = fused(kind, three_groups(pa), max_grad_norm=1.0), torch_optim(kind, three_groups(pb)), fp64_optim(kind, three_groups(pc))
    assert oa.max_grad_norm == 1.0 and not oa.skip_nonfinite
    keys, report, same = STATE[kind], [], True
    for it in range(5):
        g1, g2 = draw(g, it), draw(g, it)
        two_pass(oa, pa, g1, g2)
        give(pb, summed(g1, g2))
        give(pc, summed(g1, g2))
        if it == 2:
            for o in (oa, ob):
                o.param_groups[1]["lr"] = 1e-3               # schedules poke param_groups
            ref.groups[1]["lr"] = 1e-3
        n32 = torch.nn.utils.clip_grad_norm_(pb, 1.0)
        n64 = torch.nn.utils.clip_grad_norm_(pc, 1.0)
        assert float(n64) > 100.0                            # far from the clamp: an ulp of the norm cannot switch it
        v0 = versions(oa, pa, keys)
        oa.step()
        ob.step()
        ref.step()
        assert_versions_advanced(oa, pa, keys, v0)           # the engine caches key on this
        assert abs(float(oa.grad_norm) - float(n64)) / float(n64) <= 2 * abs(float(n32) - float(n64)) / float(n64) + 1e-7
        same = within_reference_error("step %d" % it, keys, oa, pa, ob, pb, ref, pc, report) and same
    print_report("clip " + kind, keys, report, same)
    assert int(oa.skipped_steps) == 0


@pytest.mark.parametrize("kind", KINDS)
def test_inactive_clipping_is_bit_identical_to_no_clipping(kind):
    g, pa = make_params(4)
    pb = clones(pa)
    oa, ob = fused(kind, three_groups(pa), max_grad_norm=1e6), fused(kind, three_groups(pb))
    for it in range(3):
        g1, g2 = draw(g, it), draw(g, it)
        two_pass(oa, pa, g1, g2)
        two_pass(ob, pb, g1, g2)
        oa.step()
        ob.step()
        for a, b in zip(pa, pb):
            assert torch.equal(a, b) and set(oa.state[a]) == set(ob.state[b])
            for k in STATE[kind]:
                if k in ob.state[b]:
                    assert torch.equal(oa.state[a][k], ob.state[b][k]), k
    assert 100.0 < float(oa.grad_norm) < 1e4


@pytest.mark.parametrize("kind", ["sgd", "nesterov", "adam0.5"])
def test_default_keywords_leave_the_plain_path_alone(kind):
    """Canary: nothing of the control-block plumbing runs unless asked for -- the step is what it was (bit-identical to torch for
    the kernels that share ATen's operation order and contraction; the plain-momentum kernel within its 1e-6,
    tests/test_gpu_optim.py)."""
    g, pa = make_params(6)
    pb = clones(pa)
    oa, ob = fused(kind, three_groups(pa)), torch_optim(kind, three_groups(pb))
    assert (oa.max_grad_norm, oa.skip_nonfinite, oa.track_grad_norm) == (None, False, False)
    for it in range(2):
        grads = draw(g, it)
        give(pa, grads, place=True)
        give(pb, grads)
        oa.step()
        ob.step()
    assert oa._ctl is None and "ctl" not in oa._tables       # no control block was ever allocated, no combined table built
    for a, b in zip(pa, pb):
        for x, y in [(a, b)] + [(oa.state[a][k], ob.state[b][k]) for k in STATE[kind]]:
            assert rel_err(x, y) < 1e-6 if kind == "sgd" else torch.equal(x, y)


def all_state(opt, ps, keys):
    return [p.detach().clone() for p in ps] + [opt.state[p][k].detach().clone() for p in ps for k in keys]


def poisoned(g, bad):
    grads = draw(g, 1)
    grads[LATE].view(-1)[4096] = bad                         # the last, partial chunk of the 4097-element gradient
    return grads


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("kind", ["sgd", "nesterov", "adam0.5"])
def test_a_nonfinite_gradient_skips_the_step_on_the_device(kind, bad):
    g, pa = make_params(8)
    keys = STATE[kind]
    oa = fused(kind, three_groups(pa), skip_nonfinite=True)
    start = [p.detach().clone() for p in pa]
    give(pa, poisoned(g, bad), place=True)
    oa.step()                                                # skipped: the very first step
    assert int(oa.skipped_steps) == 1 and not torch.isfinite(oa.grad_norm)
    assert all(torch.equal(p, s) for p, s in zip(pa, start))
    for p in pa:                                             # fresh state: Adam's zeros untouched, SGD's new buffer 0
        assert all(not oa.state[p][k].any() for k in keys)
    # a finite step next: exactly the step a fresh optimiser takes (for Adam: one whose host step count is one ahead)
    pb = clones(pa)
    ob = fused(kind, three_groups(pb))
    if kind.startswith("adam"):
        for p in pb:
            ob.state[p] = {"step": torch.tensor(1.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
    grads = draw(g, 1)
    give(pa, grads, place=True)
    give(pb, grads, place=True)
    v0 = versions(oa, pa, keys)
    oa.step()
    ob.step()
    assert_versions_advanced(oa, pa, keys, v0)
    assert int(oa.skipped_steps) == 1 and torch.isfinite(oa.grad_norm)
    for a, b in zip(pa, pb):
        assert torch.equal(a, b)
        for k in keys:
            assert torch.equal(oa.state[a][k], ob.state[b][k]), k
    assert not torch.equal(pa[0], start[0])
    # a later step is skipped the same way: everything bit-unchanged, moments included
    snap = all_state(oa, pa, keys)
    give(pa, poisoned(g, bad), place=True)
    oa.step()
    assert int(oa.skipped_steps) == 2 and not torch.isfinite(oa.grad_norm)
    assert all(torch.equal(x, y) for x, y in zip(all_state(oa, pa, keys), snap))
    assert not oa._stash


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("kind", ["sgd", "adam0.5"])
def test_without_skipping_a_nonfinite_norm_clips_as_torch_does(kind, bad):
    """error_if_nonfinite=False: an Inf norm gives the coefficient 0 (Inf * 0 = NaN in one element, 0 elsewhere), a NaN norm a
    NaN coefficient (everything NaN)."""
    g, pa = make_params(9)
    pb = clones(pa)
    keys = STATE[kind]
    oa, ob = fused(kind, three_groups(pa), max_grad_norm=1.0), torch_optim(kind, three_groups(pb))
    grads = poisoned(g, bad)
    give(pa, grads, place=True)
    give(pb, grads)
    torch.nn.utils.clip_grad_norm_(pb, 1.0, error_if_nonfinite=False)
    oa.step()
    ob.step()
    assert int(oa.skipped_steps) == 0 and not torch.isfinite(oa.grad_norm)
    nans = 0
    for a, b in zip(pa, pb):
        for x, y in [(a, b)] + [(oa.state[a][k], ob.state[b][k]) for k in keys]:
            assert torch.allclose(x, y, rtol=1e-6, atol=0.0, equal_nan=True)
            nans += int(torch.isnan(x).sum())
    assert nans >= (1 if bad == float("inf") else sum(p.numel() for p in pa))


@pytest.mark.parametrize("kind", ["sgd", "nesterov", "adam0.5"])
def test_stashed_gradients_are_clipped_by_the_norm_of_their_sum_bit_for_bit(kind):
    """stash_scenario: backward, stash_grads(), backward, step() against the unstashed run that accumulated into .grad; with
    clipping on, both see the norm of g2 + g (were it the norm of g alone, the coefficients and every tensor would differ)."""
    stash_scenario(lambda gs: fused(kind, gs, max_grad_norm=1.0))


@pytest.mark.parametrize("kind", ["sgd", "adam0.5"])
def test_version_counters_advance_on_a_clipped_step(kind):
    g, pa = make_params(10, [(64,), (4097,)])
    oa = fused(kind, [{"params": pa, "lr": 1e-2}], max_grad_norm=1.0, skip_nonfinite=True)
    for it in range(2):                                      # the step that creates the state and one that finds it
        for p in pa:
            p.grad = torch.randn(p.shape, generator=g).cuda()
        before = {id(t): t._version for p in pa for t in [p] + [oa.state[p][k] for k in STATE[kind] if p in oa.state]}
        oa.step()
        for p in pa:
            for t in [p] + [oa.state[p][k] for k in STATE[kind]]:
                assert t._version > before.get(id(t), -1)
    assert int(oa.skipped_steps) == 0


@pytest.mark.parametrize("fuse", [False, True])
@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_one_clipped_training_iteration_runs_no_aten_arithmetic(sac_net, kind, fuse):
    """The scenario of test_one_training_iteration_with_the_fused_optimisers_runs_no_aten_arithmetic with clipping and
    skipping switched on: one warm-up iteration, then two recorded."""
    import driver
    from types import SimpleNamespace as NS
    from test_gpu_no_aten_compute import Recorder
    cfg, net, src, tgt = sac_net
    cfg = NS(**dict(vars(cfg), **(dict(OPT="Adam", BETA1=0.5) if kind == "adam" else {})))
    net.backbone.load_state_dict(rn101_state(3), strict=True)
    optim = driver.make_optimizer(net, cfg, max_grad_norm=1.0, skip_nonfinite=True)
    assert optim.max_grad_norm == 1.0 and optim.skip_nonfinite
    clone = lambda: (tgt[0], tgt[1].clone(), tgt[2], tgt[3], tgt[4])
    driver.sac_train_iteration(net, optim, src, clone(), 2, True, cfg.LR_TARGET, fuse_passes=fuse)
    big = []
    for update in (True, False):
        with Recorder() as rec:
            driver.sac_train_iteration(net, optim, src, clone(), 2, update, cfg.LR_TARGET, fuse_passes=fuse)
            torch.cuda.synchronize()
        big += rec.big
    assert not big, sorted(set(big))[:12]
    assert float(optim.grad_norm) > 0.0 and torch.isfinite(optim.grad_norm) and int(optim.skipped_steps) == 0
