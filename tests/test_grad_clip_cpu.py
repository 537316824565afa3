"""Host side of gradient-norm clipping / non-finite step skipping in the fused optimisers (no GPU): keyword validation, the
`driver.make_optimizer` plumbing, torch's `param_groups` / `state_dict()` layouts with clipping configured, the new entry points
declared, exported and bound with matching arity, and the refusal of CPU parameters before any state exists."""
import ctypes
import os
import re
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn as nn

from oracle.step_ref import DEFAULT_CFG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dasac_grad_norm_workspace", "dasac_grad_norm", "dasac_sgd_step_ctl", "dasac_sgd_nesterov_step_ctl", "dasac_adam_step_ctl")


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def makers():
    from dasac_hip.optim import FusedAdam, FusedSGD
    return [lambda ps, **kw: FusedAdam(ps, lr=0.1, **kw), lambda ps, **kw: FusedSGD(ps, lr=0.1, momentum=0.9, **kw),
            lambda ps, **kw: FusedSGD(ps, lr=0.1, momentum=0.9, nesterov=True, **kw)]


@pytest.mark.parametrize("bad", [0, 0.0, -1.0, float("nan"), float("inf"), -float("inf"), "1.0", True])
def test_max_grad_norm_must_be_a_finite_positive_number_or_none(bad):
    for make in makers():
        with pytest.raises(ValueError):
            make([nn.Parameter(torch.zeros(3))], max_grad_norm=bad)


def test_keywords_are_attributes_with_off_defaults():
    for make in makers():
        p = [nn.Parameter(torch.zeros(3))]
        off = make(p)
        assert (off.max_grad_norm, off.skip_nonfinite, off.track_grad_norm) == (None, False, False)
        on = make(p, max_grad_norm=2, skip_nonfinite=1, track_grad_norm=True)
        assert on.max_grad_norm == 2.0 and isinstance(on.max_grad_norm, float) and on.skip_nonfinite is True and on.track_grad_norm is True
        assert all(callable(getattr(on, m)) for m in ("measure_grad_norm", "stash_grads", "full_grads"))
        assert isinstance(type(on).grad_norm, property) and isinstance(type(on).skipped_steps, property)


def test_groups_and_state_dict_keep_torchs_layout_with_clipping_configured():
    from dasac_hip.optim import FusedAdam, FusedSGD
    ps = [nn.Parameter(torch.zeros(3)), nn.Parameter(torch.zeros(2, 2))]
    groups = lambda: [{"params": ps[:1], "lr": 1e-2}, {"params": ps[1:], "weight_decay": 1e-3}]
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True, track_grad_norm=True)
    pairs = [(FusedAdam(groups(), lr=1e-3, betas=(0.5, 0.999), **kw), torch.optim.Adam(groups(), lr=1e-3, betas=(0.5, 0.999))),
             (FusedSGD(groups(), lr=1e-3, momentum=0.9, nesterov=True, **kw), torch.optim.SGD(groups(), lr=1e-3, momentum=0.9, nesterov=True))]
    plain = {FusedAdam: FusedAdam(groups(), lr=1e-3, betas=(0.5, 0.999)), FusedSGD: FusedSGD(groups(), lr=1e-3, momentum=0.9, nesterov=True)}
    for fused, ref in pairs:
        assert [set(g) for g in fused.param_groups] == [set(g) for g in plain[type(fused)].param_groups]      # what they were without
        if isinstance(fused, FusedAdam):
            assert set(fused.param_groups[0]) == set(ref.param_groups[0])
        else:
            assert set(fused.param_groups[0]) <= set(ref.param_groups[0])      # FusedSGD: the keys its kernel has (no foreach / fused ...)
        assert not {"max_grad_norm", "skip_nonfinite", "track_grad_norm"} & set(fused.param_groups[0])
        sd = fused.state_dict()
        assert set(sd) == set(ref.state_dict()) == {"state", "param_groups"}
        assert not {"max_grad_norm", "skip_nonfinite", "track_grad_norm"} & set(sd["param_groups"][0])
        ref.load_state_dict(sd)
        fused.load_state_dict(ref.state_dict())
        assert fused.max_grad_norm == 1.0 and fused.skip_nonfinite and fused.track_grad_norm      # loading a checkpoint leaves them alone
        assert fused.param_groups[0]["lr"] == 1e-2 and fused.param_groups[1]["weight_decay"] == 1e-3


def test_make_optimizer_passes_the_keywords_and_implies_fused_all():
    import models
    import driver
    from dasac_hip.optim import FusedAdam, FusedSGD
    cfg = NS(**dict(DEFAULT_CFG, INIT_MODEL="", OPT_NESTEROV=False))
    net = models.get_model(cfg, 0, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    net.train()
    with_cfg = lambda **kw: NS(**dict(vars(cfg), **kw))
    cases = [(cfg, FusedSGD, False), (with_cfg(OPT_NESTEROV=True), FusedSGD, True), (with_cfg(OPT="Adam", BETA1=0.5), FusedAdam, None)]
    for c, cls, nesterov in cases:
        for fused in (True, "all"):                          # the default fused=True would give torch's class for two of them
            opt = driver.make_optimizer(net, c, fused=fused, max_grad_norm=0.5)
            assert type(opt) is cls and opt.max_grad_norm == 0.5 and opt.skip_nonfinite is False and opt.track_grad_norm is False
            if nesterov is not None:
                assert all(g["nesterov"] is nesterov for g in opt.param_groups)
        opt = driver.make_optimizer(net, c, skip_nonfinite=True)
        assert type(opt) is cls and opt.max_grad_norm is None and opt.skip_nonfinite is True
        opt = driver.make_optimizer(net, c, max_grad_norm=3.0, skip_nonfinite=True)
        assert type(opt) is cls and opt.max_grad_norm == 3.0 and opt.skip_nonfinite is True
        assert [g["weight_decay"] for g in opt.param_groups] == [5e-4, 0.0, 5e-4, 0.0]
        for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True)):
            with pytest.raises(ValueError):
                driver.make_optimizer(net, c, fused=False, **kw)
        with pytest.raises(ValueError):
            driver.make_optimizer(net, c, max_grad_norm=-1.0)
    with pytest.raises(ValueError):                          # no fused class for this one
        driver.make_optimizer(net, with_cfg(OPT="RMSprop"), fused="all", max_grad_norm=1.0)
    # without the keywords the factory is what it was
    assert type(driver.make_optimizer(net, with_cfg(OPT="Adam"))) is torch.optim.Adam
    assert type(driver.make_optimizer(net, with_cfg(OPT="RMSprop"), fused="all")) is torch.optim.RMSprop
    assert driver.make_optimizer(net, cfg).max_grad_norm is None


def test_new_entry_points_are_declared_exported_and_bound():
    from dasac_hip import lib as L
    txt = open(os.path.join(ROOT, "include", "dasac_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decls = dict(re.findall(r"\b(dasac_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt))
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert name in decls and hasattr(raw, name)
        params = [a.strip() for a in decls[name].split(",")]
        res, argtypes = L.PROTOTYPES[name]
        assert res is (ctypes.c_size_t if name.endswith("_workspace") else ctypes.c_int)
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for p, t in zip(params, argtypes):
            if p.startswith(("float ", "double ")):
                assert t is (ctypes.c_float if p.startswith("float ") else ctypes.c_double), (name, p, t)
    # the old arguments, then the control block, the two flags and the stream
    tail = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    for old in ("dasac_sgd_step", "dasac_sgd_nesterov_step", "dasac_adam_step"):
        assert L.PROTOTYPES[old + "_ctl"] == (ctypes.c_int, L.PROTOTYPES[old][1][:-1] + tail)
    lib = L.load()
    assert lib.dasac_grad_norm_workspace(0) == 0 and lib.dasac_grad_norm_workspace(86) == 86 * 8      # one double per chunk
    assert lib.dasac_version() == 1


def test_bad_arguments_are_refused_before_any_launch():
    """The C entry points validate on the host (no device needed for a refusal)."""
    from dasac_hip import lib as L
    lib = L.load()
    assert lib.dasac_grad_norm(None, 48, 1, None, 1, 1.0, None, 0, None, None, None) != 0
    buf = (ctypes.c_double * 8)()
    at = ctypes.addressof(buf)
    assert at % 8 == 0
    assert lib.dasac_grad_norm(at, 40, 1, at, 1, 1.0, at, 64, at, None, None) != 0          # no such table layout
    assert b"row_bytes" in lib.dasac_last_error()
    assert lib.dasac_grad_norm(at, 48, 1, at, 9, 1.0, at, 64, at, None, None) != 0          # 9 chunks need 72 bytes
    assert b"workspace" in lib.dasac_last_error()
    wd = (ctypes.c_float * 1)(0.0)
    assert lib.dasac_adam_step_ctl(at, 1, at, 1, ctypes.cast(wd, ctypes.c_void_p), 1, 0.5, 0.999, 1e-8, None, 1, 1, None) != 0
    assert b"control block" in lib.dasac_last_error()


@pytest.mark.parametrize("which", [0, 1, 2])
def test_clipping_optimisers_refuse_cpu_parameters_before_touching_any_state(which):
    from dasac_hip import DasacError
    p = nn.Parameter(torch.ones(5))
    opt = makers()[which]([p], max_grad_norm=1.0, skip_nonfinite=True, track_grad_norm=True)
    opt.step()                                               # no gradient anywhere: nothing to do, nothing to refuse
    p.grad = torch.ones(5)
    with pytest.raises(DasacError):
        opt.step()
    with pytest.raises(DasacError):
        opt.measure_grad_norm()
    with pytest.raises(DasacError):
        opt.grad_norm
    assert torch.equal(p.detach(), torch.ones(5)) and not opt.state.get(p) and torch.equal(p.grad, torch.ones(5))
