"""Host side of the fused optimisers (no GPU): `driver.make_optimizer(..., fused="all")` follows the reference's factory
(base_trainer.py:47-73) with the HIP classes, construction needs no device, step() on CPU parameters raises the project's usual
error (no CPU fallback), and the new entry points are declared, exported and bound with matching arity."""
import ctypes
import os
import re
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn as nn

from oracle.step_ref import DEFAULT_CFG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dasac_sgd_nesterov_step", "dasac_adam_step")


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def test_make_optimizer_fused_all_returns_the_hip_classes():
    import models
    import driver
    from dasac_hip.optim import FusedAdam, FusedSGD
    cfg = NS(**dict(DEFAULT_CFG, INIT_MODEL="", OPT_NESTEROV=False))
    net = models.get_model(cfg, 0, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    net.train()
    with_cfg = lambda **kw: NS(**dict(vars(cfg), **kw))
    plain = driver.make_optimizer(net, cfg, fused="all")
    assert type(plain) is FusedSGD and not plain.param_groups[0]["nesterov"]
    nes = driver.make_optimizer(net, with_cfg(OPT_NESTEROV=True), fused="all")
    assert type(nes) is FusedSGD and all(g["nesterov"] is True for g in nes.param_groups) and nes.param_groups[0]["momentum"] == 0.9
    adam = driver.make_optimizer(net, with_cfg(OPT="Adam", BETA1=0.5), fused="all")
    assert type(adam) is FusedAdam and all(g["betas"] == (0.5, 0.999) for g in adam.param_groups)
    for opt in (nes, adam):
        assert [g["lr"] for g in opt.param_groups] == pytest.approx([2.5e-4, 5e-4, 2.5e-3, 5e-3])
        assert [g["weight_decay"] for g in opt.param_groups] == [5e-4, 0.0, 5e-4, 0.0]
        assert all(hasattr(opt, m) for m in ("stash_grads", "full_grads", "zero_grad"))
    # the defaults are what they were: torch's classes unless the caller opts in
    assert type(driver.make_optimizer(net, with_cfg(OPT_NESTEROV=True))) is torch.optim.SGD
    assert type(driver.make_optimizer(net, with_cfg(OPT="Adam"), fused=True)) is torch.optim.Adam
    assert type(driver.make_optimizer(net, with_cfg(OPT="Adam"), fused=False)) is torch.optim.Adam
    assert type(driver.make_optimizer(net, with_cfg(OPT_NESTEROV=True), fused=False)) is torch.optim.SGD
    assert type(driver.make_optimizer(net, with_cfg(OPT="RMSprop"), fused="all")) is torch.optim.RMSprop
    with pytest.raises(NotImplementedError):
        driver.make_optimizer(net, with_cfg(OPT="NoSuchOptimiser"), fused="all")


def test_fused_adam_has_torch_adams_group_and_state_dict_layout():
    from dasac_hip.optim import FusedAdam
    ps = [nn.Parameter(torch.zeros(3)), nn.Parameter(torch.zeros(2, 2))]
    groups = lambda: [{"params": ps[:1], "lr": 1e-2}, {"params": ps[1:], "weight_decay": 1e-3}]
    fused, ref = FusedAdam(groups(), lr=1e-3, betas=(0.5, 0.999)), torch.optim.Adam(groups(), lr=1e-3, betas=(0.5, 0.999))
    assert [set(g) for g in fused.param_groups] == [set(g) for g in ref.param_groups]
    for a, b in zip(fused.param_groups, ref.param_groups):
        assert all(a[k] == b[k] for k in ("lr", "betas", "eps", "weight_decay", "amsgrad", "maximize", "capturable"))
    ref.load_state_dict(fused.state_dict())
    fused.load_state_dict(ref.state_dict())
    assert fused.param_groups[0]["lr"] == 1e-2 and fused.param_groups[1]["weight_decay"] == 1e-3


@pytest.mark.parametrize("kind", ["adam", "nesterov"])
def test_fused_optimisers_refuse_cpu_parameters_at_step(kind):
    from dasac_hip import DasacError
    from dasac_hip.optim import FusedAdam, FusedSGD
    p = nn.Parameter(torch.ones(5))
    opt = FusedAdam([p], lr=0.1) if kind == "adam" else FusedSGD([p], lr=0.1, momentum=0.9, nesterov=True)
    opt.step()                                               # no gradient anywhere: nothing to do, nothing to refuse
    p.grad = torch.ones(5)
    with pytest.raises(DasacError):
        opt.step()
    assert torch.equal(p.detach(), torch.ones(5)) and not opt.state.get(p)


def test_refusals_that_need_no_device():
    from dasac_hip.optim import FusedAdam, FusedSGD
    ps = [nn.Parameter(torch.zeros(2)) for _ in range(9)]
    for make in (lambda gs: FusedAdam(gs), lambda gs: FusedSGD(gs, momentum=0.9, nesterov=True)):
        with pytest.raises(ValueError):
            make([{"params": [p]} for p in ps])
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(capturable=True)):
        with pytest.raises(NotImplementedError):
            FusedAdam(ps[:1], **kw)
    with pytest.raises(NotImplementedError):
        FusedAdam([{"params": ps[:1]}, {"params": ps[1:2], "betas": (0.5, 0.999)}])
    with pytest.raises(NotImplementedError):
        FusedAdam([{"params": ps[:1]}, {"params": ps[1:2], "eps": 1e-6}])
    with pytest.raises(ValueError):
        FusedSGD(ps[:1], momentum=0.0, nesterov=True)         # torch's condition
    with pytest.raises(NotImplementedError):
        FusedSGD(ps[:1], momentum=0.9, nesterov=True, dampening=0.5)


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
        assert res is ctypes.c_int and len(argtypes) == len(params), (name, len(argtypes), len(params))
        for p, t in zip(params, argtypes):
            if p.startswith(("float ", "double ")):
                assert t is (ctypes.c_float if p.startswith("float ") else ctypes.c_double), (name, p, t)
    # same table layout and arguments as the plain-momentum entry point
    assert L.PROTOTYPES["dasac_sgd_nesterov_step"] == L.PROTOTYPES["dasac_sgd_step"]
    assert L.load().dasac_version() == 1
