"""Host side of the per-tensor gradient health table (no GPU): `driver.gradient_report` / `skipped_step_report` /
`format_gradient_report` over a hand-made table and a three-parameter module, the `track_tensor_stats` keyword, the
`driver.make_optimizer(tensor_stats=)` plumbing, and the host-side refusals of dasac_tensor_stats."""
import ctypes
import math
from types import SimpleNamespace as NS

import pytest
import torch
import torch.nn as nn

from oracle.step_ref import DEFAULT_CFG


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


class Three(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(2, 3, 3)                        # weight [3,2,3,3] = 54 elements, bias [3]
        self.scale = nn.Parameter(torch.ones(5))


#          g_sumsq g_maxabs nonfinite first zeros p_sumsq p_maxabs s_sumsq
TABLE = [[9.0, 2.0, 2.0, 41.0, 6.0, 4.0, 1.5, 0.25],          # conv.weight: first non-finite at flat index 40 = (2, 0, 1, 1)
         [16.0, 4.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0],           # conv.bias: a zero weight norm
         [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]]            # scale: nothing pending


def setup():
    net = Three()
    optim = torch.optim.SGD([{"params": [net.conv.weight, net.scale], "lr": 0.5}, {"params": [net.conv.bias], "lr": 0.1}], lr=1.0)
    # rows in the flattened param_groups order: conv.weight, scale, conv.bias
    table = torch.tensor([TABLE[0], TABLE[2], TABLE[1]], dtype=torch.float64)
    return net, optim, table


def test_gradient_report_reads_shares_ratios_indices_and_groups():
    import driver
    net, optim, table = setup()
    rep = driver.gradient_report(net, optim, table=table, top=2)
    assert [t["name"] for t in rep["tensors"]] == ["conv.weight", "scale", "conv.bias"]
    w, s, b = rep["tensors"]
    assert (w["group"], s["group"], b["group"]) == (0, 0, 1) and (w["numel"], s["numel"], b["numel"]) == (54, 5, 3)
    assert w["grad_norm"] == 3.0 and b["grad_norm"] == 4.0 and rep["grad_norm"] == 5.0
    assert w["share"] == 9.0 / 25.0 and b["share"] == 16.0 / 25.0 and s["share"] == 0.0
    assert w["g_maxabs"] == 2.0 and w["zero_share"] == 6.0 / 54.0 and w["weight_norm"] == 2.0 and w["state_norm"] == 0.5
    assert w["update_ratio"] == 0.5 * 3.0 / 2.0
    assert b["update_ratio"] == 0.0 and b["weight_norm"] == 0.0 and b["state_norm"] == 1.0      # no division by a zero weight norm
    assert w["nonfinite"] == 2 and w["first_nonfinite"] == (2, 0, 1, 1) and b["first_nonfinite"] is None
    # the absent row
    assert s == dict(name="scale", group=0, numel=5, grad_norm=0.0, share=0.0, g_maxabs=0.0, zero_share=0.0, weight_norm=0.0,
                     update_ratio=0.0, state_norm=0.0, nonfinite=0, first_nonfinite=None)
    g0, g1 = rep["groups"]
    assert (g0["group"], g0["lr"], g0["tensors"], g0["numel"]) == (0, 0.5, 2, 59) and (g1["lr"], g1["tensors"], g1["numel"]) == (0.1, 1, 3)
    assert g0["grad_norm"] == 3.0 and g0["share"] == 9.0 / 25.0 and g0["g_maxabs"] == 2.0 and g0["zero_share"] == 6.0 / 59.0
    assert g0["weight_norm"] == 2.0 and g0["state_norm"] == 0.5 and g0["nonfinite"] == 2 and g0["update_ratio"] == 0.75
    assert g1["grad_norm"] == 4.0 and g1["share"] == 16.0 / 25.0 and g1["nonfinite"] == 0
    assert rep["nonfinite"] == ["conv.weight"] and rep["top"] == ["conv.bias", "conv.weight"]
    assert abs(sum(t["share"] for t in rep["tensors"]) - 1.0) < 1e-15
    # a wrapped module is read through .module; a 1-element and a last-element index unravel too
    wrapped = NS(module=net)
    table[0, 3] = 54.0
    assert driver.gradient_report(wrapped, optim, table=table)["tensors"][0]["first_nonfinite"] == (2, 1, 2, 2)
    table[2, 2:4] = torch.tensor([1.0, 3.0], dtype=torch.float64)
    assert driver.gradient_report(wrapped, optim, table=table)["tensors"][2]["first_nonfinite"] == (2,)


def test_an_all_zero_table_gives_zero_shares_not_a_division():
    import driver
    net, optim, table = setup()
    rep = driver.gradient_report(net, optim, table=torch.zeros_like(table))
    assert rep["grad_norm"] == 0.0 and all(t["share"] == 0.0 and t["update_ratio"] == 0.0 for t in rep["tensors"]) and rep["nonfinite"] == []


def test_the_table_must_have_one_row_per_parameter():
    import driver
    net, optim, table = setup()
    with pytest.raises(AssertionError):
        driver.gradient_report(net, optim, table=table[:2])


def test_the_default_table_is_the_optimisers_and_the_skipped_report_adds_captured_at():
    import driver
    net, optim, table = setup()
    fake = NS(param_groups=optim.param_groups, tensor_stats=table, last_skipped_stats=(table.clone(), torch.tensor(3)))
    assert driver.gradient_report(net, fake) == driver.gradient_report(net, optim, table=table)
    rep = driver.skipped_step_report(net, fake)
    assert rep["captured_at"] == 3 and rep["nonfinite"] == ["conv.weight"] and rep["grad_norm"] == 5.0


def test_format_gradient_report_lists_the_top_tensors_and_every_nonfinite_one():
    import driver
    net, optim, table = setup()
    rep = driver.gradient_report(net, optim, table=table)
    lines = driver.format_gradient_report(rep, top=1).split("\n")
    assert lines[0].split()[:4] == ["tensor", "group", "numel", "|g|"]
    assert lines[1].startswith("conv.bias") and lines[2].startswith("conv.weight") and lines[2].endswith("(2, 0, 1, 1)")      # top 1 + the non-finite one
    assert lines[3].startswith("group 0 (lr 0.5, 2 tensors)") and lines[4].startswith("group 1 (lr 0.1, 1 tensors)")
    assert lines[5] == "global gradient norm 5.000000e+00; tensors with non-finite entries: conv.weight" and len(lines) == 6
    assert len({len(l) for l in (lines[1], lines[3], lines[4])}) == 1 and lines[0].index(" group") == lines[1].index("     1")      # fixed width
    full = driver.format_gradient_report(rep).split("\n")
    assert len(full) == 1 + 3 + 2 + 1 and full[3].startswith("scale")
    rep["captured_at"] = 2
    assert driver.format_gradient_report(rep).split("\n")[-1] == "captured at skipped step 2"
    clean = driver.gradient_report(net, optim, table=torch.tensor([TABLE[1], TABLE[2], TABLE[2]], dtype=torch.float64))
    assert driver.format_gradient_report(clean).split("\n")[-1].endswith("non-finite entries: none")


def makers():
    from dasac_hip.optim import FusedAdam, FusedSGD
    return [lambda ps, **kw: FusedAdam(ps, lr=0.1, **kw), lambda ps, **kw: FusedSGD(ps, lr=0.1, momentum=0.9, **kw),
            lambda ps, **kw: FusedSGD(ps, lr=0.1, momentum=0.9, nesterov=True, **kw)]


def test_the_keyword_is_an_attribute_off_by_default_and_not_part_of_the_state_dict():
    from dasac_hip.optim import TENSOR_STATS_COLUMNS
    assert TENSOR_STATS_COLUMNS == ("g_sumsq", "g_maxabs", "g_nonfinite", "g_first_nonfinite", "g_zeros", "p_sumsq", "p_maxabs", "s_sumsq")
    for make in makers():
        p = [nn.Parameter(torch.zeros(3))]
        off, on = make(p), make(p, track_tensor_stats=1)
        assert off.track_tensor_stats is False and not off._controlled()
        assert on.track_tensor_stats is True and on._controlled()      # it implies the controlled path
        assert (on.max_grad_norm, on.skip_nonfinite, on.track_grad_norm) == (None, False, False)
        assert callable(on.measure_tensor_stats) and isinstance(type(on).tensor_stats, property) and isinstance(type(on).last_skipped_stats, property)
        sd = on.state_dict()
        assert set(sd) == {"state", "param_groups"} and "track_tensor_stats" not in sd["param_groups"][0]
        assert [set(g) for g in on.param_groups] == [set(g) for g in off.param_groups]
        on.load_state_dict(off.state_dict())
        assert on.track_tensor_stats is True


@pytest.mark.parametrize("which", [0, 1, 2])
def test_tracking_optimisers_refuse_cpu_parameters_before_touching_any_state(which):
    from dasac_hip import DasacError
    p = nn.Parameter(torch.ones(5))
    opt = makers()[which]([p], track_tensor_stats=True)
    opt.step()                                               # no gradient anywhere: nothing to do, nothing to refuse
    p.grad = torch.ones(5)
    for refused in (opt.step, opt.measure_tensor_stats, lambda: opt.tensor_stats, lambda: opt.last_skipped_stats):
        with pytest.raises(DasacError):
            refused()
    assert torch.equal(p.detach(), torch.ones(5)) and not opt.state.get(p) and torch.equal(p.grad, torch.ones(5))


def test_make_optimizer_passes_tensor_stats_and_implies_fused_all():
    import models
    import driver
    from dasac_hip.optim import FusedAdam, FusedSGD
    cfg = NS(**dict(DEFAULT_CFG, INIT_MODEL="", OPT_NESTEROV=False))
    net = models.get_model(cfg, 0, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    net.train()
    with_cfg = lambda **kw: NS(**dict(vars(cfg), **kw))
    for c, cls in [(cfg, FusedSGD), (with_cfg(OPT_NESTEROV=True), FusedSGD), (with_cfg(OPT="Adam", BETA1=0.5), FusedAdam)]:
        for fused in (True, "all"):                          # the default fused=True would give torch's class for two of them
            opt = driver.make_optimizer(net, c, fused=fused, tensor_stats=True)
            assert type(opt) is cls and opt.track_tensor_stats is True
            assert (opt.max_grad_norm, opt.skip_nonfinite, opt.track_grad_norm) == (None, False, False)
        opt = driver.make_optimizer(net, c, tensor_stats=True, skip_nonfinite=True, max_grad_norm=2.0)
        assert type(opt) is cls and opt.track_tensor_stats and opt.skip_nonfinite and opt.max_grad_norm == 2.0
        assert driver.make_optimizer(net, c, max_grad_norm=2.0).track_tensor_stats is False
        with pytest.raises(ValueError):
            driver.make_optimizer(net, c, fused=False, tensor_stats=True)
    with pytest.raises(ValueError):                          # no fused class for this one
        driver.make_optimizer(net, with_cfg(OPT="RMSprop"), fused="all", tensor_stats=True)
    # without the keyword the factory is what it was
    assert type(driver.make_optimizer(net, with_cfg(OPT="Adam"))) is torch.optim.Adam
    assert driver.make_optimizer(net, cfg).track_tensor_stats is False
    names = {p: n for n, p in net.named_parameters()}
    assert all(p in names for g in opt.param_groups for p in g["params"])      # every row of a report has a name


def test_bad_arguments_are_refused_on_the_host():
    """The entry point validates before it launches (no device needed for a refusal)."""
    from dasac_hip import lib as L
    lib = L.load()
    assert L.PROTOTYPES["dasac_tensor_stats_workspace"] == (ctypes.c_size_t, [ctypes.c_int])
    assert len(L.PROTOTYPES["dasac_tensor_stats"][1]) == 15
    assert lib.dasac_tensor_stats_workspace(0) == 0 and lib.dasac_tensor_stats_workspace(-3) == 0 and lib.dasac_tensor_stats_workspace(86) == 86 * 64
    buf = (ctypes.c_double * 16)()
    at = ctypes.addressof(buf)
    assert at % 16 == 0 or (at + 8) % 16 == 0
    at += at % 16
    call = lambda *a: lib.dasac_tensor_stats(*a, None)
    assert call(None, 48, 1, None, 1, None, 1, None, 0, None, None, None, None, None) != 0
    assert call(at, 40, 1, at, 1, at, 1, at, 64, at, None, None, None, None) != 0
    assert b"row_bytes" in lib.dasac_last_error()
    assert call(at, 64, 1, at, 2, at, 1, at, 127, at, None, None, None, None) != 0              # 2 chunks need 128 bytes
    assert b"workspace" in lib.dasac_last_error()
    assert call(at, 64, 1, at, 1, at, 1, at, 64, at + 4, None, None, None, None) != 0
    assert b"misaligned" in lib.dasac_last_error()
    assert call(at, 48, 1, at, 1, at, 0, at, 64, at, None, None, None, None) != 0
    for given in ((at, None, None, None), (at, at, at, None), (None, at, at, at), (None, None, None, at)):
        assert call(at, 48, 1, at, 1, at, 1, at, 64, at, *given) != 0
        assert b"all null or all given" in lib.dasac_last_error()
    assert call(at, 48, 1, at, 1, at, 1, at, 64, at, at + 8, at, at, at) != 0                   # the control block wants 16 bytes
    assert b"misaligned" in lib.dasac_last_error()
    assert not any(buf) and math.isfinite(sum(buf))
