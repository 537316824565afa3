"""The per-layer activation tables (dasac_activation_stats, `ops.ActivationStatsPlan`, `Engine.probe`, `driver.activation_probe` /
`activation_stats` / `activation_report` / `domain_gap_report`) against the numpy float64 restatement of the contract in
tests/activation_stats_ref.py.

Bounds.  On the lattice k * 2^-6, |k| <= 512, every double sum of the table is exact whatever its order: the whole table must be
== the reference.  On float data the counts, indices and maxima (columns 2-5) are still exact; a double sum of n terms carries at
most (n-1) * 2^-53 * sum|term| of rounding error whatever its order (Higham, Accuracy and Stability, 4.2), on the kernel's side
and on numpy's, so columns 0 and 1 must be within 2 * n * 2^-53 * sum|x| resp. 2 * n * 2^-53 * sum x^2 of the reference (the
squares themselves are exact in double)."""
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils._python_dispatch import TorchDispatchMode

import activation_stats_ref as ref
from oracle import nets_ref as NR
from oracle.step_ref import DEFAULT_CFG

pytestmark = pytest.mark.gpu
CRIT = nn.CrossEntropyLoss(ignore_index=255, reduction="none")
U = 2.0 ** -53
# (C, HW): every C and HW of the contract, every HW % 4 residue (0: 5120, 1: 1 and 97*97, 2: 2 and 1026, 3: 3, 63 and 1023), planes
# shorter than one thread's quad, planes of one partial sweep, and planes longer than a block's sweep of 4096 floats (97*97, 5120)
SHAPES = [(1, 97 * 97), (19, 1023), (64, 63), (257, 3), (19, 1), (64, 2), (1, 1026), (19, 5120), (257, 1)]
CASES = [(1, (0, 1)), (3, (0, 3)), (3, (0, 1, 3)), (5, (0, 5)), (5, (0, 1, 5)), (5, (0, 2, 3, 5))]


def lattice(N, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for c, hw in SHAPES:
        k = torch.randint(-512, 513, (N, c, hw), generator=g)
        k = k * (torch.rand(N, c, hw, generator=g) >= 1.0 / 3.0)
        out.append(k.to(torch.float32) / 64.0)
    return out


def floats(N, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for c, hw in SHAPES:
        scale = 10.0 ** (torch.rand(c, generator=g) * 6.0 - 3.0)                # per channel, 1e-3 .. 1e3
        x = torch.randn(N, c, hw, generator=g) * scale.view(1, c, 1)
        out.append(torch.where(torch.rand(N, c, hw, generator=g) < 0.05, torch.zeros(()), x).to(torch.float32))
    return out


def run(tensors, bounds):
    from dasac_hip import ops
    table, plan = ops.activation_stats([t.cuda() if not t.is_cuda else t for t in tensors], bounds)
    assert table.dtype == torch.float64 and tuple(table.shape) == (len(plan.bounds) - 1, plan.R, 6)
    return table


def assert_within_bound(table, tensors, bounds, what):
    """columns 2-5 exact, 0 and 1 within the summation bound of the module docstring; prints the worst ratio to the bound."""
    got = table.cpu().numpy()
    want, abs_sum, count = ref.table([t.cpu().numpy() for t in tensors], bounds)
    assert got.shape == want.shape
    assert np.array_equal(got[..., 2:], want[..., 2:]), what
    bound0, bound1 = 2.0 * count * U * abs_sum, 2.0 * count * U * want[..., 1]
    err0, err1 = np.abs(got[..., 0] - want[..., 0]), np.abs(got[..., 1] - want[..., 1])
    worst = max(float((err0 / np.maximum(bound0, 1e-300)).max()), float((err1 / np.maximum(bound1, 1e-300)).max()))
    print("{}: worst summation error / bound = {:.3e}".format(what, worst))
    assert (err0 <= bound0).all() and (err1 <= bound1).all(), (what, worst)


@pytest.mark.parametrize("N,bounds", CASES)
def test_lattice_tables_are_exact(N, bounds):
    tensors = lattice(N, 100 + N)
    got = run(tensors, bounds).cpu().numpy()
    want, _, _ = ref.table([t.numpy() for t in tensors], bounds)
    assert 0.25 < want[..., 5].sum() / sum(t.numel() for t in tensors) < 0.42       # about a third of the entries are zero
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


def test_float_tables_within_the_summation_bound():
    tensors = floats(5, 7)
    for bounds in [(0, 5), (0, 2, 3, 5)]:
        assert_within_bound(run(tensors, bounds), tensors, bounds, "float data, bounds {}".format(bounds))


def test_planted_nonfinite_entries_are_counted_located_and_left_out_of_the_sums():
    INF, NAN = float("inf"), float("nan")
    g = torch.Generator().manual_seed(11)
    mk = lambda *shape: (torch.randint(-512, 513, shape, generator=g) * (torch.rand(*shape, generator=g) >= 1.0 / 3.0)).to(torch.float32) / 64.0
    a, b = mk(3, 4, 97 * 97), mk(3, 2, 64)                   # a: planes at every 4-byte phase; b: aligned planes
    a[0, 0, 0] = INF                                         # the first element of a tensor
    b[2, 1, 63] = NAN                                        # the last element of a tensor
    a[1, 2, 97 * 97 - 1] = -INF                              # the last element of a misaligned plane (plane 6 starts at float 6 * 9409)
    b[0, 0, 5], b[2, 0, 7] = NAN, INF                        # one channel, two segments
    a[2, 3, 100], a[2, 3, 4100], a[1, 3, 9000] = NAN, INF, -INF      # one channel, one segment, three threads: the smallest index wins
    bounds = (0, 1, 3)
    got = run([a, b], bounds).cpu().numpy()
    want, _, _ = ref.table([a.numpy(), b.numpy()], bounds)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    HW = 97 * 97
    # and the planted values, spelled out (rows: a's channels 0-3, b's channels 4-5)
    assert got[0, 0, 3] == 1 and got[0, 0, 4] == 1 and got[1, 0, 3] == 0 and got[1, 0, 4] == 0
    assert got[1, 2, 3] == 1 and got[1, 2, 4] == 1 + (1 * 4 + 2) * HW + HW - 1 and got[0, 2, 3] == 0
    assert got[1, 3, 3] == 3 and got[1, 3, 4] == 1 + (1 * 4 + 3) * HW + 9000
    assert got[0, 4, 3] == 1 and got[0, 4, 4] == 1 + 5 and got[1, 4, 3] == 1 and got[1, 4, 4] == 1 + (2 * 2 + 0) * 64 + 7
    assert got[1, 5, 3] == 1 and got[1, 5, 4] == 3 * 2 * 64
    assert np.isfinite(got).all()


def test_tables_do_not_depend_on_where_the_tensors_lie():
    from dasac_hip import ops
    tensors = floats(3, 21)
    bounds = (0, 1, 3)
    fresh = [t.cuda() for t in tensors]
    base = run(fresh, bounds)
    assert torch.equal(base.view(torch.int64), run(fresh, bounds).view(torch.int64))      # two consecutive calls
    for off in range(4):
        carved, phases = [], set()
        for t in tensors:
            buf = torch.empty(t.numel() + 8, dtype=torch.float32, device="cuda")
            view = buf[off:off + t.numel()].view(t.shape)
            view.copy_(t)
            assert view.is_contiguous() and view.data_ptr() == buf.data_ptr() + 4 * off
            phases.add(view.data_ptr() % 16)
            carved.append(view)
        assert phases == {4 * off}
        table, _ = ops.activation_stats(carved, bounds)
        assert torch.equal(base.view(torch.int64), table.view(torch.int64)), off


def test_bad_arguments_are_refused_and_leave_the_table_alone():
    from dasac_hip import DasacError, ops
    from dasac_hip import lib as L
    lib = L.load()
    dev = torch.device("cuda")
    x = torch.arange(1.0, 13.0, device=dev).view(2, 3, 2)                       # N = 2, C = 3, HW = 2
    plan = ops.ActivationStatsPlan([(3, 2)], 2)
    rows = plan.rows.copy()
    rows["x"] = x.data_ptr()
    desc = torch.from_numpy(rows.view(np.int64)).to(dev)
    seg = torch.tensor([0, 2], dtype=torch.int32, device=dev)
    need = lib.dasac_activation_stats_workspace(6)
    assert need == 6 * 48
    ws = torch.zeros(need + 8, dtype=torch.uint8, device=dev)
    table = torch.full((1, 3, 6), 7.0, dtype=torch.float64, device=dev)
    good = dict(tensors=desc.data_ptr(), n_tensors=1, N=2, R=3, seg_bounds=seg.data_ptr(), n_segments=1, workspace=ws.data_ptr(),
                workspace_bytes=need, table=table.data_ptr())
    order = list(good)

    def call(**change):
        a = dict(good, **change)
        L.check(lib.dasac_activation_stats(*[a[k] for k in order], L.stream_ptr()), "dasac_activation_stats")
    bad = [dict(tensors=0), dict(seg_bounds=0), dict(workspace=0), dict(table=0), dict(n_tensors=0), dict(n_tensors=-1), dict(n_tensors=1 << 17),
           dict(N=0), dict(N=-2), dict(R=0), dict(n_segments=0), dict(n_segments=9), dict(n_segments=3), dict(workspace_bytes=need - 1),
           dict(workspace_bytes=0), dict(N=1 << 20, R=1 << 12), dict(table=table.data_ptr() + 4), dict(workspace=ws.data_ptr() + 4),
           dict(tensors=desc.data_ptr() + 4), dict(seg_bounds=seg.data_ptr() + 2)]
    for change in bad:
        with pytest.raises(DasacError):
            call(**change)
    torch.cuda.synchronize()
    assert bool((table == 7.0).all())
    call()
    expect = [[1 + 2 + 7 + 8, 1 + 4 + 49 + 64, 8, 0, 0, 0], [3 + 4 + 9 + 10, 9 + 16 + 81 + 100, 10, 0, 0, 0], [5 + 6 + 11 + 12, 25 + 36 + 121 + 144, 12, 0, 0, 0]]
    assert torch.equal(table.cpu(), torch.tensor([expect], dtype=torch.float64))
    table.fill_(7.0)
    call(workspace=ws.data_ptr() + 8)                        # 8-byte alignment is enough
    assert torch.equal(table.cpu(), torch.tensor([expect], dtype=torch.float64))
    # the Python layer vouches for what lives in device memory: bounds and shapes
    for wrong in [(0, 2, 1, 3), (0, 2), (0, 3, 3), (4,)]:
        with pytest.raises(DasacError):
            ops.activation_stats([torch.zeros(3, 2, 5, device=dev)], wrong)
    with pytest.raises(DasacError):
        plan.run([torch.zeros(2, 3, 3, device=dev)])          # not the plan's shape
    with pytest.raises(DasacError):
        plan.run([torch.zeros(2, 3, 2, device=dev, dtype=torch.float64)])
    with pytest.raises(DasacError):
        ops.activation_stats([torch.zeros(3, 2, 5, device=dev), torch.zeros(2, 2, 5, device=dev)])      # one N per call


# ---------------------------------------------------------------------------------------------- engine and driver
def rn101(seed=3):
    import models
    net = models.DeepLabV2_ResNet101(num_classes=19, criterion=CRIT, freeze_bn=True)
    net.load_state_dict(NR.resnet101_state(seed=seed, randomize_bn=True, he_init=True, residual_gain=0.25, aspp_gain=0.2), strict=True)
    return net.cuda().train()


def fcn8s():
    import models
    net = models.VGG16_FCN8s(19, criterion=CRIT, use_bn=True, freeze_bn=True, drop_rate=0.0)
    net.load_state_dict(NR.fcn8s_vgg16_state(seed=12, randomize_bn=True), strict=True)
    return net.cuda().train()


@pytest.mark.parametrize("which", ["rn101", "fcn8s"])
def test_engine_tables_agree_with_float64_reductions_over_the_saved_activations(which):
    import driver
    net, size = (rn101(), (65, 65)) if which == "rn101" else (fcn8s(), (64, 64))
    x = torch.randn(2, 3, *size, generator=torch.Generator().manual_seed(5)).cuda()
    rec = driver.activation_stats(net, x, bounds=(1,))
    assert rec.net == "backbone" and rec.N == 2 and rec.bounds == (0, 1, 2) and net._engine.probe is None
    eng = net._engine
    with torch.no_grad():
        _, saved = eng.forward(x, keep=True)
    names = [e["name"] for e in rec.layout]
    assert len(rec.layout) == len(eng.plan.ops) + 1 and len(set(names)) == len(names) and names[0] == "input"
    assert [e["slot"] for e in rec.layout] == [0] + [op.dst for op in eng.plan.ops] and [e["op"] for e in rec.layout] == list(range(-1, len(eng.plan.ops)))
    module_names = {n for n, _ in net.named_modules()}
    assert all(e["name"] in module_names for e in rec.layout if e["kind"] == "conv")
    acts = [saved["acts"][e["slot"]] for e in rec.layout]
    assert all(tuple(a.shape) == (2, e["C"], e["H"], e["W"]) for a, e in zip(acts, rec.layout))
    assert [e["row0"] for e in rec.layout] == list(np.cumsum([0] + [e["C"] for e in rec.layout[:-1]]))
    assert all(e["relu"] == bool(op.relu) for e, op in zip(rec.layout[1:], eng.plan.ops))
    assert_within_bound(rec.table, acts, rec.bounds, which)
    report = driver.activation_report(rec, segment=1)
    assert report["first_nonfinite_layer"] is None and len(report["layers"]) == len(rec.layout)
    relu_layers = [l for l, e in zip(report["layers"], rec.layout) if e["relu"]]
    assert relu_layers and all(l["zero_share"] > 0 for l in relu_layers)            # a ReLU leaves zeros
    assert driver.format_activation_report(report).count("\n") == 11


class Recorder(TorchDispatchMode):
    """Every ATen operator that touches more than SMALL elements and is not allocation / view / copy plumbing."""
    PLUMBING = {"empty", "empty_like", "empty_strided", "new_empty", "new_empty_strided", "zeros", "zeros_like", "ones", "full", "zero_", "fill_",
                "view", "_unsafe_view", "reshape", "as_strided", "narrow", "slice", "select", "expand", "permute", "transpose", "t", "squeeze",
                "unsqueeze", "flatten", "unflatten", "detach", "detach_", "alias", "clone", "contiguous", "copy_", "_to_copy", "to", "cat",
                "lift_fresh", "_local_scalar_dense", "item", "is_pinned", "_pin_memory", "pin_memory", "record_stream", "set_", "resize_",
                "scalar_tensor", "result_type", "_has_compatible_shallow_copy_type", "is_same_size", "equal", "unbind", "split", "chunk", "stack"}
    SMALL = 64

    def __init__(self):
        super().__init__()
        self.big = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = func.overloadpacket.__name__ if hasattr(func, "overloadpacket") else str(func)
        if name not in self.PLUMBING:
            sizes = [t.numel() for t in torch.utils._pytree.tree_leaves((args, kwargs, out)) if isinstance(t, torch.Tensor)]
            if sizes and max(sizes) > self.SMALL:
                self.big.append((name, max(sizes)))
        return out


def sac_net(seed=3):
    import models
    import driver
    cfg = NS(**dict(DEFAULT_CFG, INIT_MODEL="", OPT_NESTEROV=False))
    net = models.get_model(cfg, 0, num_classes=19, criterion=CRIT)
    net.backbone.load_state_dict(NR.resnet101_state(seed=seed, randomize_bn=True, he_init=True, residual_gain=0.25, aspp_gain=0.2), strict=True)
    net.cuda().train()
    return cfg, net, driver.make_optimizer(net, cfg)


@pytest.mark.parametrize("fuse", [False, True])
def test_probe_in_a_training_iteration_records_the_passes_and_changes_nothing(fuse):
    import driver
    src, tgt = driver.synthetic_batches(2, 1, 2, (33, 49), "cuda", seed=5)
    clone = lambda: (tgt[0], tgt[1].clone(), tgt[2], tgt[3], tgt[4])
    results = []
    for probed in (False, True):
        cfg, net, optim = sac_net()
        driver.sac_train_iteration(net, optim, src, clone(), 2, True, cfg.LR_TARGET, fuse_passes=fuse)      # first call: teacher init, caches
        if probed:
            with Recorder() as rec, driver.activation_probe(net, bounds=lambda N: (2,) if N == 4 else None) as probe:
                out = driver.sac_train_iteration(net, optim, src, clone(), 2, True, cfg.LR_TARGET, fuse_passes=fuse)
                torch.cuda.synchronize()
            assert not rec.big, sorted(set(rec.big))[:12]
            assert net.backbone._engine.probe is None and net.slow_net._engine.probe is None      # detached on exit
        else:
            out = driver.sac_train_iteration(net, optim, src, clone(), 2, True, cfg.LR_TARGET, fuse_passes=fuse)
        results.append((out, {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None},
                        {k: v.clone() for k, v in net.state_dict().items()}))
    seen = [(r.net, r.N, r.bounds) for r in probe.passes]
    if fuse:
        assert seen == [("slow_net", 2, (0, 2)), ("backbone", 4, (0, 2, 4))]
    else:
        assert seen == [("backbone", 2, (0, 2)), ("backbone", 2, (0, 2)), ("slow_net", 2, (0, 2))]
    for r in probe.passes:
        assert r.table.is_cuda and r.table.dtype == torch.float64 and tuple(r.table.shape) == (len(r.bounds) - 1, sum(e["C"] for e in r.layout), 6)
        assert float(r.table[..., 3].sum()) == 0 and float(r.table[..., 2].max()) > 0
    (plain, g0, s0), (with_probe, g1, s1) = results
    for a, b in zip(plain[:2], with_probe[:2]):               # source and target losses
        assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert all(torch.equal(plain[2][k], with_probe[2][k]) for k in ("logits_up", "logits", "teacher_labels"))
    assert set(g0) == set(g1) and len(g0) > 300 and all(torch.equal(g0[k], g1[k]) for k in g0)
    assert all(torch.equal(s0[k], s1[k]) for k in s0)         # and the step it fed
    if fuse:                                                  # the two domains of the one student pass
        gap = driver.domain_gap_report(probe.passes[-1])
        assert len(gap["layers"]) == len(probe.passes[-1].layout) and all(np.isfinite(l["gap"]) for l in gap["layers"])
        assert gap["layers"][0]["gap"] > 0                    # source and target crops differ
        assert driver.format_domain_gap_report(gap).count("\n") == 11


def test_off_means_off(monkeypatch):
    import driver
    from dasac_hip import lib as L

    def refuse(*args):
        raise AssertionError("dasac_activation_stats called without a probe")
    monkeypatch.setattr(L.load(), "dasac_activation_stats", refuse)
    net = rn101()
    g = torch.Generator().manual_seed(9)
    x, y = torch.randn(2, 3, 33, 49, generator=g).cuda(), torch.randint(0, 19, (2, 33, 49), generator=g).cuda()
    losses, _ = net(x, y)
    losses["loss_ce"].mean().backward()
    with torch.no_grad():
        net(x)
    torch.cuda.synchronize()
    assert net._engine.probe is None and net.model.conv1.weight.grad is not None
    with pytest.raises(AssertionError):                      # control: with a probe attached the patched entry point is reached
        with driver.activation_probe(net):
            net(x, y)
    assert net._engine.probe is None                          # detached on the way out of a failing block too


def test_domain_gap_end_to_end():
    import driver
    net = rn101()
    a = torch.randn(1, 3, 65, 65, generator=torch.Generator().manual_seed(13))
    # Identical segments.  Two passes over the same batch hold the same activations bit for bit (the run-to-run identity the
    # project documents): segment 0 of the two records, every layer, exactly 0.
    aa = torch.cat([a, a]).cuda()
    first, second = driver.activation_stats(net, aa, bounds=(1,)), driver.activation_stats(net, aa, bounds=(1,))
    assert torch.equal(first.table.view(torch.int64), second.table.view(torch.int64))
    same = driver.domain_gap_report(first, second)
    assert len(same["layers"]) == len(first.layout) > 100
    assert all(l["gap"] == 0.0 and l["gap_max"] == 0.0 and l["mean_shift"] == 0.0 for l in same["layers"])
    # The same image twice in ONE batch: the two samples of a layer are identical wherever the convolutions gave them the same
    # bits (a GEMM tile's split-K schedule depends on the tile's position, so sample 1's sums may run in another order than sample
    # 0's: measured 1.5e-8 at model.layer4.0.conv3) -- and there, the input included, the two segments' gap is exactly 0 although
    # the two samples' planes lie at different addresses.
    with torch.no_grad():
        _, saved = net._engine.forward(aa, keep=True)
    in_batch = driver.domain_gap_report(first)
    twins = [torch.equal(saved["acts"][e["slot"]][0], saved["acts"][e["slot"]][1]) for e in first.layout]
    worst = max(in_batch["layers"], key=lambda l: l["gap_max"])
    print("one batch, the image twice: {} of {} layers bit-identical; largest gap_max {:.3e} at {}".format(
        sum(twins), len(twins), worst["gap_max"], worst["name"]))
    assert twins[0]
    assert all(l["gap"] == 0.0 and l["gap_max"] == 0.0 and l["mean_shift"] == 0.0 for l, twin in zip(in_batch["layers"], twins) if twin)
    # the second segment's image scaled by 0.5: the input layer's numbers follow from the images alone
    rec = driver.activation_stats(net, torch.cat([a, 0.5 * a]).cuda(), bounds=(1,))
    layer = driver.domain_gap_report(rec)["layers"][0]
    xa, xb = a[0].double().reshape(3, -1).numpy(), (0.5 * a)[0].double().reshape(3, -1).numpy()
    mu_a, mu_b = xa.mean(axis=1), xb.mean(axis=1)
    var_a, var_b = (xa * xa).mean(axis=1) - mu_a ** 2, (xb * xb).mean(axis=1) - mu_b ** 2
    gaps = [ref.gap(mu_a[c], var_a[c], mu_b[c], var_b[c]) for c in range(3)]
    # Sums of n = 4225 terms on both sides: a mean is good to 2 * n * 2^-53 * mean|x| on the two sides together (module docstring), a
    # mean square likewise.  mean_shift is an RMS of differences of two means per channel, so it moves by at most twice the largest
    # error of a mean.  gap = num / den with num ~ 0.25 and den ~ 0.6 here (sigma_b = sigma_a / 2 ~ 0.5): moments of order 1 that are
    # good to ~1e-12, through a function whose relative condition number is of order 10 (sigma_a - sigma_b is half of sigma_a).
    n = xa.shape[1]
    tol_mu = 2.0 * n * U * max(np.abs(xa).mean(axis=1).max(), np.abs(xb).mean(axis=1).max())
    assert layer["name"] == "input" and layer["dead_both"] == 0
    assert abs(layer["mean_shift"] - np.sqrt(np.mean((mu_a - mu_b) ** 2))) <= 2.0 * tol_mu
    assert abs(layer["gap"] - np.mean(gaps)) <= 1e-10 * np.mean(gaps)
    assert abs(layer["gap_max"] - max(gaps)) <= 1e-10 * max(gaps) and layer["gap_max_channel"] == int(np.argmax(gaps))
