"""The class-conditional feature tables (dasac_label_nodes, dasac_class_feature_stats, `ops.label_nodes` / `class_feature_stats`,
`Engine.tap`, `driver.class_features`) against the numpy restatement of the contract in tests/class_features_ref.py.

Bounds.  dasac_label_nodes is integer work: equal to the reference.  On the lattice k * 2^-6, |k| <= 512, every double sum of the
table is exact whatever its order: sums and counts must be == the reference.  On float data the counts are still exact; a double
sum of n exact terms carries at most (n-1) * 2^-53 * sum|term| of rounding error whatever its order (Higham, Accuracy and
Stability, 4.2), on the kernel's side and on numpy's, so column 0 must be within 2 * n * 2^-53 * sum|x| and column 1 within
2 * n * 2^-53 * sum x^2 of the reference (the squares themselves are exact in double), n = the entries of the cell."""
import numpy as np
import pytest
import torch

import class_features_ref as ref
from exact_workspace import ExactWorkspace
from test_gpu_activation_stats import fcn8s, rn101, sac_net

pytestmark = pytest.mark.gpu
U = 2.0 ** -53

NODE_SHAPES = [((33, 49), (5, 7)),      # exact stride 8
               ((30, 52), (5, 8)),      # inexact stride
               ((65, 65), (9, 9)),
               ((17, 40), (1, 6)),      # h == 1
               ((40, 17), (6, 1)),      # w == 1
               ((9, 9), (9, 9))]        # unit scale
RADII = (0, 1, 2, 4, 8)
# (N, Cf, HW, C).  The last two are this kernel's own: a block takes G = min(8, N * Cf / 2048) channels, so they reach G = 2 and
# G = 8 with a channel count that is no multiple of the group.
SHAPES = [(1, 1, 1, 19),                # a single element
          (3, 5, 3, 19),                # plane shorter than a quad
          (2, 4, 1023, 19),             # HW % 4 == 3
          (2, 3, 1026, 7),              # HW % 4 == 2
          (2, 2, 9409, 19),             # 97^2, % 4 == 1, longer than one block sweep
          (1, 3, 5120, 32),             # C = 32: two passes of the generic kernel
          (1, 1, 4096, 2),              # C = 2
          (70, 2, 5, 19),               # many samples
          (3, 257, 64, 19),             # an odd channel count
          (3, 1367, 8, 19),             # two channels per block, the last block one
          (4, 4099, 4, 19)]             # eight channels per block, the last block three


# ---------------------------------------------------------------------------------------------- label_nodes
def label_maps(size, C, dtype, seed=0, N=3):
    lab = ref.blocks(N, size[0], size[1], C, seed)
    lab[N - 1, size[0] // 2, size[1] // 2] = 200                  # neither a class nor 255
    lab[0, 0, 0] = C                                              # the first label that is no class
    return lab.astype(np.uint8) if dtype == torch.uint8 else lab  # uint8: -1 becomes 255, no class either way


@pytest.mark.parametrize("C", [19, 2])
@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8])
@pytest.mark.parametrize("size,nodes_hw", NODE_SHAPES)
def test_label_nodes_equal_the_reference(size, nodes_hw, dtype, C):
    from dasac_hip import ops
    lab = label_maps(size, C, dtype)
    dev = torch.from_numpy(lab).cuda()
    for r in RADII:
        got = ops.label_nodes(dev, nodes_hw, C, r)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (3,) + nodes_hw
        want = ref.label_nodes(lab, nodes_hw[0], nodes_hw[1], C, r)
        assert np.array_equal(got.cpu().numpy(), want), (r, np.argwhere(got.cpu().numpy() != want)[:8])
        assert not np.isin(want, [200, C]).any() and set(np.unique(want)) <= set(range(C)) | {255}
        if C == 19 and r in (1, 2) and (size, nodes_hw) in NODE_SHAPES[:3]:      # the window bites, and not everywhere
            assert 0.05 <= ref.kept_share(want) <= 0.95, (size, r, ref.kept_share(want))
    if size == (9, 9):                                            # unit scale, radius 0: the map itself
        assert np.array_equal(ref.label_nodes(lab, 9, 9, C, 0), np.where((lab.astype(np.int64) >= 0) & (lab.astype(np.int64) < C), lab, 255).astype(np.uint8))


def test_label_nodes_refuses_bad_arguments():
    from dasac_hip import DasacError, ops
    from dasac_hip import lib as L
    lib = L.load()
    lab = torch.zeros(1, 8, 8, dtype=torch.int64, device="cuda")
    out = torch.full((1, 2, 2), 7, dtype=torch.uint8, device="cuda")
    for args in [(0, 0, 1, 8, 8, 2, 2, 19, 0, out.data_ptr()), (lab.data_ptr(), 0, 1, 8, 8, 2, 2, 19, 0, 0), (lab.data_ptr(), 0, 1, 8, 8, 2, 2, 19, 9, out.data_ptr()),
                 (lab.data_ptr(), 0, 1, 8, 8, 2, 2, 19, -1, out.data_ptr()), (lab.data_ptr(), 0, 1, 8, 8, 2, 2, 0, 0, out.data_ptr()),
                 (lab.data_ptr(), 0, 1, 8, 8, 2, 2, 256, 0, out.data_ptr()), (lab.data_ptr(), 0, 1, 8, 8, 0, 2, 19, 0, out.data_ptr()),
                 (lab.data_ptr() + 4, 0, 1, 4, 4, 2, 2, 19, 0, out.data_ptr())]:
        with pytest.raises(DasacError):
            L.check(lib.dasac_label_nodes(*args, L.stream_ptr()), "dasac_label_nodes")
    for bad in [lambda: ops.label_nodes(lab.to(torch.int32), (2, 2), 19), lambda: ops.label_nodes(lab[0], (2, 2), 19),
                lambda: ops.label_nodes(lab, (2, 2), 19, radius=9), lambda: ops.label_nodes(lab, (0, 2), 19)]:
        with pytest.raises(DasacError):
            bad()
    torch.cuda.synchronize()
    assert bool((out == 7).all())


# ---------------------------------------------------------------------------------------------- class_feature_stats
def make_nodes(N, HW, C, seed):
    """uint8 [N,HW]: 10 % are 255, class C - 1 is absent from every sample, and (N >= 2) the last sample holds class 0 alone."""
    rng = np.random.RandomState(seed)
    nodes = rng.randint(0, max(C - 1, 1), size=(N, HW)).astype(np.uint8)
    if N >= 2:
        nodes[N - 1] = 0
    nodes[rng.rand(N, HW) < 0.1] = 255
    return nodes


def lattice(N, Cf, HW, seed):
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-512, 513, (N, Cf, HW), generator=g)
    k = k * (torch.rand(N, Cf, HW, generator=g) >= 1.0 / 3.0)
    return k.to(torch.float32) / 64.0


def floats(N, Cf, HW, seed):
    g = torch.Generator().manual_seed(seed)
    scale = 10.0 ** (torch.rand(Cf, generator=g) * 6.0 - 3.0)                    # per channel, 1e-3 .. 1e3
    x = torch.randn(N, Cf, HW, generator=g) * scale.view(1, Cf, 1)
    return torch.where(torch.rand(N, Cf, HW, generator=g) < 0.05, torch.zeros(()), x).to(torch.float32)


def run(x, nodes, C, table=None):
    from dasac_hip import ops
    t = ops.class_feature_stats(x.cuda(), torch.as_tensor(nodes).cuda(), C, table)
    assert t.sums.dtype == torch.float64 and tuple(t.sums.shape) == (C, x.shape[1], 2) and t.counts.dtype == torch.int64 and tuple(t.counts.shape) == (C,)
    return t


def bits(table):
    return table.sums.view(torch.int64).clone(), table.counts.clone()


def same_bits(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def assert_within_bound(table, x, nodes, C, what):
    """counts exact, the two columns within the summation bound of the module docstring; prints the worst ratio to the bound."""
    sums, counts, abs_sum, entries = ref.table(x, nodes, C)
    got, got_counts = table.sums.cpu().numpy(), table.counts.cpu().numpy()
    assert np.array_equal(got_counts, counts), what
    n = entries[:, None].astype(np.float64)
    bound0, bound1 = 2.0 * n * U * abs_sum, 2.0 * n * U * sums[..., 1]
    err0, err1 = np.abs(got[..., 0] - sums[..., 0]), np.abs(got[..., 1] - sums[..., 1])
    worst = max(float((err0 / np.maximum(bound0, 1e-300)).max()), float((err1 / np.maximum(bound1, 1e-300)).max()))
    print("{}: worst summation error / bound = {:.3e}".format(what, worst))
    assert (err0 <= bound0).all() and (err1 <= bound1).all(), (what, worst)


@pytest.mark.parametrize("N,Cf,HW,C", SHAPES)
def test_lattice_tables_are_exact(N, Cf, HW, C):
    x, nodes = lattice(N, Cf, HW, 100 + HW), make_nodes(N, HW, C, 200 + HW)
    table = run(x, nodes, C)
    sums, counts, _, _ = ref.table(x.numpy(), nodes, C)
    got = table.sums.cpu().numpy()
    assert np.array_equal(table.counts.cpu().numpy(), counts)
    assert np.array_equal(got, sums), np.argwhere(got != sums)[:8]
    assert counts[C - 1] == 0 and (got[C - 1] == 0).all()        # the absent class: exactly 0
    if N * HW >= 200:
        assert counts.sum() > 0 and 0.02 < (nodes == 255).mean() < 0.3


@pytest.mark.parametrize("N,Cf,HW,C", SHAPES)
def test_float_tables_within_the_summation_bound(N, Cf, HW, C):
    x, nodes = floats(N, Cf, HW, 300 + HW), make_nodes(N, HW, C, 400 + HW)
    assert_within_bound(run(x, nodes, C), x.numpy(), nodes, C, "float data {}".format((N, Cf, HW, C)))


def test_two_half_batches_accumulate_to_the_whole_batch():
    for N, Cf, HW, C in [(4, 4, 1023, 19), (6, 3, 130, 7)]:
        x, nodes = lattice(N, Cf, HW, 17), make_nodes(N, HW, C, 18)
        whole = run(x, nodes, C)
        halves = run(x[:N // 2], nodes[:N // 2], C)
        assert run(x[N // 2:], nodes[N // 2:], C, halves) is halves
        assert same_bits(bits(whole), bits(halves))
        assert int(whole.counts.sum()) == int((nodes < C).sum())


def test_tables_do_not_depend_on_where_x_and_nodes_lie():
    from dasac_hip import ops
    N, Cf, HW, C = 2, 4, 1023, 19
    x, nodes = floats(N, Cf, HW, 21), torch.from_numpy(make_nodes(N, HW, C, 22))
    xd, nd = x.cuda(), nodes.cuda()
    base = bits(ops.class_feature_stats(xd, nd, C))
    assert same_bits(base, bits(ops.class_feature_stats(xd, nd, C)))             # two consecutive calls
    for xo in range(4):
        xbuf = torch.empty(x.numel() + 8, dtype=torch.float32, device="cuda")
        xv = xbuf[xo:xo + x.numel()].view(x.shape)
        xv.copy_(x)
        assert xv.is_contiguous() and xv.data_ptr() % 16 == (xbuf.data_ptr() + 4 * xo) % 16
        for no in range(4):
            nbuf = torch.full((nodes.numel() + 8,), 3, dtype=torch.uint8, device="cuda")      # a class around the view: a stray read would count
            nv = nbuf[no:no + nodes.numel()].view(nodes.shape)
            nv.copy_(nodes)
            assert nv.data_ptr() % 4 == (nbuf.data_ptr() + no) % 4
            assert same_bits(base, bits(ops.class_feature_stats(xv, nv, C))), (xo, no)


def test_bad_arguments_are_refused_and_leave_the_table_alone():
    from dasac_hip import DasacError, ops
    from dasac_hip import lib as L
    lib = L.load()
    dev = torch.device("cuda")
    N, Cf, HW, C = 2, 3, 5, 19
    x = torch.arange(1.0, 1.0 + N * Cf * HW, device=dev).view(N, Cf, HW)
    nodes = torch.tensor([[0, 1, 255, 1, 0], [2, 2, 0, 19, 1]], dtype=torch.uint8, device=dev)
    need = lib.dasac_class_feature_stats_workspace(N, Cf, C)
    assert need == N * Cf * C * 16
    ws = torch.zeros(need + 8, dtype=torch.uint8, device=dev)
    sums = torch.full((C, Cf, 2), 7.0, dtype=torch.float64, device=dev)
    counts = torch.full((C,), 7, dtype=torch.int64, device=dev)
    good = dict(x=x.data_ptr(), nodes=nodes.data_ptr(), N=N, Cf=Cf, HW=HW, C=C, sums=sums.data_ptr(), counts=counts.data_ptr(),
                workspace=ws.data_ptr(), ws_bytes=need)
    order = list(good)

    def call(**change):
        a = dict(good, **change)
        L.check(lib.dasac_class_feature_stats(*[a[k] for k in order], L.stream_ptr()), "dasac_class_feature_stats")
    bad = [dict(C=33), dict(C=0), dict(C=-1), dict(x=0), dict(nodes=0), dict(sums=0), dict(counts=0), dict(workspace=0), dict(ws_bytes=need - 1),
           dict(ws_bytes=0), dict(N=0), dict(N=65536), dict(Cf=0), dict(HW=0), dict(HW=1 << 30), dict(x=x.data_ptr() + 2), dict(sums=sums.data_ptr() + 4),
           dict(workspace=ws.data_ptr() + 4)]
    for change in bad:
        with pytest.raises(DasacError):
            call(**change)
    # the Python layer vouches for what lives in device memory: dtypes and shapes
    table = ops.ClassFeatureTable(sums, counts)
    for wrong in [lambda: ops.class_feature_stats(x.double(), nodes, C, table),                            # an fp64 x
                  lambda: ops.class_feature_stats(x, nodes[:1], C, table),                                 # nodes of another N
                  lambda: ops.class_feature_stats(x, nodes[:, :4], C, table),                              # ... of another HW
                  lambda: ops.class_feature_stats(x, nodes.to(torch.int64), C, table),
                  lambda: ops.class_feature_stats(x[:, :2], nodes, C, table),                              # a table of another Cf
                  lambda: ops.class_feature_stats(x, nodes, 7, table),                                     # ... of another C
                  lambda: ops.class_feature_stats(x, nodes, 33), lambda: ops.class_feature_stats(x, nodes, 0),
                  lambda: ops.class_feature_stats(x, nodes, C, (sums, counts))]:
        with pytest.raises(DasacError):
            wrong()
    with pytest.raises(DasacError):
        ops.ClassFeatureTable(sums.float(), counts)
    with pytest.raises(DasacError):
        ops.ClassFeatureTable(sums, counts[:5])
    torch.cuda.synchronize()
    assert bool((sums == 7.0).all()) and bool((counts == 7).all())
    call(workspace=ws.data_ptr() + 8)                            # 8-byte alignment is enough
    xs, ns = x.cpu().numpy(), nodes.cpu().numpy()
    want, want_counts, _, _ = ref.table(xs, ns, C)
    assert np.array_equal(sums.cpu().numpy(), want + 7.0) and np.array_equal(counts.cpu().numpy(), want_counts + 7)      # small integers: exact
    assert want_counts.tolist()[:3] == [3, 3, 2] and want_counts[3:].sum() == 0                            # 255 and 19 are no class


def test_on_exactly_the_workspace_it_asks_for(monkeypatch):
    from dasac_hip import lib as L
    cases = [(2, 4, 1023, 19), (70, 2, 5, 19)]
    data = [(floats(N, Cf, HW, 31), make_nodes(N, HW, C, 32), C) for N, Cf, HW, C in cases]
    real = [bits(run(x, nodes, C)) for x, nodes, C in data]
    exact = ExactWorkspace()
    monkeypatch.setattr(L, "workspace", exact)
    got = [bits(run(x, nodes, C)) for x, nodes, C in data]
    assert exact.check() == len(cases)
    assert [r[0] for r in exact.requests] == [N * Cf * C * 16 for N, Cf, HW, C in cases]
    assert all(same_bits(a, b) for a, b in zip(real, got))


# ---------------------------------------------------------------------------------------------- engine and driver
@pytest.fixture(scope="module")
def rn():
    return rn101()


def inputs(size, seed=5, N=2):
    x = torch.randn(N, 3, *size, generator=torch.Generator().manual_seed(seed)).cuda()
    lab = ref.blocks(N, size[0], size[1], 19, seed)
    return x, lab


def check_layer(net, size, layer, radius, Cf=None):
    import driver
    x, lab = inputs(size)
    rec = driver.class_features(net, [(x, torch.from_numpy(lab).cuda())], layer=layer, radius=radius)
    eng = net._engine
    index, name = eng.tap_index(layer, {m: n for n, m in net.named_modules()})
    assert eng.tap is None and rec.layer == name and rec.batches == 1 and rec.radius == radius and rec.labels == "given" and rec.net == "backbone"
    assert net.training                                           # the mode it came in
    with torch.no_grad():
        _, saved = eng.forward(x, keep=True)
    feat = saved["acts"][0 if index < 0 else eng.plan.ops[index].dst]
    assert rec.Cf == feat.shape[1] == rec.table.Cf and (Cf is None or rec.Cf == Cf)
    nodes = ref.label_nodes(lab, feat.shape[2], feat.shape[3], 19, radius)
    assert ref.kept_share(nodes) > 0
    assert_within_bound(rec.table, feat.cpu().numpy(), nodes, 19, "{} at {}".format(type(net).__name__, name))
    return rec, feat


def test_driver_tables_of_the_classifier_input(rn):
    rec, feat = check_layer(rn, (65, 65), None, 1, Cf=2048)
    assert tuple(feat.shape) == (2, 2048, 9, 9) and rec.layer.startswith("model.layer4.2")


def test_driver_tables_of_an_interior_layer_and_of_the_input(rn):
    rec, feat = check_layer(rn, (65, 65), "input", 0, Cf=3)
    assert tuple(feat.shape) == (2, 3, 65, 65)
    layout = rn._engine.activation_layout([(0, 0, 0)] * (len(rn._engine.plan.ops) + 1), {m: n for n, m in rn.named_modules()})
    interior = [e["name"] for e in layout if e["kind"] == "conv" and e["name"].startswith("model.layer2.")][3]
    rec, feat = check_layer(rn, (65, 65), interior, 1)
    assert rec.layer == interior and feat.shape[1] < 2048
    import driver
    x, lab = inputs((65, 65))
    with pytest.raises(ValueError) as err:
        driver.class_features(rn, [(x, torch.from_numpy(lab).cuda())], layer="no.such.layer")
    assert "model.conv1" in str(err.value) and interior in str(err.value) and rn._engine.tap is None


def test_driver_tables_of_fcn8s():
    rec, feat = check_layer(fcn8s(), (64, 64), None, 1, Cf=4096)
    assert tuple(feat.shape[2:]) == (2, 2)


def test_prediction_labels_are_the_inferred_label_map(rn):
    import driver
    x, _ = inputs((65, 65), seed=6)
    maps, _ = driver.infer_label_maps(rn, x)
    for radius in (0, 1):
        pred = driver.class_features(rn, [(x, None)], labels="prediction", radius=radius)
        given = driver.class_features(rn, [(x, maps)], labels="given", radius=radius)
        assert pred.labels == "prediction" and same_bits(bits(pred.table), bits(given.table))
        kept = int((ref.label_nodes(maps.cpu().numpy(), 9, 9, 19, radius) != 255).sum())
        print("radius {}: {} of {} nodes keep their predicted class".format(radius, kept, 2 * 81))
        assert int(pred.table.counts.sum()) == kept
    with pytest.raises(ValueError):
        driver.class_features(rn, [(x, None)], labels="given")
    with pytest.raises(ValueError):
        driver.class_features(rn, [(x, maps)], labels="teacher")


def test_into_continues_a_record(rn):
    import driver
    (x1, l1), (x2, l2) = [(lattice(2, 3, 65 * 65, s).view(2, 3, 65, 65).cuda(), torch.from_numpy(ref.blocks(2, 65, 65, 19, s)).cuda()) for s in (1, 2)]
    one = driver.class_features(rn, [(x1, l1)], layer="input", radius=0)
    assert driver.class_features(rn, [(x2, l2)], layer="input", radius=0, into=one) is one and one.batches == 2
    both = driver.class_features(rn, [(x1, l1), (x2, l2)], layer="input", radius=0)
    assert both.batches == 2 and same_bits(bits(one.table), bits(both.table)) and int(both.table.counts.sum()) > 0
    before = bits(one.table)
    for change in [dict(radius=1), dict(layer=None), dict(num_classes=7), dict(labels="prediction")]:
        with pytest.raises(ValueError):
            driver.class_features(rn, [(x1, l1)], **dict(dict(layer="input", radius=0, into=one), **change))
    assert same_bits(before, bits(one.table)) and one.batches == 2 and rn._engine.tap is None
    assert driver.reduce_class_features(one) is one and same_bits(before, bits(one.table))      # no process group: nothing happens
    report = driver.class_gap_report(one, both, min_nodes=1)
    present = [c for c in range(19) if c not in report["skipped"]]
    assert present and all(report["gap"][c] == 0 for c in present)


def test_off_means_off(rn, monkeypatch):
    import driver
    from dasac_hip import DasacError
    from dasac_hip import lib as L
    x, lab = inputs((65, 65), seed=8)
    lab = torch.from_numpy(lab).cuda()
    with torch.no_grad():
        before = rn(x)[0].clone()
    driver.class_features(rn, [(x, lab)], radius=1)
    assert rn._engine.tap is None
    with torch.no_grad():
        after = rn(x)[0]
    assert torch.equal(before, after)
    seen = []
    rn._engine.tap = (len(rn._engine.plan.ops) - 1, seen.append)                 # a tapped pass gives the same logits, and the tap sees them
    try:
        with torch.no_grad():
            tapped = rn(x)[0]
    finally:
        rn._engine.tap = None
    assert torch.equal(before, tapped) and len(seen) == 1 and torch.equal(seen[0], before)
    with pytest.raises(DasacError):                              # a failure inside the tapped forward: a host tensor
        driver.class_features(rn, [(x, lab), (x.cpu(), lab)], radius=1)
    assert rn._engine.tap is None and rn.training

    calls = []
    lib = L.load()
    for name in ("dasac_label_nodes", "dasac_class_feature_stats", "dasac_class_feature_stats_workspace"):
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _f=real: (calls.append(_n), _f(*a))[1])
    cfg, net, optim = sac_net()
    src, tgt = driver.synthetic_batches(2, 1, 2, (33, 49), "cuda", seed=5)
    driver.sac_train_iteration(net, optim, src, tgt, 2, True, cfg.LR_TARGET)
    torch.cuda.synchronize()
    assert calls == [] and net.backbone._engine.tap is None and net.slow_net._engine.tap is None
    rec = driver.class_features(net, [(src[0], src[1])], radius=0, teacher=True)  # control: the patched entries are reached
    assert rec.net == "slow_net" and sorted(set(calls)) == ["dasac_class_feature_stats", "dasac_class_feature_stats_workspace", "dasac_label_nodes"]
    assert net.slow_net._engine.tap is None and net.backbone._engine.tap is None
