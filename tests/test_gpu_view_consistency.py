"""`dasac_view_consistency` on the GPU against the numpy reference of tests/consistency_ref.py, which sums in the kernel's own
prescribed order, and `driver.validation(consistency=True)` end to end.

Bounds: none.  Every table is integers and every float32 sum behind them has a fixed order, so the tables are compared with
torch.equal.  The synthetic inputs sit on an exactly summable lattice besides (consistency_ref.lattice: multiples of 2^-12, coverage
0, 1/4, 3/4 or 1 -- no view sum on the cover boundary); the end-to-end test runs on real soft-max outputs."""
import numpy as np
import pytest
import torch

from consistency_ref import lattice, view_consistency_ref
from test_gpu_validation import EINVAL, LAYERS, Recorder, _build, _loader, g19  # noqa: F401  (g19: fixture)

pytestmark = pytest.mark.gpu

# (N, T, C, H, W): HW < 4 and no pair; an odd HW with a 3-pixel tail; the compiled C = 19, T = 4 path; the runtime C / T path;
# both maxima; several blocks per group; the compiled T = 2 path with a 1-pixel tail
SHAPES = [(1, 1, 19, 1, 3), (1, 2, 19, 5, 7), (2, 4, 19, 33, 35), (1, 3, 5, 9, 11), (1, 8, 32, 6, 10), (3, 4, 19, 97, 131),
          (2, 2, 19, 15, 27)]


def _place(t, offset):
    """`t` on the device, starting `offset` ELEMENTS into its allocation (offset > 0: the planes sit at odd 4-byte phases)."""
    flat = torch.empty(t.numel() + offset, dtype=t.dtype, device="cuda")
    view = flat[offset:].view(t.shape)
    view.copy_(t)
    return view


def _check(tables, a, T, cover=0.5, times=1, base=None):
    """The three tables equal `times` x the reference (+ `base`), and the identities that tie them together."""
    agree, flips, per_view = (torch.from_numpy(x) for x in view_consistency_ref(a, T, cover))
    got = [t.cpu() for t in tables]
    want = [w * times + (b if base is not None else 0) for w, b in zip((agree, flips, per_view), base or (0, 0, 0))]
    for name, g, w in zip(("agree", "flips", "per_view"), got, want):
        assert g.dtype == torch.int64 and torch.equal(g, w), (name, int((g != w).sum()))
    if base is None:
        N, HW = a.shape[0] // T, a.shape[2] * a.shape[3]
        ks = torch.arange(T + 1)
        assert int(got[0].sum()) == times * N * HW
        assert int(got[2][:, 0].sum()) == int((got[0].sum(2) * ks[None, :]).sum())              # sum_t covered = sum k * agree
        assert int(got[2][:, 1].sum()) == int((got[0] * ks[None, None, :]).sum())               # sum_t hits = sum m * agree
        assert int(got[1].sum()) == int((got[0].sum(2) * (ks * (ks - 1) // 2)[None, :]).sum())  # pairs = sum k(k-1)/2 * agree
    return agree, flips, per_view


# ---------------------------------------------------------------------------------------------------------------------
# edge shapes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("N,T,C,H,W", SHAPES)
def test_view_consistency_edge_shapes_match_the_reference(N, T, C, H, W, offset):
    from dasac_hip import ops
    rng = np.random.default_rng(1000 * H + W + T)
    labels = rng.integers(0, C, (N, 1, H, W)).repeat(T, 1)
    flip = rng.random((N, T, H, W)) < 0.3
    labels = np.where(flip, rng.integers(0, C, (N, T, H, W)), labels)                  # most views agree, some do not
    for a in (lattice(rng, N, T, C, H, W), lattice(rng, N, T, C, H, W, labels=labels)):
        x = _place(torch.from_numpy(a), offset)
        assert x.data_ptr() % 16 == (4 * offset) % 16
        _check(ops.view_consistency(x, T), a, T)


# ---------------------------------------------------------------------------------------------------------------------
# several trips of a thread's quad loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,C", [(4, 19), (2, 19), (3, 5)])
def test_view_consistency_several_quads_per_thread(T, C):
    """The launch gives a thread more than one quad only once the grid holds two blocks per CU -- 512 groups here, as 64 copies of
    8 (the reference counts the 8 and is multiplied).  H * W = 2397 is 600 quads per group: two blocks, the first runs two full
    trips of its quad loop with the per-view counts carried across them, the second one trip that ends at quad 88 of its 512 with
    a one-pixel tail.  What a full-size target step launches (two trips at 769 x 769 and at 512 x 1024)."""
    from dasac_hip import ops
    N, copies, H, W = 8, 64, 51, 47
    rng = np.random.default_rng(17 + T)
    labels = rng.integers(0, C, (N, 1, H // 3, 1)).repeat(3, 2).repeat(W, 3).repeat(T, 1)       # bands: merged keys across trips
    labels = np.where(rng.random((N, T, H, W)) < 0.2, rng.integers(0, C, (N, T, H, W)), labels)
    a = lattice(rng, N, T, C, H, W, labels=labels)
    x = torch.from_numpy(a).cuda().repeat(copies, 1, 1, 1)
    assert x.shape[0] == 512 * T
    tables = ops.view_consistency(x, T)
    _check(tables, a, T, times=copies)
    prefix = ops.view_consistency(x[: 3 * N * T], T)                                   # 24 groups: one quad per thread, the same counts
    assert all(torch.equal(p * copies, t * 3) for p, t in zip(prefix, tables))


# ---------------------------------------------------------------------------------------------------------------------
# merged keys: uniform and blocky maps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "blocky"])
@pytest.mark.parametrize("shifted", [False, True])
def test_view_consistency_uniform_and_blocky_maps(kind, shifted):
    from dasac_hip import ops
    N, T, C, H, W = 2, 4, 19, 48, 80
    rng = np.random.default_rng(5)
    if kind == "uniform":
        base = np.full((N, 1, H, W), 7)
    else:
        base = rng.integers(0, C, (N, 1, H // 16, W // 16)).repeat(16, 2).repeat(16, 3)
    labels = base.repeat(T, 1)
    if shifted:
        labels[:, 2] = (labels[:, 2] + 1) % C                                          # one view slot is the outlier everywhere
    coverage = np.full((N, T, H, W), 4)
    coverage[:, 3, :, : W // 2] = 0                                                    # the last view reaches the right half only
    coverage[:, 0, : H // 3] = 1                                                       # a rim weight on top of the first
    a = lattice(rng, N, T, C, H, W, labels=labels, coverage=coverage)
    agree, flips, per_view = _check(ops.view_consistency(torch.from_numpy(a).cuda(), T), a, T)
    if kind == "uniform" and not shifted:
        assert int(agree[7].sum()) == N * H * W and int(flips.sum()) == int(flips[7, 7]) > 0
        assert torch.equal(per_view[:, 0], per_view[:, 1])
    if shifted:
        # the outlier meets the consensus only where the other views' weights are small enough for its own class to win the sum
        assert int(per_view[2, 1]) * 10 < int(per_view[1, 1]) and int(torch.diagonal(flips).sum()) < int(flips.sum())


# ---------------------------------------------------------------------------------------------------------------------
# ties
# ---------------------------------------------------------------------------------------------------------------------
def test_view_consistency_ties_take_the_first_maximum():
    from dasac_hip import ops
    T, C = 2, 5
    pixels = [  # (view 0, view 1) -> (a_0, a_1, c*)
        ([.25, .25, .25, .25, 0], [.25, .25, .25, .25, 0], (0, 0, 0)),                 # equal maxima inside both views
        ([0, .5, .5, 0, 0], [0, 0, .5, .5, 0], (1, 2, 2)),                             # a tie that starts later than class 0
        ([.5, .25, .25, 0, 0], [.25, .5, .25, 0, 0], (0, 1, 0)),                       # equal consensus sums .75, .75: class 0
        ([0, 0, .25, .75, 0], [0, 0, .75, .25, 0], (3, 2, 2)),                         # equal consensus sums 1, 1 at classes 2, 3
        ([0, 0, 0, 0, 1], [0, 0, 0, 0, 1], (4, 4, 4)),
    ]
    for C_run in (C, 19):                                                              # the runtime path and the compiled one
        a = np.zeros((T, C_run, 1, len(pixels)), np.float32)
        want_agree, want_flips = np.zeros((C_run + 1, 3, 3), np.int64), np.zeros((C_run, C_run), np.int64)
        for p, (v0, v1, (a0, a1, cs)) in enumerate(pixels):
            a[0, :C, 0, p], a[1, :C, 0, p] = v0, v1
            want_agree[cs, 2, int(a0 == cs) + int(a1 == cs)] += 1
            want_flips[a0, a1] += 1
        agree, flips, per_view = _check(ops.view_consistency(torch.from_numpy(a).cuda(), T), a, T)
        assert np.array_equal(agree.numpy(), want_agree) and np.array_equal(flips.numpy(), want_flips)
        assert per_view.tolist() == [[5, 3], [5, 4]]


# ---------------------------------------------------------------------------------------------------------------------
# coverage
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,C", [(4, 19), (3, 7)])
def test_view_consistency_coverage_and_the_cover_threshold(T, C):
    from dasac_hip import ops
    N, H, W = 1, 12, 21
    rng = np.random.default_rng(11)
    coverage = np.full((N, T, H, W), 4)
    coverage[:, :, 0, :5] = 0                                                          # pixels no view covers
    coverage[:, 0, 3:6], coverage[:, 2, 4:9] = 1, 3                                    # 0.25 and 0.75 around cover = 0.5
    coverage[:, :, 10, 10:] = 1                                                        # every view on its rim: uncovered at 0.5
    coverage[:, 1] = 0                                                                 # a view that is zero everywhere
    labels = rng.integers(0, C, (N, 1, H, W)).repeat(T, 1)
    labels[:, 2, :, ::3] = (labels[:, 2, :, ::3] + 2) % C
    a = lattice(rng, N, T, C, H, W, labels=labels, coverage=coverage)
    x = torch.from_numpy(a).cuda()
    half = _check(ops.view_consistency(x, T), a, T)
    assert int(half[0][C, 0, 0]) == 5 + (W - 10) and half[2][1].tolist() == [0, 0]
    assert int(half[2][0, 0]) == H * W - 5 - 3 * W - (W - 10)
    fifth = _check(ops.view_consistency(x, T, cover=0.2), a, T, cover=0.2)
    assert int(fifth[0][C, 0, 0]) == 5 and int(fifth[2][0, 0]) == H * W - 5 and fifth[2][1].tolist() == [0, 0]
    assert not torch.equal(half[0], fifth[0]) and not torch.equal(half[1], fifth[1])
    everything = _check(ops.view_consistency(x, T, cover=0.0), a, T, cover=0.0)           # z >= 0: even the empty view counts
    assert int(everything[0][C].sum()) == 0 and everything[2][:, 0].tolist() == [H * W] * T


# ---------------------------------------------------------------------------------------------------------------------
# accumulation
# ---------------------------------------------------------------------------------------------------------------------
def test_view_consistency_accumulates():
    from dasac_hip import ops
    N, T, C, H, W = 2, 4, 19, 17, 23
    rng = np.random.default_rng(3)
    a = lattice(rng, N, T, C, H, W)
    x = torch.from_numpy(a).cuda()
    tables = ops.view_consistency(x, T)
    assert ops.view_consistency(x, T, tables) is tables
    _check(tables, a, T, times=2)
    flat = ops.view_consistency(x, T, tables.buffer)                                   # the flat buffer is accepted as well
    assert flat.buffer.data_ptr() == tables.buffer.data_ptr()
    _check(tables, a, T, times=3)
    filled = ops.consistency_tables(C, T, "cuda")
    filled.buffer.copy_(torch.arange(filled.buffer.numel()) * 1000003 + (1 << 40))     # past 32 bits: the adds are 64-bit
    base = [t.cpu().clone() for t in filled]
    _check(ops.view_consistency(x, T, filled), a, T, base=base)


# ---------------------------------------------------------------------------------------------------------------------
# largest tables
# ---------------------------------------------------------------------------------------------------------------------
def test_view_consistency_largest_tables_reach_every_bin():
    """T = 8, C = 32.  One pixel per reachable bin [c][k][m] (k = 1..8, m = 0..k) and one that nothing covers: views 0..k-1 are
    covered; m of them put everything on c; the others put 410/1024 on a class of their own, 400/1024 on c and the rest on a
    second class of their own; views k..7 lie on their rim (coverage 1/4) with everything on c.  The summed views then peak at c
    by construction, whatever the covered views say."""
    from dasac_hip import ops
    T, C = 8, 32
    bins = [(c, k, m) for c in range(C) for k in range(1, T + 1) for m in range(k + 1)]
    a = np.zeros((T, C, 1, len(bins) + 1), np.float32)
    for p, (c, k, m) in enumerate(bins):
        others = [d for d in range(C) if d != c]
        for t in range(T):
            if t < m:
                a[t, c, 0, p] = 1.0
            elif t < k:
                a[t, others[2 * t], 0, p], a[t, c, 0, p], a[t, others[2 * t + 1], 0, p] = 410 / 1024, 400 / 1024, 214 / 1024
            else:
                a[t, c, 0, p] = 0.25
    a[:, 5, 0, -1] = 0.25                                                              # the last pixel: rims only
    agree, flips, per_view = _check(ops.view_consistency(torch.from_numpy(a).cuda(), T), a, T)
    reachable = torch.zeros(C + 1, T + 1, T + 1, dtype=torch.bool)
    for c, k, m in bins:
        reachable[c, k, m] = True
    reachable[C, 0, 0] = True
    assert torch.equal(agree, reachable.to(torch.int64))                               # every reachable bin exactly once, no other
    assert int(flips.sum()) == C * sum(k * (k - 1) // 2 * (k + 1) for k in range(1, T + 1))


# ---------------------------------------------------------------------------------------------------------------------
# bad arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_view_consistency_refuses_bad_arguments():
    from dasac_hip import lib as L, ops, DasacError
    lib = L.load()
    x = torch.rand(8, 33, 2, 4, device="cuda")
    tables = ops.consistency_tables(33, 9, "cuda")                                     # roomy enough for every call below

    def call(a=x.data_ptr(), N=1, T=4, C=19, HW=8, cover=0.5, agree=tables.agree.data_ptr(), flips=tables.flips.data_ptr(),
             per_view=tables.per_view.data_ptr()):
        return lib.dasac_view_consistency(a, N, T, C, HW, cover, agree, flips, per_view, L.stream_ptr())
    assert call(T=0) == EINVAL and call(T=9) == EINVAL and call(T=-1) == EINVAL
    assert b"view_consistency" in lib.dasac_last_error()
    assert call(C=0) == EINVAL and call(C=33) == EINVAL
    assert call(N=0) == EINVAL and call(HW=0) == EINVAL and call(HW=-8) == EINVAL and call(HW=1 << 30) == EINVAL
    assert call(a=0) == EINVAL and call(agree=0) == EINVAL and call(flips=0) == EINVAL and call(per_view=0) == EINVAL
    assert call(a=x.data_ptr() + 2) == EINVAL                                          # fp32 at a 2-byte phase
    assert call(agree=tables.agree.data_ptr() + 4) == EINVAL and call(flips=tables.flips.data_ptr() + 4) == EINVAL and \
        call(per_view=tables.per_view.data_ptr() + 4) == EINVAL
    torch.cuda.synchronize()
    assert int(tables.buffer.abs().sum()) == 0                                         # nothing was launched
    assert call() == 0 and call(T=8, C=32) == 0 and call(T=1, C=1) == 0
    torch.cuda.synchronize()
    assert int(tables.buffer.sum()) > 0
    y = x[:, :19].contiguous()
    with pytest.raises(DasacError):
        ops.view_consistency(y, 0)
    with pytest.raises(DasacError):
        ops.view_consistency(y, 9)
    with pytest.raises(DasacError):
        ops.view_consistency(x, 4)                                                     # 33 classes
    with pytest.raises(DasacError):
        ops.view_consistency(y, 3)                                                     # 8 views are no whole groups of 3
    with pytest.raises(DasacError):
        ops.view_consistency(y.double(), 4)
    with pytest.raises(DasacError):
        ops.view_consistency(y[0], 1)                                                  # wrong rank
    with pytest.raises(DasacError):
        ops.view_consistency(y.cpu(), 4)                                               # no CPU path
    with pytest.raises(DasacError):
        ops.view_consistency(y, 4, ops.consistency_tables(19, 2, "cuda"))              # tables of another T
    with pytest.raises(DasacError):
        ops.view_consistency(y, 4, torch.zeros(ops.consistency_size(19, 4) + 1, dtype=torch.int64, device="cuda"))
    with pytest.raises(DasacError):
        ops.view_consistency(y, 4, torch.zeros(ops.consistency_size(19, 4), dtype=torch.int32, device="cuda"))
    with pytest.raises(DasacError):
        ops.view_consistency(y, 4, torch.zeros(2 * ops.consistency_size(19, 4), dtype=torch.int64, device="cuda")[::2])
    _check(ops.view_consistency(x[:, :19], 4), y.cpu().numpy(), 4)                      # a non-contiguous INPUT is copied


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net19(g19):
    return _build(g19)


def test_validation_with_view_consistency_end_to_end(g19, net19):
    import driver
    T = int(g19["T"])
    kw = dict(step="target", group_size=T, max_iter=int(g19["max_iter"]), ignore_classes=[9, 14, 16])
    keys = list(net19.state_dict())
    assert net19.consistency_tables() is None
    plain = driver.validation(net19, _loader(g19, "tgt"), **kw)
    assert plain.consistency == {} and plain.consistency_summary is None
    assert net19.consistency_tables() is None                                          # off: nothing collected, nothing allocated
    seen = []

    def keep(module, args, output):
        seen.append(output[1]["teacher_aligned"].cpu().numpy())
    hook = net19.register_forward_hook(keep)
    try:
        res = driver.validation(net19, _loader(g19, "tgt"), consistency=True, **kw)
    finally:
        hook.remove()
    assert len(seen) == int(g19["counted"]) and seen[0].shape[1] == 19
    # the tables of the pass's own aligned views: real soft-max outputs, and still exact
    want = [sum(parts) for parts in zip(*(view_consistency_ref(a, T) for a in seen))]
    assert list(res.consistency) == ["agree", "flips", "per_view"]
    for name, w in zip(res.consistency, want):
        got = res.consistency[name]
        assert got.dtype == torch.int64 and not got.is_cuda and np.array_equal(got.numpy(), w), name
    assert int(res.consistency["agree"].sum()) == sum(a.shape[0] // T * a.shape[2] * a.shape[3] for a in seen)
    assert int(res.consistency["agree"][:19, 2:].sum()) > 0                            # views do overlap in this fixture
    assert res.consistency_summary == driver.summarise_consistency(res.consistency, [9, 14, 16])
    assert 0 < res.consistency_summary["agreement"] <= 1 and res.consistency_summary["classes_present"] >= 1
    assert driver.format_consistency(res.consistency_summary, range(19)).count("\n") >= 20
    # everything the default run returns, unchanged
    assert list(res.counts) == LAYERS["tgt"] and res.losses == plain.losses
    assert res.checkpoint_score == plain.checkpoint_score and res.mean == plain.mean
    assert res.confusion == {} and res.reliability == {}
    for layer in LAYERS["tgt"]:
        assert torch.equal(res.counts[layer], plain.counts[layer]), layer
        assert all(torch.equal(a, b) for a, b in zip(res.per_class[layer], plain.per_class[layer])), layer
    # the model is left as it was: switch off, no accumulator, the same state dict
    assert net19.consistency_tables() is None and not net19._consistency_on
    assert list(net19.state_dict()) == keys
    with pytest.raises(ValueError):                                                    # tables sized for another class count
        driver.validation(net19, _loader(g19, "tgt"), consistency=True, **dict(kw, num_classes=18))
    assert net19.consistency_tables() is None and not net19._consistency_on
    # a switch and an accumulator of the user's own survive the pass, and neither touches the state dict
    net19.collect_consistency(True, cover=0.25)
    assert list(net19.state_dict()) == keys
    with torch.no_grad():
        f1, gt, f2, affine, affine_inv = (driver.prep_batch(t, t.shape[0], T, device="cuda") for t in _loader(g19, "tgt")[0])
        net19.eval()
        net19(f1, gt, f2, affine, affine_inv, use_teacher=True, update_teacher=False, T=T)
        net19.train()
    mine = net19.consistency_tables()
    before = mine.buffer.clone()
    assert int(before.sum()) > 0 and list(net19.state_dict()) == keys
    again = driver.validation(net19, _loader(g19, "tgt"), consistency=True, **kw)
    assert all(torch.equal(again.consistency[k], res.consistency[k]) for k in res.consistency)
    assert net19.consistency_tables() is mine and torch.equal(mine.buffer, before)
    assert net19._consistency_on and net19._consistency_cover == 0.25
    assert net19.consistency_tables(reset=True) is mine and net19.consistency_tables() is None
    net19.collect_consistency(False)


def test_validation_with_view_consistency_runs_no_aten_arithmetic_on_tensors(g19, net19):
    import driver
    kw = dict(step="target", group_size=int(g19["T"]), max_iter=0, ignore_classes=[9, 14, 16], consistency=True)
    driver.validation(net19, _loader(g19, "tgt"), **kw)                                # first call: caches
    loader = _loader(g19, "tgt")
    with Recorder() as rec:
        res = driver.validation(net19, loader, **kw)
        torch.cuda.synchronize()
    assert res.checkpoint_score > 0 and int(res.consistency["agree"].sum()) > 0
    assert not rec.big, sorted(set(rec.big))[:12]
