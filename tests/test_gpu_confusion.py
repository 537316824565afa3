"""`dasac_confusion_counts` on the GPU: the confusion matrices and reliability tables of the validation pass against the numpy
definitions of tests/test_confusion_cpu.py, against `ops.mask_counts` / `ops.iou_counts` through the identity
tp = M[c][c], fp = column - tp, fn = row - tp, on the reference's own tensors (g19), and `driver.validation` /
`driver.validation_iou` end to end with the options on.

Bounds.  Every table is integers: exact -- with one derived band.  A logits layer is binned by 1 / sum_c expf(x_c - max) in
fp32, the reference here is a float64 soft-max: fp32 evaluation over 19 terms carries about 1.5e-6 relative error, 2.4e-5 bins at
16 bins, so a pixel whose float64 confidence x n_bins lies within 1e-4 (four times that) of an integer may fall in either
adjacent bin; every other pixel, and every class / hit marginal, must match exactly, and such pixels must stay under 1 % of the
counted ones (N(0, 3^2) logits put 0.03 % there)."""
import numpy as np
import pytest
import torch

from test_confusion_cpu import argmax_first, bin_of, confusion_ref, reliability_ref, softmax_max64
from test_gpu_validation import EINVAL, LAYERS, SCORE_LAYERS, Recorder, _build, _loader, _window, g19  # noqa: F401  (g19: fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(2, 19, 7, 9, 0), (1, 19, 1, 3, 0), (3, 19, 129, 257, 0), (2, 19, 23, 31, 1), (2, 19, 16, 16, 3),
          (2, 5, 13, 17, 0), (1, 5, 8, 8, 1), (2, 64, 9, 11, 0), (1, 1, 5, 5, 0)]


def _counts(M):
    """(tp, fp, fn) of matrices [..., C+1, C+1] in numpy: the identity, restated."""
    M = M.cpu().numpy() if torch.is_tensor(M) else M
    C = M.shape[-1] - 1
    tp = np.diagonal(M, axis1=-2, axis2=-1)[..., :C]
    return np.stack([tp, M[..., :, :C].sum(-2) - tp, M[..., :C, :].sum(-1) - tp], -2)


def _place(t, offset):
    """`t` on the device, starting `offset` ELEMENTS into its allocation (offset > 0: the base pointer is not 16-byte aligned)."""
    flat = torch.empty(t.numel() + offset, dtype=t.dtype, device="cuda")
    view = flat[offset:].view(t.shape)
    view.copy_(t)
    return view


def _random_case(B, C, H, W, seed):
    """scores with exact ties, a label map with 255 and a value >= C, gt with 255, -1, a value >= C and 255 over 255."""
    g = torch.Generator().manual_seed(seed)
    scores = [torch.randn(B, C, H, W, generator=g) for _ in range(2)]
    scores[1][:, :, : H // 2] = scores[1][:, :1, : H // 2]                            # exact ties: the first maximum must win
    labels = torch.randint(0, C, (B, H, W), generator=g)
    labels[torch.rand(B, H, W, generator=g) < 0.4] = 255
    gt = torch.randint(0, C, (B, H, W), generator=g)
    same = torch.rand(B, H, W, generator=g) < 0.3
    gt[same] = labels[same]                                                         # includes 255 over 255
    gt[torch.rand(B, H, W, generator=g) < 0.1] = 255
    gt[0, 0, : min(W, 5)] = -1
    labels[-1, -1, -1], gt[-1, -1, -2:] = C, C + 1                                   # values >= C: no class, not ignored
    labels[0, 0, 0], gt[0, 0, 0] = 255, 255
    return scores, labels, gt


# ---------------------------------------------------------------------------------------------------------------------
# the reference's own tensors
# ---------------------------------------------------------------------------------------------------------------------
def test_confusion_counts_give_the_reference_counts_on_its_own_tensors(g19):
    import driver
    from dasac_hip import ops
    n_win = int(g19["win"][3])
    M, counts, M_u8 = None, None, None
    single = [None] * 4
    for b in range(n_win):
        scores, labels, gt = _window(g19, b)
        assert (scores[0].shape[-2] * scores[0].shape[-1]) % 4 != 0                  # the tail path is part of this test
        M, none = ops.confusion_counts(scores, [labels], gt, M)                      # all four layers, ONE launch, accumulating
        assert none is None
        M_u8, _ = ops.confusion_counts(scores, [labels.to(torch.uint8)], gt, M_u8)   # the label map as uint8
        counts = ops.mask_counts(scores, [labels], gt, counts)
        for i in range(3):
            single[i], _ = ops.confusion_counts([scores[i]], [], gt, single[i])      # one layer at a time
        single[3], _ = ops.confusion_counts([], [labels], gt, single[3], num_classes=19)
        derived = driver.counts_from_confusion(M)
        assert torch.equal(derived, counts.cpu()) and np.array_equal(derived.numpy(), _counts(M))
        for i, layer in enumerate(LAYERS["tgt"]):
            assert torch.equal(derived[i], torch.from_numpy(g19["win%d_%s_counts" % (b, layer)])), (b, layer)
            assert torch.equal(single[i][0], M[i]), (b, layer)
        assert torch.equal(M_u8, M)
    assert int(M[3, :19, 19].sum()) > 0                                              # rejected pseudo labels are counted, as column C


# ---------------------------------------------------------------------------------------------------------------------
# random, uniform and blocky maps
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,H,W,offset", SHAPES)
def test_confusion_counts_edge_shapes_match_numpy_bincount(B, C, H, W, offset):
    from dasac_hip import ops
    scores, labels, gt = _random_case(B, C, H, W, 100 + H)
    d_scores, d_labels, d_gt = [_place(s, offset) for s in scores], _place(labels, offset), _place(gt, offset)
    if offset:
        assert d_scores[0].data_ptr() % 16 != 0 and d_gt.data_ptr() % 16 != 0 and d_scores[0].is_contiguous()
    want = np.stack([confusion_ref(argmax_first(s.numpy())[0], gt, C) for s in scores] + [confusion_ref(labels, gt, C)])
    got, _ = ops.confusion_counts(d_scores, [d_labels], d_gt, num_classes=C)
    again, _ = ops.confusion_counts(d_scores, [d_labels], d_gt, num_classes=C)
    assert torch.equal(got, again)                                                  # two runs, the same bits
    assert np.array_equal(got.cpu().numpy(), want)
    assert all(int(got[i].sum()) == int((gt != 255).sum()) for i in range(3))       # every pixel that is not ignored, once
    assert int(got[2, C, C]) > 0                                                    # a label and a gt that are both no class
    counts = ops.mask_counts(d_scores, [d_labels], d_gt, num_classes=C)
    assert np.array_equal(_counts(got), counts.cpu().numpy())                       # the identity, against the marginal kernel
    for i in range(2):
        assert np.array_equal(_counts(got[i]), ops.iou_counts(d_scores[i], d_gt).cpu().numpy())
        assert torch.equal(ops.confusion_counts([d_scores[i]], [], d_gt)[0][0], got[i])
    acc, _ = ops.confusion_counts(d_scores, [d_labels], d_gt, got.clone())          # accumulates into what is there
    assert torch.equal(acc, 2 * got)
    for off in sorted({offset, 1}):                                                 # uint8 map, also at an odd address
        d_u8 = _place(labels.to(torch.uint8), off)
        assert off != 1 or d_u8.data_ptr() % 2 == 1
        both, _ = ops.confusion_counts([], [d_u8, d_labels], d_gt, num_classes=C)
        assert torch.equal(both[0], got[2]) and torch.equal(both[1], got[2]), off
    other = ops.confusion_counts(d_scores[:1], [d_labels], d_gt, ignore_index=C - 1)[0]                   # another ignore index: 255 is a value
    assert np.array_equal(other.cpu().numpy(), np.stack([confusion_ref(argmax_first(scores[0].numpy())[0], gt, C, C - 1),
                                                         confusion_ref(labels, gt, C, C - 1)]))


def test_confusion_counts_uniform_maps():
    from dasac_hip import ops
    B, C, H, W = 2, 19, 37, 53
    hw = B * H * W
    scores = torch.zeros(B, C, H, W, device="cuda")
    scores[:, 7] = 1.0
    labels = torch.full((B, H, W), 7, dtype=torch.int64, device="cuda")
    gt = torch.full((B, H, W), 7, dtype=torch.int64, device="cuda")

    def only(r, c):
        want = torch.zeros(C + 1, C + 1, dtype=torch.int64)
        want[r, c] = hw
        return want

    def run(labels=labels, gt=gt, **kw):
        return ops.confusion_counts([scores], [labels, labels.to(torch.uint8)], gt, **kw)[0].cpu()
    got = run()                                                                      # uniform maps: every wave merges to one add
    assert all(torch.equal(got[i], only(7, 7)) for i in range(3))
    got = run(gt=torch.full_like(gt, 3))                                             # uniformly wrong
    assert all(torch.equal(got[i], only(3, 7)) for i in range(3))
    assert int(run(gt=torch.full_like(gt, 255)).abs().sum()) == 0                    # gt all ignored
    got = run(labels=torch.full_like(labels, 255))                                   # no label anywhere: column C
    assert torch.equal(got[0], only(7, 7)) and torch.equal(got[1], only(7, C)) and torch.equal(got[2], only(7, C))
    got = run(gt=torch.full_like(gt, -1))                                            # gt outside the classes: row C
    assert all(torch.equal(got[i], only(C, 7)) for i in range(3))
    got = run(labels=torch.full_like(labels, 255), gt=torch.full_like(gt, -1))
    assert torch.equal(got[1], only(C, C)) and torch.equal(got[2], only(C, C))
    assert int(run(ignore_index=7).abs().sum()) == 0                                 # another ignore index
    got = run(gt=torch.full_like(gt, 255), ignore_index=7)                           # ... under which 255 is a value like any other
    assert all(torch.equal(got[i], only(C, 7)) for i in range(3))


def test_confusion_counts_blocky_maps():
    """8 x 8 constant blocks: threads with four equal keys beside threads with runs, several keys per wave."""
    from dasac_hip import ops
    B, C, H, W = 2, 19, 70, 90
    g = torch.Generator().manual_seed(5)

    def blocks(values):
        small = values[torch.randint(0, len(values), (B, (H + 7) // 8, (W + 7) // 8), generator=g)]
        return small.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W].contiguous()
    classes = torch.arange(C)
    gt = blocks(torch.cat([classes, torch.tensor([255, 255, -1])]))
    labels = blocks(torch.cat([classes, torch.tensor([255] * 6)]))
    pred = blocks(classes)
    scores = torch.nn.functional.one_hot(pred, C).permute(0, 3, 1, 2).float().contiguous()
    got, rel = ops.confusion_counts([scores.cuda()], [labels.cuda(), labels.to(torch.uint8).cuda()], gt.cuda(), bins=4)
    assert np.array_equal(got[0].cpu().numpy(), confusion_ref(pred, gt, C))
    assert np.array_equal(got[1].cpu().numpy(), confusion_ref(labels, gt, C)) and torch.equal(got[1], got[2])
    assert np.array_equal(rel[0].cpu().numpy(), reliability_ref(pred, np.full(pred.shape, 3), gt, C, 4))     # confidence 1.0: the last bin


# ---------------------------------------------------------------------------------------------------------------------
# reliability
# ---------------------------------------------------------------------------------------------------------------------
def _check_sums(rel, M):
    """sum_b rel[p][b][1] = M[p][p], sum_b rel[p][b][0] = sum_r M[r][p] - M[p][p]."""
    C = M.shape[0] - 1
    assert np.array_equal(rel[:, :, 1].sum(1), np.diag(M)[:C])
    assert np.array_equal(rel[:, :, 0].sum(1), M[:, :C].sum(0) - np.diag(M)[:C])


@pytest.mark.parametrize("n_bins", [1, 10, 16, 32])
@pytest.mark.parametrize("C", [19, 5])
def test_reliability_of_a_probability_layer_is_exact(C, n_bins):
    from dasac_hip import ops
    B, H, W = 2, 23, 31
    g = torch.Generator().manual_seed(n_bins + C)
    probs = torch.softmax(torch.randn(B, C, H, W, generator=g) * 3, 1)
    for k in range(n_bins + 1):                                                      # winning values exactly k / n_bins (0 and 1.0 among them)
        probs[0, :, 2 + k // W, k % W] = 0
        probs[0, 3, 2 + k // W, k % W] = float(np.float32(k) / np.float32(n_bins))
    probs[1, :, 0, 0] = float("nan")                                                 # NaN: class 0, bin 0
    probs[1, :, 0, 1], probs[1, 2, 0, 1] = 0, 2.5                                    # above 1: the last bin
    probs[1, :, 0, 2] = -1.0                                                         # nothing positive: class 0, bin 0
    gt = torch.randint(0, C, (B, H, W), generator=g)
    hit = torch.rand(B, H, W, generator=g) < 0.5
    arg, best = argmax_first(probs.numpy())
    gt[hit] = torch.from_numpy(arg)[hit]
    gt[torch.rand(B, H, W, generator=g) < 0.1] = 255
    gt[0, 0, :3] = -1
    assert best.dtype == np.float32 and arg[1, 0, 0] == 0 and arg[1, 0, 2] == 0
    want = reliability_ref(arg, bin_of(best, n_bins), gt, C, n_bins)
    M, rel = ops.confusion_counts([probs.cuda()], [], gt.cuda(), bins=n_bins)
    assert tuple(rel.shape) == (1, C, n_bins, 2) and rel.dtype == torch.int64
    assert np.array_equal(rel[0].cpu().numpy(), want)
    assert np.array_equal(M[0].cpu().numpy(), confusion_ref(arg, gt, C))
    _check_sums(rel[0].cpu().numpy(), M[0].cpu().numpy())
    M2, rel2 = ops.confusion_counts([probs.cuda()], [], gt.cuda(), M.clone(), rel.clone())               # accumulates; bins from the tensor
    assert torch.equal(rel2, 2 * rel) and torch.equal(M2, 2 * M)


def _check_banded(got, arg, p64, gt, C, n_bins):
    """`got` [C,n_bins,2] against float64 confidences: pixels outside the band exactly, band pixels in either adjacent bin."""
    x = p64 * n_bins
    edge = np.rint(x).astype(np.int64)
    band = (np.abs(x - edge) < 1e-4) & (gt != 255)
    counted = int((gt != 255).sum())
    print("bins", n_bins, "band pixels", int(band.sum()), "of", counted)
    assert band.sum() < 0.01 * counted
    fixed = reliability_ref(arg[~band], bin_of(p64[~band], n_bins, np.float64), gt[~band], C, n_bins)
    assert np.array_equal(got.sum(1), reliability_ref(arg, bin_of(p64, n_bins, np.float64), gt, C, n_bins).sum(1))   # class / hit marginals
    rest = got - fixed                                                              # what the band pixels added
    assert (rest >= 0).all()
    # n[p][k][h]: band pixels at edge k (between bins k - 1 and k); edge n_bins can only land in the last bin
    n = np.zeros((C, n_bins + 1, 2), np.int64)
    np.add.at(n, (arg[band], edge[band], (arg[band] == gt[band]).astype(np.int64)), 1)
    assert n[:, 0].sum() == 0                                                       # a soft-max maximum is at least 1 / C
    upper = np.zeros((C, 2), np.int64)                                              # of edge b's pixels, those that took bin b
    for b in range(n_bins):
        nxt = n[:, b + 1] if b + 1 < n_bins else np.zeros((C, 2), np.int64)
        lower = rest[:, b] - upper                                                  # of edge b + 1's pixels, those that took bin b
        if b + 1 == n_bins:
            lower = lower - n[:, n_bins]
            assert (lower == 0).all()
        else:
            assert ((lower >= 0) & (lower <= nxt)).all(), b
        upper = nxt - lower


@pytest.mark.parametrize("B,C,H,W,n_bins", [(4, 19, 129, 257, 16), (2, 19, 23, 31, 10), (2, 5, 23, 31, 16)])
def test_reliability_of_a_logits_layer_matches_a_float64_softmax(B, C, H, W, n_bins):
    from dasac_hip import ops
    g = torch.Generator().manual_seed(C + n_bins)
    logits = torch.randn(B, C, H, W, generator=g) * 3
    probs = torch.softmax(torch.randn(B, C, H, W, generator=g), 1)
    arg, _ = argmax_first(logits.numpy())
    gt = torch.randint(0, C, (B, H, W), generator=g)
    hit = torch.rand(B, H, W, generator=g) < 0.5
    gt[hit] = torch.from_numpy(arg)[hit]
    gt[torch.rand(B, H, W, generator=g) < 0.1] = 255
    gt = gt.numpy()
    # a logits layer beside a probability layer in ONE launch: the flag is per layer
    M, rel = ops.confusion_counts([logits.cuda(), probs.cuda()], [], torch.from_numpy(gt).cuda(), bins=n_bins, logits_layers=[0])
    M, rel = M.cpu().numpy(), rel.cpu().numpy()
    _check_banded(rel[0], arg, softmax_max64(logits.numpy()), gt, C, n_bins)
    arg1, best1 = argmax_first(probs.numpy())
    assert np.array_equal(rel[1], reliability_ref(arg1, bin_of(best1, n_bins), gt, C, n_bins))
    for l in range(2):
        _check_sums(rel[l], M[l])
    assert np.array_equal(M[0], confusion_ref(arg, gt, C))


# ---------------------------------------------------------------------------------------------------------------------
# bad arguments
# ---------------------------------------------------------------------------------------------------------------------
def test_confusion_counts_refuses_bad_arguments():
    from dasac_hip import lib as L, ops, DasacError
    lib = L.load()
    s = torch.zeros(1, 19, 4, 4, device="cuda")
    m = torch.zeros(1, 4, 4, dtype=torch.int64, device="cuda")
    big = torch.zeros(1, 65, 4, 4, device="cuda")
    out = torch.zeros(2, 66, 66, dtype=torch.int64, device="cuda")
    rel = torch.zeros(1, 65, 32, 2, dtype=torch.int64, device="cuda")

    def call(s0=s.data_ptr(), m0=m.data_ptr(), gt=m.data_ptr(), B=1, C=19, HW=16, conf=out.data_ptr(), rel=0, n_bins=0):
        return lib.dasac_confusion_counts(s0, 0, 0, 0, m0, 0, 0, gt, B, C, HW, 255, conf, rel, n_bins, 0, L.stream_ptr())
    assert call() == 0
    assert call(gt=0) == EINVAL                     # null gt
    assert call(conf=0) == EINVAL                   # null confusion
    assert call(s0=0, m0=0) == EINVAL               # no layer at all
    assert call(B=0) == EINVAL and call(B=-1) == EINVAL
    assert call(C=0) == EINVAL
    assert call(HW=0) == EINVAL and call(HW=-4) == EINVAL
    assert call(s0=big.data_ptr(), C=65) == EINVAL  # C > 64
    assert call(s0=big.data_ptr(), C=64) == 0
    assert call(rel=rel.data_ptr(), n_bins=0) == EINVAL and call(rel=rel.data_ptr(), n_bins=33) == EINVAL and \
        call(rel=rel.data_ptr(), n_bins=-1) == EINVAL
    assert b"confusion_counts" in lib.dasac_last_error()
    assert call(rel=rel.data_ptr(), n_bins=32) == 0 and call(rel=0, n_bins=99) == 0       # without a table n_bins is not read
    torch.cuda.synchronize()
    with pytest.raises(DasacError):
        ops.confusion_counts([], [], m)
    with pytest.raises(DasacError):
        ops.confusion_counts([s.cpu()], [], m.cpu())                 # no CPU path
    with pytest.raises(DasacError):
        ops.confusion_counts([s], [m.to(torch.int32)], m)
    with pytest.raises(DasacError):
        ops.confusion_counts([s.double()], [], m)
    with pytest.raises(DasacError):
        ops.confusion_counts([s], [], m.to(torch.uint8))             # the ground truth is int64
    with pytest.raises(DasacError):
        ops.confusion_counts([s] * 5, [], m)
    with pytest.raises(DasacError):
        ops.confusion_counts([], [m] * 3, m, num_classes=19)
    with pytest.raises(DasacError):
        ops.confusion_counts([], [m], m)                             # label maps alone do not tell C
    with pytest.raises(DasacError):
        ops.confusion_counts([s], [], m, bins=33)
    with pytest.raises(DasacError):
        ops.confusion_counts([], [m], m, num_classes=19, bins=4)     # a reliability table needs a score layer
    with pytest.raises(DasacError):
        ops.confusion_counts([s], [], m, bins=4, logits_layers=[1])
    with pytest.raises(DasacError):
        ops.confusion_counts([s], [], m, torch.zeros(1, 20, 19, dtype=torch.int64, device="cuda"))


def test_confusion_counts_largest_tables():
    """64 classes, every slot used, 32 bins: more tables than one workgroup's LDS holds (the two-launch split)."""
    from dasac_hip import ops
    B, C, H, W = 1, 64, 9, 11
    scores, labels, gt = _random_case(B, C, H, W, 7)
    scores = scores + [scores[0].flip(1).contiguous(), scores[1] * 0.5]
    M, rel = ops.confusion_counts([s.cuda() for s in scores], [labels.cuda(), labels.to(torch.uint8).cuda()], gt.cuda(), bins=32)
    want = [confusion_ref(argmax_first(s.numpy())[0], gt, C) for s in scores] + [confusion_ref(labels, gt, C)] * 2
    assert np.array_equal(M.cpu().numpy(), np.stack(want))
    for l, s in enumerate(scores):
        arg, best = argmax_first(s.numpy())
        assert np.array_equal(rel[l].cpu().numpy(), reliability_ref(arg, bin_of(best, 32), gt, C, 32)), l


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net19(g19):
    return _build(g19)


def test_validation_with_the_joint_tables_end_to_end(g19, net19):
    import driver
    bins = 10
    kw = dict(step="target", group_size=int(g19["T"]), max_iter=int(g19["max_iter"]), ignore_classes=[9, 14, 16])
    plain = driver.validation(net19, _loader(g19, "tgt"), **kw)
    assert plain.confusion == {} and plain.reliability == {}
    seen = []

    def keep(module, args, output):
        _, outs = output
        seen.append(({layer: outs[layer].cpu().numpy() for layer in LAYERS["tgt"]}, args[1].view(-1, *args[1].shape[-2:]).cpu().numpy().copy()))
    hook = net19.register_forward_hook(keep)
    try:
        res = driver.validation(net19, _loader(g19, "tgt"), confusion=True, reliability_bins=bins, **kw)
    finally:
        hook.remove()
    assert len(seen) == int(g19["counted"])
    # everything the default run returns, unchanged
    assert list(res.counts) == LAYERS["tgt"] and sorted(res.losses) == sorted(plain.losses)
    assert res.checkpoint_score == plain.checkpoint_score and res.mean == plain.mean
    for layer in LAYERS["tgt"]:
        assert res.counts[layer].dtype == torch.int64 and torch.equal(res.counts[layer], plain.counts[layer]), layer
        assert all(torch.equal(a, b) for a, b in zip(res.per_class[layer], plain.per_class[layer])), layer
    # the tables of its own layer maps
    assert list(res.confusion) == LAYERS["tgt"] and list(res.reliability) == SCORE_LAYERS
    for layer in LAYERS["tgt"]:
        want = sum(confusion_ref(t[layer] if layer == "teacher_labels" else argmax_first(t[layer])[0], gt, 19) for t, gt in seen)
        assert tuple(res.confusion[layer].shape) == (20, 20) and np.array_equal(res.confusion[layer].numpy(), want), layer
    want = np.zeros((19, bins, 2), np.int64)
    for t, gt in seen:
        arg, best = argmax_first(t["teacher_refined"])
        want += reliability_ref(arg, bin_of(best, bins), gt, 19, bins)
    assert np.array_equal(res.reliability["teacher_refined"].numpy(), want)                    # a probability layer: exact
    for layer in ("logits_up", "teacher_init"):                                                  # logits layers: the float64 band
        arg = np.concatenate([argmax_first(t[layer])[0].ravel() for t, _ in seen])
        p64 = np.concatenate([softmax_max64(t[layer]).ravel() for t, _ in seen])
        _check_banded(res.reliability[layer].numpy(), arg, p64, np.concatenate([gt.ravel() for _, gt in seen]), 19, bins)
    for layer in SCORE_LAYERS:
        _check_sums(res.reliability[layer].numpy(), res.confusion[layer].numpy())
    audit = driver.pseudo_label_audit(res.confusion["teacher_labels"], res.confusion["teacher_refined"])
    assert 0 < float(audit.coverage.max()) <= 1 and float(audit.coverage.min()) < 1               # the thresholds rejected something
    # the matrix alone
    only = driver.validation(net19, _loader(g19, "tgt"), confusion=True, **kw)
    assert only.reliability == {} and all(torch.equal(only.confusion[k], res.confusion[k]) for k in LAYERS["tgt"])


def test_validation_iou_returns_the_matrix(g19, net19):
    import driver
    batches = [(x.cuda(), y.cuda()) for x, y in _loader(g19, "src")]
    for net, kw in ((net19, dict(scales=(1.0,), flip=True)), (net19.backbone, {})):
        miou, iou = driver.validation_iou(net, batches, **kw)
        miou_m, iou_m, M = driver.validation_iou(net, batches, confusion=True, **kw)
        assert miou_m == miou and torch.equal(iou_m, iou)
        assert M.dtype == torch.int64 and tuple(M.shape) == (20, 20) and not M.is_cuda
        assert int(M.sum()) == sum(int((y != 255).sum()) for _, y in batches)
        assert torch.equal(driver.summarise_iou(driver.counts_from_confusion(M))[0], iou)


def test_validation_with_the_joint_tables_runs_no_aten_arithmetic_on_tensors(g19, net19):
    import driver
    kw = dict(step="target", group_size=int(g19["T"]), max_iter=0, ignore_classes=[9, 14, 16], confusion=True, reliability_bins=10)
    driver.validation(net19, _loader(g19, "tgt"), **kw)                                # first call: caches
    loader = _loader(g19, "tgt")
    with Recorder() as rec:
        res = driver.validation(net19, loader, **kw)
        torch.cuda.synchronize()
    assert res.checkpoint_score > 0 and int(res.confusion["logits_up"].sum()) > 0
    assert not rec.big, sorted(set(rec.big))[:12]
