"""Multi-scale and mirrored inference: ops.image_pyramid, ops.infer_fuse, driver.infer_label_maps_ms and the multi-scale forms of
driver.validation_iou -- against the plain torch composition on the CPU in float64

    F.interpolate(bilinear, align_corners=True) -> .flip(-1) -> .softmax(1) -> sum / S or torch.maximum -> topk(2)

The same composition in float32 gives e32, the fp32 rounding of the reference itself; tol = max(1e-5, 2 * e32), where 1e-5 is the
bound test_fused_inference_labels_match_oracle holds the same per-source arithmetic to.  Labels may differ from the float64 ones
only where the float64 top-2 gap is below tol.  Every figure is printed before it is asserted."""
import ctypes
import functools
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from conftest import rel_err

pytestmark = pytest.mark.gpu

CASE1 = dict(B=2, C=19, size=(61, 83), shapes=[(9, 12), (17, 23), (5, 7), (9, 12), (61, 83)], flips=[0, 1, 0, 1, 0])
CASE2 = dict(B=1, C=5, size=(33, 29), shapes=[(1, 3), (9, 7), (4, 1)], flips=[1, 0, 1])
# (case, source) of _logits() whose single-source label map is pinned by tests/golden/g21_infer_labels_bits.npz: 19 classes (the
# compile-time instantiation) at 17 x 23 -> 61 x 83 and at unit scale (weights (1, 0)); 5 classes (runtime C) from one row and
# from one column (degenerate taps).  make_goldens_infer_bits.py stores entry i as labels_i / conf_i.
BITS_INPUTS = ((0, 1), (0, 4), (1, 0), (1, 2))


@functools.lru_cache(maxsize=None)
def _logits():
    """The sources of case 1, then those of case 2, drawn in that order from one generator."""
    g = torch.Generator().manual_seed(23)
    return tuple([torch.randn(case["B"], case["C"], h, w, generator=g) * 3 for h, w in case["shapes"]] for case in (CASE1, CASE2))


def compose(sources, flips, size, mode, dtype):
    """(fused probabilities, labels, winning value, top-2 gap) of the torch composition in `dtype` on the CPU."""
    fused = None
    for x, flip in zip(sources, flips):
        p = F.interpolate(x.detach().cpu().to(dtype), size=tuple(size), mode="bilinear", align_corners=True)
        p = (p.flip(-1) if flip else p).softmax(1)
        fused = p if fused is None else (fused + p if mode == "mean" else torch.maximum(fused, p))
    if mode == "mean":
        fused = fused / len(sources)
    top = fused.topk(2, dim=1)
    return fused, top.indices[:, 0], top.values[:, 0], top.values[:, 0] - top.values[:, 1]


@functools.lru_cache(maxsize=None)
def _reference(case_index, mode):
    case, sources = (CASE1, CASE2)[case_index], _logits()[case_index]
    probs64, lab64, conf64, gap64 = compose(sources, case["flips"], case["size"], mode, torch.float64)
    probs32 = compose(sources, case["flips"], case["size"], mode, torch.float32)[0]
    e32 = float((probs32.double() - probs64).abs().max())
    return probs64, lab64, conf64, gap64, max(1e-5, 2 * e32), e32


def _check_against_float64(case_index, mode):
    from dasac_hip import ops
    case = (CASE1, CASE2)[case_index]
    probs64, lab64, conf64, gap64, tol, e32 = _reference(case_index, mode)
    dev = [x.cuda() for x in _logits()[case_index]]
    lab, conf, probs = ops.infer_fuse(dev, case["flips"], case["size"], mode, want_conf=True, want_probs=True)
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (case["B"],) + case["size"]
    assert tuple(probs.shape) == (case["B"], case["C"]) + case["size"]
    diff = lab.cpu().long() != lab64
    e_conf, e_probs = float((conf.cpu().double() - conf64).abs().max()), float((probs.cpu().double() - probs64).abs().max())
    print("case {} {}: e32 {:.2e} tol {:.2e} near-ties {} differing labels {} |conf err| {:.2e} |probs err| {:.2e}".format(
        case_index + 1, mode, e32, tol, int((gap64 < tol).sum()), int(diff.sum()), e_conf, e_probs))
    assert int(diff.sum()) == int((diff & (gap64 < tol)).sum())          # only near-ties of the reference may differ
    assert float(diff.double().mean()) <= 1e-3
    assert e_conf <= tol and e_probs <= tol
    # the optional outputs do not change the labels
    assert torch.equal(ops.infer_fuse(dev, case["flips"], case["size"], mode)[0], lab)
    return dev, lab


@pytest.mark.parametrize("mode", ["mean", "max"])
def test_infer_fuse_matches_float64_composition_19_classes(mode):
    """B = 2, 61 x 83 (odd height, width no multiple of 4), five sources of four sizes -- one of them at the output size -- two
    of them mirrored; with and without the id LUT."""
    import driver
    from dasac_hip import ops
    dev, lab = _check_against_float64(0, mode)
    lut = torch.tensor(driver.CITYSCAPES_TRAIN_TO_ID, dtype=torch.uint8, device="cuda")
    lab_lut, conf, probs = ops.infer_fuse(dev, CASE1["flips"], CASE1["size"], mode, lut=lut)
    assert conf is None and probs is None
    assert torch.equal(lut[lab.long()], lab_lut)
    diff = lab_lut.cpu() != lut.cpu()[_reference(0, mode)[1]]
    assert int(diff.sum()) == int((diff & (_reference(0, mode)[3] < _reference(0, mode)[4])).sum())


@pytest.mark.parametrize("mode", ["mean", "max"])
def test_infer_fuse_generic_class_count_and_degenerate_taps(mode):
    """Five classes (the runtime-C instantiation) from a one-row, a one-column and an ordinary source."""
    _check_against_float64(1, mode)


def test_infer_fuse_exact_identities(golden):
    """dasac_infer_labels and dasac_infer_fuse over one unflipped source run the same kernel, so comparing them with each other
    says nothing: both are held to the stored bits of the separate infer_labels<CT> kernel that preceded it (g21, labels and
    confidence), and the winner among `probs` to the confidence."""
    from dasac_hip import ops, DasacError
    from dasac_hip import lib as L
    g21 = golden("g21_infer_labels_bits")
    bits = lambda t: t.cpu().numpy().view(np.uint32)
    for i, (case_index, source) in enumerate(BITS_INPUTS):
        x, size = _logits()[case_index][source].cuda(), (CASE1, CASE2)[case_index]["size"]
        assert tuple(x.shape) == tuple(g21["shape_%d" % i])
        lab1, conf1 = ops.infer_labels(x, size, want_conf=True)
        lab, conf, probs = ops.infer_fuse([x], [0], size, "mean", want_conf=True, want_probs=True)
        for got_lab, got_conf in ((lab1, conf1), (lab, conf)):
            assert np.array_equal(got_lab.cpu().numpy(), g21["labels_%d" % i])
            assert np.array_equal(bits(got_conf), g21["conf_%d" % i].view(np.uint32))
        assert np.array_equal(bits(probs.gather(1, lab.long()[:, None])[:, 0]), bits(conf))
        assert np.array_equal(bits(probs.max(1).values), bits(conf))
    x = _logits()[0][1].cuda()                       # [2,19,17,23]
    size = CASE1["size"]
    lab, conf, probs = ops.infer_fuse([x], [0], size, "mean", want_conf=True, want_probs=True)
    labf, conff, probsf = ops.infer_fuse([x], [1], size, "mean", want_conf=True, want_probs=True)
    assert torch.equal(labf, lab.flip(-1)) and torch.equal(conff, conf.flip(-1)) and torch.equal(probsf, probs.flip(-1))
    one = ops.infer_fuse([x], [0], size, "max", want_conf=True, want_probs=True)
    eight = ops.infer_fuse([x] * 8, [0] * 8, size, "max", want_conf=True, want_probs=True)
    assert all(torch.equal(a, b) for a, b in zip(one, eight))
    # nine sources: the entry refuses and launches nothing
    table = (L.InferSource * 9)(*[L.InferSource(x.data_ptr(), 17, 23, 0, 0)] * 9)
    out = torch.full((2,) + size, 171, dtype=torch.uint8, device="cuda")
    code = L.load().dasac_infer_fuse(ctypes.cast(table, ctypes.c_void_p), 9, 2, 19, size[0], size[1], 0, 0, out.data_ptr(), 0, 0,
                                     L.stream_ptr())
    torch.cuda.synchronize()
    assert code == -1 and b"9 sources" in L.load().dasac_last_error() and bool((out == 171).all())
    with pytest.raises(DasacError):
        ops.infer_fuse([x] * 9, [0] * 9, size)


@pytest.mark.parametrize("size", [(19, 27), (37, 53), (46, 66)])
@pytest.mark.parametrize("with_flip", [0, 1])
def test_image_pyramid_matches_float64_interpolate(size, with_flip):
    from dasac_hip import ops
    x = torch.randn(2, 3, 37, 53, generator=torch.Generator().manual_seed(5))
    out = ops.image_pyramid(x.cuda(), size, bool(with_flip)).cpu()
    assert tuple(out.shape) == (4 if with_flip else 2, 3) + size
    want = F.interpolate(x.double(), size=size, mode="bilinear", align_corners=True)
    err = rel_err(out[:2], want)
    print("image_pyramid {} flip {}: rel_err {:.2e}".format(size, with_flip, err))
    assert err < 1e-6
    if with_flip:
        assert torch.equal(out[2:], out[:2].flip(-1))
    if size == (37, 53):
        assert torch.equal(out[:2], x)


# ---- through the model ---------------------------------------------------------------------------------------------------------
# Seed 0 for the weights and the image; the share of near-tie pixels of the float64 composition itself is printed by the test.
@pytest.fixture(scope="module")
def net():
    import driver
    import models
    from oracle.step_ref import DEFAULT_CFG
    d = dict(DEFAULT_CFG)
    d.update(INIT_MODEL="", OPT_NESTEROV=False)
    model = models.get_model(NS(**d), 0, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    driver.init_synthetic_weights(model, seed=0)
    model.cuda().eval()
    driver.calibrate_classifier(model, torch.randn(1, 3, 65, 81, generator=torch.Generator().manual_seed(0)).cuda())
    return model


def test_infer_label_maps_ms_through_the_model(net):
    """deeplabv2_resnet101 at 65 x 81, scales (0.75, 1.0), mirrored: the label map equals the float64 composition over the logits
    the existing forward gives for ATen-resized and ATen-flipped inputs, at every pixel whose float64 top-2 gap is >= 1e-4; such
    near-ties are at most 1 % of the image.  Seed 0 for weights and image, as specified; the near-tie share of the float64
    composition with that seed has not been measured on a device yet (the test prints it before it asserts)."""
    import driver
    x = torch.randn(1, 3, 65, 81, generator=torch.Generator().manual_seed(0)).cuda()
    scales = (0.75, 1.0)
    lab, conf, probs = driver.infer_label_maps_ms(net, x, scales=scales, flip=True, want_conf=True, want_probs=True)
    assert lab.dtype == torch.uint8 and tuple(lab.shape) == (1, 65, 81)
    sources, flips = [], []
    with torch.no_grad():
        for s in scales:
            xs = F.interpolate(x, size=driver.scaled_size(65, 81, s), mode="bilinear", align_corners=True)
            for flip in (0, 1):
                sources.append(net(xs.flip(-1) if flip else xs, teacher=False)[0].cpu())
                flips.append(flip)
    assert tuple(sources[0].shape[-2:]) != tuple(sources[2].shape[-2:])        # the scales do reach the backbone
    probs64, lab64, conf64, gap64 = compose(sources, flips, (65, 81), "mean", torch.float64)
    near = gap64 < 1e-4
    diff = lab.cpu().long() != lab64
    print("through the model: near-ties {} of {}, differing labels {}, |conf err| {:.2e}, |probs err| {:.2e}".format(
        int(near.sum()), near.numel(), int(diff.sum()), float((conf.cpu().double() - conf64).abs().max()),
        float((probs.cpu().double() - probs64).abs().max())))
    assert not bool((diff & ~near).any())
    assert float(near.double().mean()) <= 0.01
    # one scale, unflipped: the single-scale path's bits
    single = driver.infer_label_maps_ms(net, x, scales=(1.0,), flip=False, want_conf=True)
    plain = driver.infer_label_maps(net, x, want_conf=True)
    assert torch.equal(single[0], plain[0]) and torch.equal(single[1], plain[1]) and single[2] is None


def test_validation_iou_multi_scale_counts_its_own_label_maps(net, monkeypatch):
    """The counting path: tp / fp / fn of validation_iou(scales, flip) equal those computed in torch from infer_label_maps_ms's
    own label maps (255 = ignore in the ground truth)."""
    import driver
    g = torch.Generator().manual_seed(3)
    batches = []
    for _ in range(2):
        gt = torch.randint(0, 19, (1, 33, 49), generator=g)
        gt[torch.rand(1, 33, 49, generator=g) < 0.2] = 255
        batches.append((torch.randn(1, 3, 33, 49, generator=g).cuda(), gt.cuda()))
    seen = []
    summarise = driver.summarise_iou
    monkeypatch.setattr(driver, "summarise_iou", lambda counts: (seen.append(counts.clone()), summarise(counts))[1])
    miou, iou = driver.validation_iou(net, batches, scales=(0.75, 1.0), flip=True)
    want = torch.zeros(3, 19, dtype=torch.int64)
    for image, gt in batches:
        pred = driver.infer_label_maps_ms(net, image, scales=(0.75, 1.0), flip=True)[0].cpu().long()
        gt = gt.cpu()
        valid = gt != 255
        for c in range(19):
            want[0, c] += int(((pred == c) & (gt == c) & valid).sum())
            want[1, c] += int(((pred == c) & (gt != c) & valid).sum())
            want[2, c] += int(((pred != c) & (gt == c) & valid).sum())
    assert len(seen) == 1 and torch.equal(seen[0].cpu(), want)
    assert int(want.sum()) > 0 and torch.equal(iou, summarise(want)[0]) and miou == float(iou.mean())
    assert not net.training
