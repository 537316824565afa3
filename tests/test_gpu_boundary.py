"""`dasac_boundary_counts` on the GPU against the numpy model of tests/boundary_ref.py, bit for bit: integer tables, so every
comparison is exact.  Blocky, random and uniform maps at sizes that are no multiple of the 32 x 64 tile, span several tiles with
contours on the seams, are smaller than the radius or one pixel thin; transparency of 255 / -1; int64 and uint8 label maps off
their natural alignment; NULL-slot numbering; ties in the arg-max; accumulation; the slot sums against `ops.mask_counts`; refused
arguments; and `driver.validation` end to end with `boundary_radius`."""
import numpy as np
import pytest
import torch

import boundary_ref as BR
from test_gpu_validation import EINVAL, LAYERS, Recorder, _build, _loader, g19  # noqa: F401  (g19: fixture)

pytestmark = pytest.mark.gpu

# (B, C, H, W, R): no multiple of the tile; several tiles each way; smaller than the radius; one pixel thin both ways; R = 1
SHAPES = [(2, 5, 37, 83, 16), (2, 19, 150, 270, 8), (3, 19, 5, 7, 16), (2, 19, 1, 64, 3), (2, 19, 64, 1, 3), (2, 5, 37, 83, 1)]


def _place(t, offset):
    """`t` on the device, starting `offset` ELEMENTS into its allocation."""
    flat = torch.empty(t.numel() + offset, dtype=t.dtype, device="cuda")
    view = flat[offset:].view(t.shape)
    view.copy_(t)
    return view


def _case(B, C, H, W, seed):
    """Two score tensors (one-hot blocky, and random with exact ties), a label map with 255 regions and the ground truth with 255 and
    -1 regions.  Image 0 is busy -- blocks of 6 (contours fall on and beside the 32 / 64 tile seams of the larger shapes) with a noisy
    corner; image 1 is UNIFORM in every map, each map its own class: a halo that leaks across images or rows shows there, and its
    pixels fill the last slot; a third image is random per pixel."""
    rng = np.random.default_rng(seed)
    classes = list(range(C))

    def draw(values, uniform):
        m = BR.blocky((B, H, W), values, 6, rng)
        m[0, : max(1, H // 4), : max(1, W // 4)] = rng.integers(0, C, (max(1, H // 4), max(1, W // 4)))
        if B > 1:
            m[1] = uniform
        if B > 2:
            m[2] = rng.integers(0, C, (H, W))
        return m
    gt = draw(classes + [255, 255, -1], 1 % C)
    gt[0, -1, -1], gt[0, H // 2, W // 2] = -1, 255                      # also where the blocks drew neither
    labels = draw(classes + [255] * 4, 1 % C)
    labels[0, -1, 0] = 255
    if B > 1:
        labels[1, H // 2:, W // 2:] = 255                               # a 255 region inside the uniform image: still no contour
    pred = draw(classes, 2 % C)
    hit = rng.random((B, H, W)) < 0.5
    pred[0][hit[0]] = np.where(gt[0] >= 0, gt[0], 0)[hit[0]] % C
    s0 = np.zeros((B, C, H, W), np.float32)
    np.put_along_axis(s0, pred[:, None], 1.0, 1)
    s1 = rng.standard_normal((B, C, H, W)).astype(np.float32)
    a, b = W // 3, 2 * W // 3
    s1[0, :, :, :a] = s1[0, :1, :, :a]                                  # exact ties over all classes: the first maximum wins, class 0
    s1[0, 2, :, a:b] = s1[0, 1, :, a:b] = np.abs(s1[0, :, :, a:b]).max(0) + 1.0     # a two-way tie at the top: class 1
    if B > 1:
        s1[1] = 0.0                                                     # uniform by ties: class 0
    return [s0, s1], labels, gt


@pytest.fixture(scope="module")
def cases():
    """Every shape's inputs and its model tables, computed once."""
    out = {}
    for B, C, H, W, R in SHAPES:
        scores, labels, gt = _case(B, C, H, W, 10 * H + W + R)
        out[(B, C, H, W, R)] = (scores, labels, gt, BR.boundary_tables(scores, [labels, labels], gt, C, R))
    return out


@pytest.mark.parametrize("B,C,H,W,R", SHAPES)
def test_boundary_counts_match_the_model_bit_for_bit(cases, B, C, H, W, R):
    from dasac_hip import ops
    scores, labels, gt, want = cases[(B, C, H, W, R)]
    d_scores = [_place(torch.from_numpy(s), 1) for s in scores]
    d_gt = _place(torch.from_numpy(gt), 1)
    d_i64 = _place(torch.from_numpy(labels), 1)
    d_u8 = _place(torch.from_numpy(labels.astype(np.uint8)), 1)
    assert d_u8.data_ptr() % 2 == 1 and d_i64.data_ptr() % 16 == 8 and d_scores[0].data_ptr() % 16 == 4
    assert gt.min() == -1 and (gt == 255).any() and (labels == 255).any()
    got = ops.boundary_counts(d_scores, [d_i64, d_u8], d_gt, radius=R)
    assert got.dtype == torch.int64 and tuple(got.shape) == (4, R + 1, 5, C)
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got[2], got[3])                                  # the same map as int64 and as uint8
    # near and far slots are both populated, by the ground truth's distances and by each predicted map's own
    for l in range(4):
        by_gt, by_pred = got[l, :, :3].sum((1, 2)), got[l, :, 3].sum(1)
        assert int(by_gt[:R].sum()) > 0 and int(by_gt[R]) > 0, (l, by_gt.tolist())
        assert int(by_pred[:R].sum()) > 0 and int(by_pred[R]) > 0, (l, by_pred.tolist())
    # summed over the slots: ops.mask_counts on the same tensors
    plain = ops.mask_counts(d_scores, [d_i64], d_gt)
    s = got.sum(1)
    for l in range(3):
        assert torch.equal(s[l, 0], plain[l, 0]) and torch.equal(s[l, 1], plain[l, 1]) and torch.equal(s[l, 2], plain[l, 2]), l
        assert torch.equal(s[l, 3], plain[l, 0] + plain[l, 1]) and torch.equal(s[l, 4], plain[l, 0]), l
    # two calls accumulate; two runs give the same bits
    again = ops.boundary_counts(d_scores, [d_i64, d_u8], d_gt, got.clone())
    assert torch.equal(again, 2 * got)


def test_boundary_counts_uniform_image_has_no_contour(cases):
    """Image 1 of every map is uniform (the label map with a 255 quarter, the second score tensor by ties): all of its pixels are in
    the last slot of every layer, whatever the busy image 0 next to it in memory holds."""
    from dasac_hip import ops
    B, C, H, W, R = SHAPES[1]
    scores, labels, gt, _ = cases[SHAPES[1]]
    one = lambda a: torch.from_numpy(np.ascontiguousarray(a[1:2])).cuda()
    alone = ops.boundary_counts([one(s) for s in scores], [one(labels)], one(gt), radius=R)
    assert int(alone[:, :R].sum()) == 0 and int(alone[:, R, 3].sum()) == 2 * H * W + (H * W - (H - H // 2) * (W - W // 2))
    first = lambda a: torch.from_numpy(np.ascontiguousarray(a[:1])).cuda()
    busy = ops.boundary_counts([first(s) for s in scores], [first(labels)], first(gt), radius=R)
    both = ops.boundary_counts([torch.from_numpy(s).cuda() for s in scores], [torch.from_numpy(labels).cuda()], torch.from_numpy(gt).cuda(),
                               radius=R)
    assert torch.equal(both, busy + alone)                             # the images of a batch do not see each other


def test_boundary_counts_another_ignore_index_and_label_maps_alone(cases):
    from dasac_hip import ops
    B, C, H, W, R = SHAPES[0]
    scores, labels, gt, _ = cases[SHAPES[0]]
    d_labels, d_gt = torch.from_numpy(labels).cuda(), torch.from_numpy(gt).cuda()
    got = ops.boundary_counts([], [d_labels], d_gt, radius=R, ignore_index=3, num_classes=C)     # class 3 is skipped but still a neighbour
    assert np.array_equal(got.cpu().numpy(), BR.boundary_tables([], [labels], gt, C, R, 3))
    table = torch.zeros(1, 3, 5, C, dtype=torch.int64, device="cuda")                            # the table tells C and the radius
    ops.boundary_counts([], [d_labels.to(torch.uint8)], d_gt, table)
    assert np.array_equal(table.cpu().numpy(), BR.boundary_tables([], [labels], gt, C, 2))


def test_boundary_counts_numbers_the_layers_over_the_non_null_slots(cases):
    from dasac_hip import lib as L, ops
    lib = L.load()
    B, C, H, W, R = SHAPES[0]
    scores, labels, gt, want = cases[SHAPES[0]]
    s1, m = torch.from_numpy(scores[1]).cuda(), torch.from_numpy(labels.astype(np.uint8)).cuda()
    d_gt = torch.from_numpy(gt).cuda()
    table = torch.zeros(2, R + 1, 5, C, dtype=torch.int64, device="cuda")
    ws = torch.empty(lib.dasac_boundary_counts_workspace(2, B, H, W), dtype=torch.uint8, device="cuda")
    rc = lib.dasac_boundary_counts(0, 0, s1.data_ptr(), 0, 0, m.data_ptr(), 2, d_gt.data_ptr(), B, C, H, W, R, 255, table.data_ptr(),
                                   ws.data_ptr(), ws.numel(), L.stream_ptr())
    assert rc == 0, lib.dasac_last_error()
    assert np.array_equal(table.cpu().numpy(), want[[1, 3]])            # scores2 is layer 0, labels1 (uint8 by bit 1) is layer 1
    assert torch.equal(table, ops.boundary_counts([s1], [m], d_gt, radius=R))


def test_boundary_counts_refuses_bad_arguments():
    from dasac_hip import lib as L, ops, DasacError
    lib = L.load()
    s = torch.zeros(1, 19, 4, 4, device="cuda")
    big = torch.zeros(1, 65, 4, 4, device="cuda")
    m = torch.zeros(1, 4, 4, dtype=torch.int64, device="cuda")
    out = torch.zeros(2, 17, 5, 65, dtype=torch.int64, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")

    def call(s0=s.data_ptr(), m0=m.data_ptr(), gt=m.data_ptr(), B=1, C=19, H=4, W=4, R=4, table=out.data_ptr(), w=ws.data_ptr(), n=ws.numel()):
        return lib.dasac_boundary_counts(s0, 0, 0, 0, m0, 0, 0, gt, B, C, H, W, R, 255, table, w, n, L.stream_ptr())
    assert call() == 0
    assert call(R=0) == EINVAL and call(R=17) == EINVAL and call(R=-1) == EINVAL
    assert call(R=16) == 0 and call(R=1) == 0
    assert call(s0=big.data_ptr(), C=65) == EINVAL and call(C=0) == EINVAL
    assert call(s0=big.data_ptr(), C=64) == 0
    assert call(s0=0, m0=0) == EINVAL                                   # no layer at all
    assert b"boundary_counts" in lib.dasac_last_error()
    assert call(gt=0) == EINVAL and call(table=0) == EINVAL and call(w=0) == EINVAL
    assert call(B=0) == EINVAL and call(H=0) == EINVAL and call(W=-1) == EINVAL
    assert call(n=lib.dasac_boundary_counts_workspace(2, 1, 4, 4) - 1) == EINVAL               # workspace too small
    assert call(n=lib.dasac_boundary_counts_workspace(2, 1, 4, 4)) == 0
    assert call(w=ws.data_ptr() + 4) == EINVAL and call(gt=m.data_ptr() + 4) == EINVAL
    torch.cuda.synchronize()
    assert int(out.sum()) == 5 * 2 * 3 * 16                             # the five good calls of two layers: tp, pred and both per pixel
    with pytest.raises(DasacError):
        ops.boundary_counts([], [], m)
    with pytest.raises(DasacError):
        ops.boundary_counts([s.cpu()], [], m.cpu())                      # no CPU path
    with pytest.raises(DasacError):
        ops.boundary_counts([s], [], m, radius=0)
    with pytest.raises(DasacError):
        ops.boundary_counts([s], [], m, radius=17)
    with pytest.raises(DasacError):
        ops.boundary_counts([big], [], m)
    with pytest.raises(DasacError):
        ops.boundary_counts([], [m], m)                                  # label maps alone do not tell C
    with pytest.raises(DasacError):
        ops.boundary_counts([s], [m.to(torch.int32)], m)
    with pytest.raises(DasacError):
        ops.boundary_counts([s], [], m, torch.zeros(1, 5, 4, 19, dtype=torch.int64, device="cuda"))


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def net19(g19):
    return _build(g19)


@pytest.mark.parametrize("name", ["src", "tgt"])
def test_validation_with_boundary_tables_end_to_end(g19, net19, name):
    import driver
    R = 4
    kw = dict(step="source" if name == "src" else "target", group_size=int(g19["T"]), max_iter=int(g19["max_iter"]),
              ignore_classes=[9, 14, 16])
    plain = driver.validation(net19, _loader(g19, name), boundary_radius=0, **kw)
    assert plain.boundary == {} and plain.boundary_summary is None
    seen = []

    def keep(module, args, output):
        _, outs = output
        seen.append(({layer: outs[layer].cpu().numpy() for layer in LAYERS[name]}, args[1].view(-1, *args[1].shape[-2:]).cpu().numpy().copy()))
    hook = net19.register_forward_hook(keep)
    try:
        res = driver.validation(net19, _loader(g19, name), boundary_radius=R, **kw)
    finally:
        hook.remove()
    assert len(seen) == int(g19["counted"])
    # every existing field is the one of the run without the option
    assert list(res.counts) == LAYERS[name] and res.losses == plain.losses     # the forward pass is bit-identical from run to run
    assert res.checkpoint_score == plain.checkpoint_score and res.mean == plain.mean
    assert res.confusion == {} and res.reliability == {} and res.consistency == {} and res.consistency_summary is None
    for layer in LAYERS[name]:
        assert torch.equal(res.counts[layer], plain.counts[layer]), layer
        assert all(torch.equal(a, b) for a, b in zip(res.per_class[layer], plain.per_class[layer])), layer
    # the tables of its own layer maps
    assert list(res.boundary) == LAYERS[name]
    for layer in LAYERS[name]:
        want = sum(BR.boundary_table(t[layer] if layer == "teacher_labels" else BR.argmax_first(t[layer]), gt, 19, R) for t, gt in seen)
        got = res.boundary[layer]
        assert got.dtype == torch.int64 and not got.is_cuda and tuple(got.shape) == (R + 1, 5, 19)
        assert np.array_equal(got.numpy(), want), layer
        assert torch.equal(got.sum(0)[:3], res.counts[layer])
        assert int(got[:R].sum()) > 0
    assert sorted(res.boundary_summary[LAYERS[name][0]]) == [1, 2, 4]
    assert len(driver.format_boundary(res.boundary_summary, [str(c) for c in range(19)]).splitlines()) == len(LAYERS[name]) * (1 + 3 + 1 + 19)


def test_validation_iou_appends_the_boundary_table(g19, net19):
    import driver
    batches = [(x.cuda(), y.cuda()) for x, y in _loader(g19, "src")]
    for kw in (dict(scales=(1.0,), flip=True), {}):
        miou, iou = driver.validation_iou(net19 if kw else net19.backbone, batches, **kw)
        miou_b, iou_b, T = driver.validation_iou(net19 if kw else net19.backbone, batches, boundary_radius=3, **kw)
        assert miou_b == miou and torch.equal(iou_b, iou)
        assert T.dtype == torch.int64 and tuple(T.shape) == (4, 5, 19) and not T.is_cuda
        assert torch.equal(driver.summarise_iou(T.sum(0)[:3])[0], iou)
    assert len(driver.validation_iou(net19.backbone, batches, confusion=True, boundary_radius=3)) == 4


@pytest.mark.parametrize("name", ["src", "tgt"])
def test_validation_with_boundary_tables_runs_no_aten_arithmetic_on_tensors(g19, net19, name):
    import driver
    kw = dict(step="source" if name == "src" else "target", group_size=int(g19["T"]), max_iter=0, ignore_classes=[9, 14, 16],
              boundary_radius=4)
    driver.validation(net19, _loader(g19, name), **kw)                                 # first call: caches
    loader = _loader(g19, name)
    with Recorder() as rec:
        res = driver.validation(net19, loader, **kw)
        torch.cuda.synchronize()
    assert res.checkpoint_score > 0 and int(res.boundary["logits_up"].sum()) > 0
    assert not rec.big, sorted(set(rec.big))[:12]
