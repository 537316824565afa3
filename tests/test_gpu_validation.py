"""Reference-form validation on the GPU: the `dasac_mask_counts` kernel on equal inputs (exact), `driver.validation` end to end
against the reference's own `Trainer.validation` (g19: tests/golden/make_goldens_validation.py), two ranks, and no ATen compute.

Bounds.  Counts are integers: exact.  A GPU layer map may differ from the reference's only where the reference-side margin
stored in the fixture is below the project's float contract (1e-3 of the layer's max |value|); NO other pixel may differ.  What
those explained pixels can move a summary by is computed from the counts (`_ratio_bound`), not a constant.  Loss means: 1e-3
relative, the same contract."""
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils._python_dispatch import TorchDispatchMode

from oracle import nets_ref as N
from oracle.step_ref import DEFAULT_CFG

pytestmark = pytest.mark.gpu

SCORE_LAYERS = ["logits_up", "teacher_init", "teacher_refined"]
LAYERS = {"src": ["logits_up"], "tgt": SCORE_LAYERS + ["teacher_labels"]}
IGNORE = {"none": [], "synthia": [9, 14, 16]}
STATE_KW = dict(randomize_bn=True, he_init=True, residual_gain=0.25, aspp_gain=0.2)
EINVAL = -1


def recount(pred, gt, C=19, ignore_index=255):
    """utils/metrics.py:18-39 restated on integer maps: int64 [3,C] = (tp, fp, fn)."""
    pred, gt = np.asarray(pred).astype(np.int64).ravel(), np.asarray(gt).astype(np.int64).ravel()
    keep = gt != ignore_index
    pred, gt = pred[keep], gt[keep]
    hit = pred == gt
    out = np.zeros((3, C), np.int64)
    for c in range(C):
        out[0, c] = np.sum(hit & (gt == c))
        out[1, c] = np.sum(~hit & (pred == c))
        out[2, c] = np.sum(~hit & (gt == c))
    return out


@pytest.fixture(scope="module")
def g19(golden):
    return golden("g19_validation")


def _window(g19, b):
    scores = [torch.from_numpy(g19["win%d_%s" % (b, layer)]).cuda() for layer in SCORE_LAYERS]
    labels = torch.from_numpy(g19["win%d_teacher_labels" % b]).to(torch.int64).cuda()
    gt = torch.from_numpy(g19["win%d_gt" % b]).to(torch.int64).cuda()
    return scores, labels, gt


# ---------------------------------------------------------------------------------------------------------------------
# the kernel on equal inputs
# ---------------------------------------------------------------------------------------------------------------------
def test_mask_counts_equals_the_reference_on_its_own_tensors(g19):
    from dasac_hip import ops
    n_win = int(g19["win"][3])
    counts = None
    single = [None] * 4
    for b in range(n_win):
        scores, labels, gt = _window(g19, b)
        assert (scores[0].shape[-2] * scores[0].shape[-1]) % 4 != 0                  # the tail path is part of this test
        counts = ops.mask_counts(scores, [labels], gt, counts)                       # all four layers, ONE launch, accumulating
        for i in range(3):
            single[i] = ops.mask_counts([scores[i]], [], gt, single[i])             # one layer at a time
        single[3] = ops.mask_counts([], [labels], gt, single[3], num_classes=19)
        for i, layer in enumerate(LAYERS["tgt"]):
            want = torch.from_numpy(g19["win%d_%s_counts" % (b, layer)])
            assert torch.equal(counts[i].cpu(), want), (b, layer)
            assert torch.equal(single[i][0].cpu(), want), (b, layer)
    # scores first, then label maps, whichever slots are used
    scores, labels, gt = _window(g19, 0)
    two = ops.mask_counts([scores[2]], [labels, labels], gt)
    assert torch.equal(two[0].cpu(), torch.from_numpy(g19["win0_teacher_refined_counts"]))
    assert torch.equal(two[1], two[2]) and torch.equal(two[1].cpu(), torch.from_numpy(g19["win0_teacher_labels_counts"]))


def _random_case(B, C, H, W, seed, offset=0):
    """scores / label map / gt with ignore, -1 and label-255 pixels; offset > 0: every tensor starts `offset` ELEMENTS into its
    allocation (a sliced view: base pointer not 16-byte aligned)."""
    g = torch.Generator().manual_seed(seed)

    def place(t):
        flat = torch.empty(t.numel() + offset, dtype=t.dtype, device="cuda")
        view = flat[offset:].view(t.shape)
        view.copy_(t)
        return view
    scores = [torch.randn(B, C, H, W, generator=g) for _ in range(2)]
    scores[1][:, :, : H // 2] = scores[1][:, :1, : H // 2]                            # exact ties: the first maximum must win
    labels = torch.randint(0, C, (B, H, W), generator=g)
    labels[torch.rand(B, H, W, generator=g) < 0.4] = 255
    gt = torch.randint(0, C, (B, H, W), generator=g)
    same = torch.rand(B, H, W, generator=g) < 0.3
    gt[same] = labels[same]                                                         # includes 255 over 255
    gt[torch.rand(B, H, W, generator=g) < 0.1] = 255
    gt[0, 0, : min(W, 5)] = -1
    return scores, labels, gt, [place(s) for s in scores], place(labels), place(gt)


@pytest.mark.parametrize("B,C,H,W,offset", [(2, 19, 7, 9, 0), (1, 19, 1, 3, 0), (3, 19, 129, 257, 0), (2, 19, 23, 31, 1), (2, 19, 16, 16, 3),
                                            (2, 5, 13, 17, 0), (1, 5, 8, 8, 1), (2, 64, 9, 11, 0), (1, 1, 5, 5, 0)])
def test_mask_counts_edge_shapes_match_a_numpy_recount(B, C, H, W, offset):
    from dasac_hip import ops
    scores, labels, gt, d_scores, d_labels, d_gt = _random_case(B, C, H, W, 100 + H, offset)
    if offset:
        assert d_scores[0].data_ptr() % 16 != 0 and d_gt.data_ptr() % 16 != 0 and d_scores[0].is_contiguous()
    got = ops.mask_counts(d_scores, [d_labels], d_gt, num_classes=C)
    again = ops.mask_counts(d_scores, [d_labels], d_gt, num_classes=C)
    assert torch.equal(got, again)                                                  # two runs, the same bits
    for i, s in enumerate(scores):
        assert np.array_equal(got[i].cpu().numpy(), recount(s.argmax(1), gt, C)), i
        assert torch.equal(got[i], ops.iou_counts(d_scores[i], d_gt))              # one score layer == the existing kernel
        assert torch.equal(ops.mask_counts([d_scores[i]], [], d_gt)[0], got[i])
    assert np.array_equal(got[2].cpu().numpy(), recount(labels, gt, C))
    acc = ops.mask_counts(d_scores, [d_labels], d_gt, got.clone(), num_classes=C)   # accumulates into what is there
    assert torch.equal(acc, 2 * got)


def test_mask_counts_special_maps():
    from dasac_hip import ops
    B, C, H, W = 2, 19, 37, 53
    hw = B * H * W
    scores = torch.zeros(B, C, H, W, device="cuda")
    scores[:, 7] = 1.0
    labels = torch.full((B, H, W), 7, dtype=torch.int64, device="cuda")
    gt = torch.full((B, H, W), 7, dtype=torch.int64, device="cuda")
    got = ops.mask_counts([scores], [labels], gt).cpu()                             # uniform maps: every wave merges to one add
    want = torch.zeros(3, C, dtype=torch.int64)
    want[0, 7] = hw
    assert torch.equal(got[0], want) and torch.equal(got[1], want)
    got = ops.mask_counts([scores], [labels], torch.full_like(gt, 3)).cpu()         # uniformly wrong
    want = torch.zeros(3, C, dtype=torch.int64)
    want[1, 7], want[2, 3] = hw, hw
    assert torch.equal(got[0], want) and torch.equal(got[1], want)
    assert int(ops.mask_counts([scores], [labels], torch.full_like(gt, 255)).abs().sum()) == 0        # gt all 255
    # a label of 255 over a labelled ground truth is a false negative only; gt == -1 a false positive only
    got = ops.mask_counts([scores], [torch.full_like(labels, 255)], gt).cpu()
    want = torch.zeros(3, C, dtype=torch.int64)
    want[2, 7] = hw
    assert torch.equal(got[1], want)
    got = ops.mask_counts([scores], [labels], torch.full_like(gt, -1)).cpu()
    want = torch.zeros(3, C, dtype=torch.int64)
    want[1, 7] = hw
    assert torch.equal(got[0], want) and torch.equal(got[1], want)
    assert int(ops.mask_counts([scores], [], gt, ignore_index=7).abs().sum()) == 0                     # another ignore index


def test_mask_counts_refuses_bad_arguments():
    from dasac_hip import lib as L, ops, DasacError
    lib = L.load()
    s = torch.zeros(1, 19, 4, 4, device="cuda")
    m = torch.zeros(1, 4, 4, dtype=torch.int64, device="cuda")
    big = torch.zeros(1, 65, 4, 4, device="cuda")
    counts = torch.zeros(2, 3, 65, dtype=torch.int64, device="cuda")

    def call(s0=s.data_ptr(), m0=m.data_ptr(), gt=m.data_ptr(), B=1, C=19, HW=16, out=counts.data_ptr()):
        return lib.dasac_mask_counts(s0, 0, 0, 0, m0, 0, gt, B, C, HW, 255, out, L.stream_ptr())
    assert call() == 0
    assert call(gt=0) == EINVAL                     # null gt
    assert call(out=0) == EINVAL                    # null counts
    assert call(s0=0, m0=0) == EINVAL               # no layer at all
    assert call(B=0) == EINVAL and call(B=-1) == EINVAL
    assert call(C=0) == EINVAL
    assert call(HW=0) == EINVAL and call(HW=-4) == EINVAL
    assert call(s0=big.data_ptr(), C=65) == EINVAL  # C > 64
    assert call(s0=big.data_ptr(), C=64) == 0
    assert b"mask_counts" in lib.dasac_last_error()
    torch.cuda.synchronize()
    with pytest.raises(DasacError):
        ops.mask_counts([], [], m)
    with pytest.raises(DasacError):
        ops.mask_counts([s.cpu()], [], m.cpu())     # no CPU path
    with pytest.raises(DasacError):
        ops.mask_counts([s], [m.to(torch.int32)], m)


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def _build(g19):
    import models
    cfg = NS(**dict(DEFAULT_CFG, INIT_MODEL="", OPT_NESTEROV=False))
    net = models.get_model(cfg, 0, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    net.backbone.load_state_dict(N.resnet101_state(seed=int(g19["student_seed"]), **STATE_KW), strict=True)
    net.slow_net.load_state_dict(N.resnet101_state(seed=int(g19["teacher_seed"]), **STATE_KW), strict=True)
    net.slow_init[0] = True
    net.running_conf.copy_(torch.from_numpy(g19["running_conf"]))
    return net.cuda().train()


def _loader(g19, name, order=None):
    """The fixture's loader: 4 batches, the 4th a repeat of the 1st (max_iter = 1 counts 3 of them)."""
    counted, n, t = int(g19["counted"]), int(g19["N"]), int(g19["T"])
    out = []
    for b in (range(int(g19["num_batches"])) if order is None else order):
        b %= counted
        if name == "src":
            out.append((torch.from_numpy(g19["src%d_x" % b]), torch.from_numpy(g19["src%d_y" % b]).to(torch.int64)))
        else:
            ts = (g19["tgt%d_f1" % b], g19["tgt%d_gt" % b].astype(np.int64), g19["tgt%d_f2" % b], g19["affine"], g19["affine_inv"])
            out.append(tuple(torch.from_numpy(np.ascontiguousarray(a)).view(n, t, *a.shape[1:]) for a in ts))
    return out


def _ratio_bound(num, den, moved):
    """|num'/den' - num/den| when `moved` pixels change sides: num and den each move by at most `moved`, the ratio stays in
    [0, 1]:  <= moved/den' + (num/den) * moved/den' <= 2 * moved / (den - moved)."""
    den, moved = den.astype(np.float64), moved.astype(np.float64)
    return np.where(moved == 0, 0.0, np.where(den - moved > 0, np.minimum(1.0, 2 * moved / np.maximum(den - moved, 1e-3)), 1.0))


@pytest.mark.parametrize("name", ["src", "tgt"])
def test_validation_end_to_end_matches_the_reference(g19, name):
    import driver
    net = _build(g19)
    seen = []

    def keep(module, args, output):
        _, outs = output
        maps = {layer: (outs[layer] if layer == "teacher_labels" else outs[layer].argmax(1)).cpu().numpy() for layer in LAYERS[name]}
        seen.append((maps, args[1].view(-1, *args[1].shape[-2:]).cpu().numpy().copy()))
    chi, teacher = net.running_conf.clone(), net.slow_net.state_dict()["model.conv1.weight"].clone()
    results = {}
    for tag, ignore in IGNORE.items():
        del seen[:]
        hook = net.register_forward_hook(keep)
        try:
            res = driver.validation(net, _loader(g19, name), step="source" if name == "src" else "target", group_size=int(g19["T"]),
                                    max_iter=int(g19["max_iter"]), ignore_classes=ignore)
        finally:
            hook.remove()
        results[tag] = res
        assert net.training and net.backbone.training                               # the previous mode is back
        assert torch.equal(net.running_conf, chi) and torch.equal(net.slow_net.state_dict()["model.conv1.weight"], teacher)
        assert len(seen) == int(g19["counted"])                                     # max_iter + 2 batches
        assert list(res.counts) == LAYERS[name]

        # losses: 1e-3 relative
        assert sorted(res.losses) == sorted(g19[name + "_loss_keys"])
        for key, val in res.losses.items():
            want = float(g19["%s_loss_%s" % (name, key)])
            print(name, tag, "loss", key, val, want)
            assert abs(val - want) <= 1e-3 * abs(want), (key, val, want)

        contract = float(g19["contract"])
        score_bound = 0.0
        for layer in LAYERS[name]:
            own = sum(recount(maps[layer], gt) for maps, gt in seen)
            assert np.array_equal(res.counts[layer].numpy(), own), layer              # exactly its own layer maps' counts
            moved = np.zeros(19, np.int64)
            for b, (maps, gt) in enumerate(seen):
                assert np.array_equal(gt, g19["%s%d_gt_seen" % (name, b)])             # -1 rewritten to 255 by the forward pass
                ref = g19["%s%d_%s_map" % (name, b, layer)].astype(np.int64)
                diff = maps[layer] != ref
                margin = g19["%s%d_%s_margin" % (name, b, layer)].astype(np.float32)
                unexplained = diff & ~(margin < contract)
                print(name, tag, layer, "batch", b, "differing pixels", int(diff.sum()), "unexplained", int(unexplained.sum()))
                assert not unexplained.any(), (layer, b, int(unexplained.sum()))
                live = diff & (gt != 255)
                for c in range(19):                                                  # pixels that can move a count of class c
                    moved[c] += int(np.sum(live & ((maps[layer] == c) | (ref == c) | (gt == c))))
            tp, fp, fn = (g19["%s_%s_counts" % (name, layer)][i] for i in range(3))
            keep_c = [c for c in range(19) if c not in ignore]
            bounds = [_ratio_bound(tp, den, moved)[keep_c].mean() + 1e-6 for den in (tp + fp + fn, tp + fp, tp + fn)]
            want = g19["%s_%s_mean_%s" % (name, layer, tag)]
            for got, w, bound in zip(res.mean[layer], want, bounds):
                print(name, tag, layer, "mean", got, w, "bound", bound)
                assert abs(got - w) <= bound, (layer, got, w, bound)
            score_bound = max(score_bound, bounds[0])
            np.testing.assert_allclose(torch.stack(res.per_class[layer]).numpy(),
                                       torch.stack(driver.summarise_iou(res.counts[layer])).numpy(), rtol=0, atol=0)
        want = float(g19["%s_score_%s" % (name, tag)])
        print(name, tag, "score", res.checkpoint_score, want, "bound", score_bound)
        assert abs(res.checkpoint_score - want) <= score_bound
        assert res.checkpoint_score == max(m[0] for m in res.mean.values())
    for layer in LAYERS[name]:                                                       # the ignore list changes the means only
        assert torch.equal(results["none"].counts[layer], results["synthia"].counts[layer])
    assert results["none"].checkpoint_score != results["synthia"].checkpoint_score


def test_validation_baseline_batches_through_the_source_step(g19):
    """A baseline net validates its target set with the source step on (image, gt) batches (train.py:113-115)."""
    import driver
    net = _build(g19).backbone
    res = driver.validation(net, _loader(g19, "src"), step="source", max_iter=None)
    assert list(res.counts) == ["logits_up"] and list(res.losses) == ["loss_ce"]
    assert int(res.counts["logits_up"].sum()) > int(torch.from_numpy(g19["src_logits_up_counts"]).sum())      # all 4 batches


# ---------------------------------------------------------------------------------------------------------------------
# two ranks on one device
# ---------------------------------------------------------------------------------------------------------------------
def _validation_rank(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "da-sac_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    from conftest import init_ranks, GOLDEN
    init_ranks(rank, world)
    import driver
    g19 = np.load(os.path.join(GOLDEN, "g19_validation.npz"), allow_pickle=False)
    net = _build(g19)
    res = driver.validation(net, _loader(g19, "tgt", order=[2 * rank, 2 * rank + 1]), step="target", group_size=int(g19["T"]),
                            ignore_classes=[9, 14, 16])
    torch.cuda.synchronize()
    q.put((rank, {k: v.numpy() for k, v in res.counts.items()}, res.checkpoint_score, res.losses))
    dist.barrier()
    dist.destroy_process_group()


def test_validation_two_ranks_sum_their_counts(g19):
    import driver
    from conftest import run_ranks
    got = run_ranks(_validation_rank, 2, lambda r, port, q: (r, 2, port, q), timeout=420)
    one = driver.validation(_build(g19), _loader(g19, "tgt", order=[0, 1, 2, 3]), step="target", group_size=int(g19["T"]),
                            ignore_classes=[9, 14, 16])
    for rank, counts, score, losses in got:
        for layer in LAYERS["tgt"]:
            assert np.array_equal(counts[layer], one.counts[layer].numpy()), (rank, layer)        # summed over ranks, exactly
        assert score == one.checkpoint_score                                                      # the same on every rank
    assert got[0][3] == got[1][3]                                                                 # target losses: mean over ranks
    for key, val in one.losses.items():
        assert got[0][3][key] == pytest.approx(val, rel=1e-5), key


# ---------------------------------------------------------------------------------------------------------------------
# no ATen compute (the checker of test_gpu_no_aten_compute.py)
# ---------------------------------------------------------------------------------------------------------------------
PLUMBING = {"empty", "empty_like", "empty_strided", "new_empty", "new_empty_strided", "zeros", "zeros_like", "ones", "full", "zero_", "fill_",
            "view", "_unsafe_view", "reshape", "as_strided", "narrow", "slice", "select", "expand", "permute", "transpose", "t", "squeeze",
            "unsqueeze", "flatten", "unflatten", "detach", "detach_", "alias", "clone", "contiguous", "copy_", "_to_copy", "to", "cat",
            "lift_fresh", "_local_scalar_dense", "item", "is_pinned", "_pin_memory", "pin_memory", "record_stream", "set_", "resize_",
            "scalar_tensor", "result_type", "_has_compatible_shallow_copy_type", "is_same_size", "equal", "unbind", "split", "chunk", "stack"}
SMALL = 64          # per-class vectors (19 x 3), losses: arithmetic on these is bookkeeping


class Recorder(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.big = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        name = func.overloadpacket.__name__ if hasattr(func, "overloadpacket") else str(func)
        if name not in PLUMBING:
            sizes = [t.numel() for t in torch.utils._pytree.tree_leaves((args, kwargs, out)) if isinstance(t, torch.Tensor)]
            if sizes and max(sizes) > SMALL:
                self.big.append((name, max(sizes)))
        return out


@pytest.mark.parametrize("name", ["src", "tgt"])
def test_validation_runs_no_aten_arithmetic_on_tensors(g19, name):
    import driver
    net = _build(g19)
    kw = dict(step="source" if name == "src" else "target", group_size=int(g19["T"]), max_iter=0, ignore_classes=[9, 14, 16])
    driver.validation(net, _loader(g19, name), **kw)                                 # first call: caches
    loader = _loader(g19, name)
    with Recorder() as rec:
        res = driver.validation(net, loader, **kw)
        torch.cuda.synchronize()
    assert res.checkpoint_score > 0
    assert not rec.big, sorted(set(rec.big))[:12]
