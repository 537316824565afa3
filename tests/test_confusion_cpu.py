"""Confusion matrices and reliability tables of the validation pass -- the parts that need no GPU: the host summaries of
driver.py on matrices worked out by hand, the identity between a confusion matrix and the (tp, fp, fn) counts of the suite's
`recount`, and `driver.validation`'s summing of the joint tables over two gloo ranks (the kernel replaced by the numpy
definitions below, which tests/test_gpu_confusion.py also holds the kernel to)."""
import os
import socket

import numpy as np
import pytest
import torch

from test_validation_cpu import recount


# ---------------------------------------------------------------------------------------------------------------------
# the definitions, restated in numpy
# ---------------------------------------------------------------------------------------------------------------------
def confusion_ref(pred, gt, C, ignore_index=255):
    """int64 [C+1,C+1]: row = ground truth, column = prediction, a value outside [0, C) is index C; gt == ignore_index is skipped."""
    pred, gt = np.asarray(pred).astype(np.int64).ravel(), np.asarray(gt).astype(np.int64).ravel()
    keep = gt != ignore_index
    pred, gt = pred[keep], gt[keep]
    row = np.where((gt >= 0) & (gt < C), gt, C)
    col = np.where((pred >= 0) & (pred < C), pred, C)
    return np.bincount(row * (C + 1) + col, minlength=(C + 1) ** 2).reshape(C + 1, C + 1)


def argmax_first(scores):
    """(class, value) of the FIRST maximum over axis 1 under a strict `>` scan from class 0 (a NaN wins only as class 0)."""
    scores = np.asarray(scores)
    best, arg = scores[:, 0].copy(), np.zeros(scores[:, 0].shape, np.int64)
    for c in range(1, scores.shape[1]):
        better = scores[:, c] > best
        best, arg = np.where(better, scores[:, c], best), np.where(better, c, arg)
    return arg, best


def bin_of(v, n_bins, dtype=np.float32):
    """b = !(v > 0) ? 0 : min(n_bins - 1, (int)(v * n_bins)) with the multiply in `dtype`."""
    v = np.asarray(v, dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.minimum(np.nan_to_num(v * dtype(n_bins), nan=0.0, posinf=float(n_bins)), dtype(n_bins))
        return np.where(v > 0, np.minimum(n_bins - 1, t.astype(np.int64)), 0)


def softmax_max64(scores):
    """1 / sum_c exp(x_c - max_c x) in float64: the soft-max maximum."""
    x = np.asarray(scores, np.float64)
    return 1.0 / np.exp(x - x.max(1, keepdims=True)).sum(1)


def reliability_ref(arg, bins, gt, C, n_bins, ignore_index=255):
    """int64 [C,n_bins,2] from per-pixel arg-max classes and confidence bins."""
    arg, bins, gt = np.asarray(arg).ravel(), np.asarray(bins).ravel(), np.asarray(gt).astype(np.int64).ravel()
    keep = gt != ignore_index
    key = (arg[keep] * n_bins + bins[keep]) * 2 + (arg[keep] == gt[keep])
    return np.bincount(key, minlength=C * n_bins * 2).reshape(C, n_bins, 2)


def random_maps(C, seed, shape=(2, 23, 31)):
    """a label map and a ground truth with 255, -1, C, 300 and 255-over-255 pixels (the cases of the issue's identity check)."""
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, C, shape, generator=g)
    labels[torch.rand(shape, generator=g) < .4] = 255
    labels[1, 0, :4], labels[1, 1, :4] = -1, 300
    gt = torch.randint(0, C, shape, generator=g)
    same = torch.rand(shape, generator=g) < .3
    gt[same] = labels[same]
    gt[torch.rand(shape, generator=g) < .1] = 255
    gt[0, 0, :5], gt[1, 0, :2], gt[1, 1, :2], gt[1, 2, :3] = -1, -1, 300, C
    return labels.numpy(), gt.numpy()


M3 = torch.tensor([[5, 1, 0, 2],        # gt 0: 5 right, 1 taken for class 1, 2 without a label
                   [0, 3, 3, 0],        # gt 1: half of it taken for class 2
                   [0, 0, 0, 0],        # class 2 never occurs
                   [1, 0, 2, 4]])       # gt outside the classes


# ---------------------------------------------------------------------------------------------------------------------
# counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,ignore_index", [(19, 255), (5, 255), (64, 255), (19, 7)])
def test_counts_from_confusion_agree_with_the_suites_recount(C, ignore_index):
    import driver
    labels, gt = random_maps(C, C + ignore_index)
    M = confusion_ref(labels, gt, C, ignore_index)
    assert M.sum() == int((gt != ignore_index).sum())
    assert M[C].sum() > 0 and M[:, C].sum() > 0 and (ignore_index != 255 or M[C, C] > 0)
    got = driver.counts_from_confusion(torch.from_numpy(M))
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), recount(labels, gt, C, ignore_index))
    both = driver.counts_from_confusion(torch.from_numpy(np.stack([M, 2 * M])))          # leading layer dimensions are kept
    assert torch.equal(both[0], got) and torch.equal(both[1], 2 * got)


def test_counts_and_iou_summary_of_a_matrix_worked_out_by_hand():
    import driver
    counts = driver.counts_from_confusion(M3)
    assert counts.tolist() == [[5, 3, 0], [1, 1, 5], [3, 3, 0]]
    iou, precision, recall = driver.summarise_iou(counts)
    f = lambda a, b: np.float32(a) / np.maximum(np.float32(1e-3), np.float32(b))
    assert iou.tolist() == [f(5, 9), f(3, 7), f(0, 5)]
    assert precision.tolist() == [f(5, 6), f(3, 4), f(0, 5)] and recall.tolist() == [f(5, 8), f(3, 6), 0.0]


# ---------------------------------------------------------------------------------------------------------------------
# summaries
# ---------------------------------------------------------------------------------------------------------------------
def test_summarise_confusion_by_hand():
    import driver
    s = driver.summarise_confusion(M3, top=3)
    assert s.by_gt.dtype == torch.float64 and s.by_pred.dtype == torch.float64
    assert s.by_gt.tolist() == [[5 / 8, 1 / 8, 0, 2 / 8], [0, .5, .5, 0], [0, 0, 0, 0], [1 / 7, 0, 2 / 7, 4 / 7]]      # a zero row stays zero
    assert s.by_pred[:, 2].tolist() == [0, 3 / 5, 0, 2 / 5] and s.by_pred[:, 0].tolist() == [5 / 6, 0, 0, 1 / 6]
    assert s.pixel_accuracy == pytest.approx(8 / 14, abs=1e-15)
    assert s.fw_iou == pytest.approx(8 / 14 * 5 / 9 + 6 / 14 * 3 / 7, abs=1e-15)
    assert s.top == [(1, 2, 3, .5), (0, 3, 2, .25), (3, 2, 2, 2 / 7)]                     # largest first, ties by (gt, pred)
    assert [t[:3] for t in driver.summarise_confusion(M3).top] == [(1, 2, 3), (0, 3, 2), (3, 2, 2), (0, 1, 1), (3, 0, 1)]
    assert driver.summarise_confusion(M3, top=0).top == []
    zero = driver.summarise_confusion(torch.zeros(4, 4, dtype=torch.int64))
    assert zero.pixel_accuracy == 0.0 and zero.fw_iou == 0.0 and zero.top == [] and float(zero.by_gt.abs().sum()) == 0.0


def test_summarise_confusion_honours_ignore_classes():
    import driver
    s = driver.summarise_confusion(M3, ignore_classes=[1])
    assert s.pixel_accuracy == pytest.approx(5 / 8, abs=1e-15)
    assert s.fw_iou == pytest.approx(5 / 9, abs=1e-15)                                    # class 0 holds every kept pixel
    assert [t[:3] for t in s.top] == [(0, 3, 2), (3, 2, 2), (3, 0, 1)]                    # no row or column of class 1
    assert torch.equal(s.by_gt, driver.summarise_confusion(M3).by_gt)                     # the matrices keep every class


def test_pseudo_label_audit_by_hand():
    import driver
    labels = torch.tensor([[6, 1, 3],       # gt 0, 10 pixels: 7 received a label, 6 of them the right one
                           [2, 2, 4],       # gt 1, 8 pixels: 4 received a label
                           [1, 0, 1]])      # gt outside the classes
    teacher = torch.tensor([[8, 2, 0], [3, 5, 0], [1, 1, 0]])
    a = driver.pseudo_label_audit(labels, teacher)
    assert a.coverage.tolist() == [7 / 10, 4 / 8] and a.precision.tolist() == [6 / 9, 2 / 3]
    assert a.teacher_recall.tolist() == [8 / 10, 5 / 8] and a.teacher_precision.tolist() == [8 / 12, 5 / 8]
    empty = driver.pseudo_label_audit(torch.zeros(3, 3, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int64))
    assert empty.coverage.tolist() == [0, 0] and empty.teacher_precision.tolist() == [0, 0]


def test_summarise_reliability_two_bins_by_hand():
    import driver
    table = torch.tensor([[[1, 1], [2, 6]],      # class 0: bin [0, .5): 1 of 2 right; bin [.5, 1]: 6 of 8
                          [[4, 0], [0, 0]]])     # class 1: 4 pixels, all wrong, all in the low bin
    r = driver.summarise_reliability(table)
    assert r.pixels.tolist() == [[2, 8], [4, 0]] and r.accuracy.tolist() == [[.5, .75], [0, 0]]
    # midpoints .25 and .75: class 0 = 2/10 * |.5 - .25| + 8/10 * 0, class 1 = |0 - .25|
    assert r.ece.tolist() == pytest.approx([.05, .25], abs=1e-15)
    assert r.overall_pixels.tolist() == [6, 8] and r.overall_accuracy.tolist() == pytest.approx([1 / 6, .75], abs=1e-15)
    assert r.overall_ece == pytest.approx(6 / 14 * (.25 - 1 / 6), abs=1e-15)
    assert "approximation" in driver.summarise_reliability.__doc__
    assert driver.summarise_reliability(torch.zeros(2, 4, 2, dtype=torch.int64)).overall_ece == 0.0


def test_format_confusion_is_a_fixed_width_table():
    import driver
    big = M3.clone()
    big[1, 2] = 123456789
    text = driver.format_confusion(big, ["road", "sidewalk", "bus"])
    lines = text.split("\n")
    assert len(lines) == 5 and len(set(len(l) for l in lines)) == 1
    assert lines[0].split()[-4:] == ["road", "sidewalk", "bus", "none"] and lines[2].split() == ["sidewalk", "0", "3", "123456789", "0"]
    assert lines[4].split() == ["none", "1", "0", "2", "4"]
    with pytest.raises(AssertionError):
        driver.format_confusion(M3, ["road"])


# ---------------------------------------------------------------------------------------------------------------------
# two gloo ranks: driver.validation sums the HOST tables (the kernel replaced by the definitions above)
# ---------------------------------------------------------------------------------------------------------------------
C2, BINS2 = 5, 4


def _numpy_confusion_counts(scores, label_maps, gt, confusion=None, reliability=None, bins=0, logits_layers=(), ignore_index=255,
                            num_classes=None):
    """ops.confusion_counts on host tensors, from the numpy definitions: accumulates into the given tensors."""
    C = scores[0].shape[1]
    g = gt.numpy()
    for l, s in enumerate(scores):
        arg, best = argmax_first(s.numpy())
        confusion[l] += torch.from_numpy(confusion_ref(arg, g, C, ignore_index))
        if reliability is not None:
            v = softmax_max64(s.numpy()).astype(np.float32) if l in logits_layers else best
            reliability[l] += torch.from_numpy(reliability_ref(arg, bin_of(v, reliability.shape[2]), g, C, reliability.shape[2], ignore_index))
    for l, m in enumerate(label_maps):
        confusion[len(scores) + l] += torch.from_numpy(confusion_ref(m.numpy(), g, C, ignore_index))
    return confusion, reliability


def _rank_batches(rank):
    g = torch.Generator().manual_seed(40 + rank)
    out = []
    for _ in range(2):
        gt = torch.randint(0, C2, (2, 6, 7), generator=g)
        gt[0, 0, :3], gt[1, 0, :2] = 255, -1
        out.append((torch.randn(2, C2, 6, 7, generator=g), gt))
    return out


class _Net(torch.nn.Module):
    """`net(image, gt)` of the source step: the 'image' is the logits; the label layer rejects the pixels below 0.5."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))

    def forward(self, image, gt):
        probs = torch.softmax(image, 1)
        labels = torch.where(probs.max(1)[0] < 0.5, torch.full_like(gt, 255), probs.argmax(1))
        return {"loss_ce": image.mean().reshape(1)}, {"logits_up": image, "teacher_refined": probs, "teacher_labels": labels}


def _expected(batches):
    conf = {k: np.zeros((C2 + 1, C2 + 1), np.int64) for k in ("logits_up", "teacher_refined", "teacher_labels")}
    rel = {k: np.zeros((C2, BINS2, 2), np.int64) for k in ("logits_up", "teacher_refined")}
    net = _Net()
    for image, gt in batches:
        _, outs = net(image, gt)
        for k in conf:
            pred = outs[k].numpy() if k == "teacher_labels" else argmax_first(outs[k].numpy())[0]
            conf[k] += confusion_ref(pred, gt.numpy(), C2)
        for k in rel:
            arg, best = argmax_first(outs[k].numpy())
            v = softmax_max64(outs[k].numpy()).astype(np.float32) if k == "logits_up" else best
            rel[k] += reliability_ref(arg, bin_of(v, BINS2), gt.numpy(), C2, BINS2)
    return conf, rel


def _validation_rank(rank, world, port, q):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "da-sac_amd"), os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import driver
    from dasac_hip import ops
    ops.confusion_counts = _numpy_confusion_counts
    res = driver.validation(_Net(), _rank_batches(rank), step="source", num_classes=C2, confusion=True, reliability_bins=BINS2)
    q.put((rank, {k: v.numpy() for k, v in res.confusion.items()}, {k: v.numpy() for k, v in res.reliability.items()},
           {k: v.numpy() for k, v in res.counts.items()}))
    dist.barrier()
    dist.destroy_process_group()


def test_validation_sums_the_joint_tables_over_two_gloo_ranks():
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_validation_rank, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=180) for _ in procs), key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    conf, rel = _expected(_rank_batches(0) + _rank_batches(1))
    assert any(int(m[C2].sum()) > 0 for m in conf.values()) and int(conf["teacher_labels"][:, C2].sum()) > 0
    for rank, got_conf, got_rel, got_counts in got:
        assert list(got_conf) == ["logits_up", "teacher_refined", "teacher_labels"] and list(got_rel) == ["logits_up", "teacher_refined"]
        for k in conf:
            assert np.array_equal(got_conf[k], conf[k]), (rank, k)                        # both ranks' pixels, on every rank
            M = conf[k]
            tp = np.diag(M)[:C2]
            assert np.array_equal(got_counts[k], np.stack([tp, M[:, :C2].sum(0) - tp, M[:C2].sum(1) - tp])), (rank, k)
        for k in rel:
            assert np.array_equal(got_rel[k], rel[k]), (rank, k)
