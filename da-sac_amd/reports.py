"""Host-side readers and text renderers of the small tables the device passes of driver.py produce: IoU and validation summaries,
confusion and reliability tables, boundary tables, view consistency, gradient health, activation health, domain gap and
class-conditional features.  Pure arithmetic and string formatting on the host: no network, no kernels.  driver.py re-exports
every public name, and `driver.<name>` is how callers reach them.  The readers of the segment tables live in segment_reports.py
and are part of this module's surface too."""
import math
from types import SimpleNamespace

import numpy as np
import torch

from segment_reports import format_segments, summarise_segments  # noqa: F401  (the readers of the segment tables: part of this surface)


def _ratio(num, den):
    """num / den in float64 with 0 where den is not above 0: python numbers, numpy arrays (broadcasting) or torch tensors (float64
    tensor out)."""
    if isinstance(num, torch.Tensor):
        return torch.as_tensor(_ratio(num.numpy(), den.numpy()), dtype=torch.float64)
    if np.ndim(num) == 0 and np.ndim(den) == 0:
        return num / den if den > 0 else 0.0
    return np.where(den > 0, num / np.where(den > 0, den, 1), 0.0)


def _largest_entries(M, ignore, top, upper=False):
    """The `top` largest positive off-diagonal entries [(value, r, c)] of a square matrix (`upper`: of its upper triangle), rows and
    columns in `ignore` left out: largest first, ties by (r, c)."""
    n = M.shape[0]
    entries = [(int(M[r, c]), r, c) for r in range(n) for c in range(r + 1 if upper else 0, n)
               if r != c and r not in ignore and c not in ignore and int(M[r, c]) > 0]
    return sorted(entries, key=lambda t: (-t[0], t[1], t[2]))[:top]


def _by_key(rows, key):
    """The indices of `rows` (dicts) by `key`, largest first, ties in order."""
    return sorted(range(len(rows)), key=lambda i: (-rows[i][key], i))


def _top_then_flagged(rows, key, top):
    """The `top` rows by `key`, then every row with non-finite entries that is not among them, in order."""
    first = _by_key(rows, key)[:top]
    return [rows[i] for i in first + [i for i, row in enumerate(rows) if row["nonfinite"] and i not in first]]


def _table(corner, cols, width, names, cells):
    """The lines of a fixed-width table: a left-justified head column under `corner`, as wide as the longest name, then the cells
    right-justified to `width`; cells beyond `width` follow unpadded."""
    head = max([len(corner)] + [len(n) for n in names])
    return [" ".join([n.ljust(head)] + [c.rjust(w) for c, w in zip(row, width)] + list(row[len(width):]))
            for n, row in zip([corner] + list(names), [cols] + list(cells))]


def summarise_iou(counts):
    """`Jaccard.summarise` (utils/metrics.py:40-53) on int64 counts [3, C] = (tp, fp, fn): per-class
    (jaccard, precision, recall) = tp / max(1e-3, .) in float32 like the reference (a class that never occurs scores 0)."""
    tp, fp, fn = (counts[i].to(torch.float32).cpu() for i in range(3))
    floor = torch.tensor(1e-3)
    return tp / torch.maximum(floor, fn + fp + tp), tp / torch.maximum(floor, tp + fp), tp / torch.maximum(floor, tp + fn)


def counts_from_confusion(matrix):
    """(tp, fp, fn) of a confusion matrix int64 [C+1,C+1] (row = ground truth, column = prediction, index C = no class; leading
    layer dimensions are kept): tp[c] = M[c][c], fp[c] = sum_r M[r][c] - M[c][c], fn[c] = sum_k M[c][k] - M[c][c] for c < C -- int64
    [..., 3, C] on the host, the integers ops.mask_counts counts (integer bookkeeping on a small host table)."""
    M = matrix.detach().cpu().numpy()
    C = M.shape[-1] - 1
    tp = np.diagonal(M, axis1=-2, axis2=-1)[..., :C]
    return torch.from_numpy(np.stack([tp, M[..., :, :C].sum(-2) - tp, M[..., :C, :].sum(-1) - tp], -2).astype(np.int64))


def summarise_confusion(matrix, ignore_classes=(), top=10):
    """Reading of one confusion matrix int64 [C+1,C+1] (host or device; the result is on the host).  Returns a namespace:
      by_gt, by_pred   the matrix divided by its ground-truth row sums / prediction column sums, float64; a zero row (column) stays 0;
      pixel_accuracy   correct pixels over the pixels whose ground truth is a class (a prediction of "no class" is wrong);
      fw_iou           sum_c freq_c * IoU_c with freq_c the class's share of those pixels and IoU_c = tp / (tp + fp + fn);
      top              the `top` largest off-diagonal entries [(gt, pred, pixels, share of the gt row)], largest first, ties by
                       (gt, pred); index C stands for "no class".
    Classes in `ignore_classes` leave the accuracy, the frequencies of fw_iou and, as row or column, the top list; every class's
    IoU is still computed on the whole matrix, as the class-subset means of `validation` are."""
    M = matrix.detach().cpu().to(torch.int64)
    C = M.shape[0] - 1
    rows, cols = M.sum(1), M.sum(0)
    by_gt, by_pred = _ratio(M, rows[:, None]), _ratio(M, cols[None, :])
    ignore = set(int(i) for i in ignore_classes)
    keep = torch.tensor([c for c in range(C) if c not in ignore], dtype=torch.int64)
    tp, fp, fn = counts_from_confusion(M)
    labelled = rows[keep].sum()
    accuracy = float(_ratio(tp[keep].sum(), labelled))
    fw_iou = float((_ratio(rows[keep], labelled) * _ratio(tp, tp + fp + fn)[keep]).sum())
    worst = [(r, c, n, float(by_gt[r, c])) for n, r, c in _largest_entries(M, ignore, top)]
    return SimpleNamespace(by_gt=by_gt, by_pred=by_pred, pixel_accuracy=accuracy, fw_iou=fw_iou, top=worst)


def pseudo_label_audit(labels_matrix, teacher_matrix):
    """What the pseudo-label thresholds do per class, from the confusion matrices of `teacher_labels` (the thresholded label map,
    255 = rejected = column C) and `teacher_refined` (the same teacher before thresholding).  float64 [C] each, 0 where a class has
    no pixel:
      coverage           share of the class's ground-truth pixels that received any label: 1 - M[c][C] / sum_k M[c][k];
      precision          of the pixels labelled c, the share whose ground truth is c: M[c][c] / sum_r M[r][c];
      teacher_recall     M_t[c][c] / sum_k M_t[c][k] of the unthresholded teacher;
      teacher_precision  M_t[c][c] / sum_r M_t[r][c]."""
    Ml, Mt = labels_matrix.detach().cpu().to(torch.int64), teacher_matrix.detach().cpu().to(torch.int64)
    C = Ml.shape[0] - 1
    rows = Ml[:C].sum(1)
    return SimpleNamespace(coverage=_ratio(rows - Ml[:C, C], rows), precision=_ratio(torch.diagonal(Ml)[:C], Ml[:, :C].sum(0)),
                           teacher_recall=_ratio(torch.diagonal(Mt)[:C], Mt[:C].sum(1)),
                           teacher_precision=_ratio(torch.diagonal(Mt)[:C], Mt[:, :C].sum(0)))


def summarise_reliability(table):
    """Reading of one reliability table int64 [C,n_bins,2] (arg-max class, confidence bin, miss / hit).  Returns a namespace with,
    per class, pixels int64 [C,n_bins], accuracy float64 [C,n_bins] (hits / pixels, 0 for an empty bin) and ece float64 [C]; and over
    all classes overall_pixels [n_bins], overall_accuracy [n_bins], overall_ece (float).  The expected calibration error is
    sum_b pixels_b / pixels * |accuracy_b - (b + 0.5) / n_bins|: it takes the bin MIDPOINT for the bin's confidence, because the table
    keeps no sum of confidences -- an approximation, off by up to half a bin width (0.5 / n_bins) from the usual definition."""
    R = table.detach().cpu().to(torch.int64)
    n_bins = R.shape[1]
    mid = (torch.arange(n_bins, dtype=torch.float64) + 0.5) / n_bins

    def read(hit, pixels):
        acc = _ratio(hit, pixels)
        return acc, (_ratio(pixels, pixels.sum(-1, keepdim=True)) * (acc - mid).abs()).sum(-1)
    pixels = R.sum(-1)
    acc, ece = read(R[..., 1], pixels)
    all_acc, all_ece = read(R[..., 1].sum(0), pixels.sum(0))
    return SimpleNamespace(pixels=pixels, accuracy=acc, ece=ece, overall_pixels=pixels.sum(0), overall_accuracy=all_acc,
                           overall_ece=float(all_ece))


def format_confusion(matrix, names):
    """Fixed-width text table of a confusion matrix int64 [C+1,C+1] for the log: one row per ground-truth class (`names`, C of them,
    then "none"), one column per prediction, pixel counts."""
    M = matrix.detach().cpu().to(torch.int64)
    names = [str(n) for n in names] + ["none"]
    assert len(names) == M.shape[0] == M.shape[1], (len(names), tuple(M.shape))
    width = max(6, len(str(int(M.max()))))
    return "\n".join(_table("gt \\ pred", [n[:width] for n in names], [width] * len(names), names,
                            [[str(v) for v in row] for row in M.tolist()]))


def summarise_boundary(tables, ignore_classes=(), radii=(1, 2, 4, 8)):
    """Reading of boundary tables (`validation(..., boundary_radius=R).boundary`: {layer: int64 [R+1,5,C]}, host or device; include/
    dasac_hip.h: dasac_boundary_counts).  Slot s < R of a table holds the pixels at Chebyshev distance s + 1 from a class contour, slot
    R everything further; the rows are tp, fp, fn (by the pixel's distance in the ground truth), pred (by its distance in the predicted
    map) and both.  Returns {layer: {r: dict}} for every r of `radii` (a radius above R is a ValueError), each dict with
      band_iou, band_miou            per-class IoU float32 [C] of the pixels within r of a ground-truth contour (the trimap band:
                                     slots < r of tp, fp, fn), and its mean over the classes not in `ignore_classes`;
      interior_iou, interior_miou    the same of all other pixels (slots >= r);
      boundary_iou, boundary_miou    Boundary IoU (Cheng et al., 2021): I / (G + P - I) with G = sum (tp + fn), P = sum pred, I = sum both
                                     over the slots < r -- the band inside the ground-truth mask against the band inside the predicted one;
      error_share                    of all fp + fn of the classes not ignored, the share inside the band (0 without any error);
      pixel_share                    of the pixels whose ground truth is such a class, the share inside the band.
    Ratios follow summarise_iou: float32, numerator / max(1e-3, denominator), so a class without a pixel scores 0; means are
    class_subset_mean; the two shares are python floats."""
    radii = [int(r) for r in radii]
    ignore = set(int(i) for i in ignore_classes)
    floor = torch.tensor(1e-3)
    out = {}
    for layer, table in tables.items():
        T = table.detach().cpu().numpy().astype(np.int64)             # small host tables: integer bookkeeping in numpy
        R, C = T.shape[0] - 1, T.shape[2]
        if any(r < 1 or r > R for r in radii):
            raise ValueError("summarise_boundary: radii {} for a table of radius {} (1..{} can be read from it)".format(radii, R, R))
        keep = [c for c in range(C) if c not in ignore]
        total = T.sum(0)
        out[layer] = {}
        for r in radii:
            band = T[:r].sum(0)
            inner = total - band
            G, P, I = (torch.from_numpy(v).to(torch.float32) for v in (band[0] + band[2], band[3], band[4]))
            rows = dict(band_iou=summarise_iou([torch.from_numpy(v) for v in band[:3]])[0],
                        interior_iou=summarise_iou([torch.from_numpy(v) for v in inner[:3]])[0],
                        boundary_iou=I / torch.maximum(floor, G + P - I))
            entry = {}
            for key, values in rows.items():
                entry[key] = values
                entry[key.replace("_iou", "_miou")] = class_subset_mean(values, ignore_classes)
            entry["error_share"] = _ratio(int((band[1] + band[2])[keep].sum()), int((total[1] + total[2])[keep].sum()))
            entry["pixel_share"] = _ratio(int((band[0] + band[2])[keep].sum()), int((total[0] + total[2])[keep].sum()))
            out[layer][r] = entry
    return out


def format_boundary(summary, names):
    """Fixed-width text of a `summarise_boundary` result for the log: per layer one line per radius with the three means and the
    two shares, then one row per class (`names`, C of them) with band / interior / Boundary IoU at every radius."""
    names = [str(n) for n in names]
    lines = []
    for layer, by_radius in summary.items():
        radii = sorted(by_radius)
        lines.append("{}: boundary bands".format(layer))
        for r in radii:
            e = by_radius[r]
            assert len(names) == len(e["band_iou"]), (len(names), len(e["band_iou"]))
            lines.append("  r={:<2d} band mIoU {:.4f}  interior mIoU {:.4f}  boundary mIoU {:.4f}  errors in band {:.4f}  pixels in band {:.4f}".format(
                r, e["band_miou"], e["interior_miou"], e["boundary_miou"], e["error_share"], e["pixel_share"]))
        cells = [["{:.4f}  {:.4f}  {:.4f}".format(float(by_radius[r]["band_iou"][c]), float(by_radius[r]["interior_iou"][c]),
                                                 float(by_radius[r]["boundary_iou"][c])) for r in radii] for c in range(len(names))]
        lines += _table("class", ["band@{0} intr@{0} bIoU@{0}".format(r) for r in radii], [23] * len(radii), names, cells)
    return "\n".join(lines)


def summarise_consistency(tables, ignore_classes=(), top=10):
    """Reading of the view-consistency tables (`validation(..., consistency=True).consistency`, or `SAC.consistency_tables()`: a
    dict or anything with agree / flips / per_view, host or device; the result is plain host numbers).  Per pixel the kernel counted
    k, the teacher views that cover it, the consensus class c* (arg-max of the summed views) and m, the covered views whose own
    arg-max is c*: agree[c*][k][m], and agree[C][0][0] where no view reaches.  Every share below counts the pixels with k >= 2
    only -- a pixel seen by one view cannot disagree.  Returns a dict:
      classes               one dict per class c: pixels (k >= 2), agreement = sum m / sum k, unanimous = share with m == k, by_k =
                            [T+1] shares of those pixels seen by exactly k views (entries 0 and 1 are 0); all 0 without such pixels;
      agreement             sum_c pixels_c * agreement_c / sum_c pixels_c over the classes not in `ignore_classes`: pixel-weighted;
      class_mean_agreement  the plain mean of agreement_c over the classes not ignored that have any k >= 2 pixel;
      classes_present       how many those are;
      uncovered_share       agree[C][0][0] over all pixels;
      flips                 the `top` largest off-diagonal entries of flips + flips^T (a pair of covered views whose arg-maxes are a
                            and b, in either order): dicts with a < b, pairs, share_a and share_b = pairs over all pairs that involve
                            a (b), the agreeing ones on the diagonal included; largest first, ties by (a, b); ignored classes left out;
      views                 one dict per view slot t: coverage = covered pixels / all pixels, agreement = covered pixels whose
                            arg-max is c* / covered pixels.
    `agreement` is a label-free score of a checkpoint, with one caveat that no table can remove: a COLLAPSED model that predicts one
    class everywhere agrees with itself perfectly and scores 1.0.  `classes_present` stands next to the score for that reason --
    read them together (and `flips`, which is empty in that case)."""
    get = (lambda k: tables[k]) if isinstance(tables, dict) else (lambda k: getattr(tables, k))
    A, F, V = (get(k).detach().cpu().to(torch.int64).numpy() for k in ("agree", "flips", "per_view"))   # small host tables: numpy
    C, T = A.shape[0] - 1, A.shape[1] - 1
    ks = np.arange(T + 1, dtype=np.int64)
    multi = A[:C, 2:]                                             # [C, T-1, T+1]: k >= 2
    by_k_pixels = np.concatenate([np.zeros((C, min(2, T + 1)), np.int64), multi.sum(2)], 1)
    pixels = multi.sum((1, 2))
    sum_m, sum_k = (multi * ks[None, None, :]).sum((1, 2)), (multi.sum(2) * ks[None, 2:]).sum(1)
    unanimous = sum((A[:C, k, k] for k in range(2, T + 1)), np.zeros(C, np.int64))
    agreement, una, by_k = _ratio(sum_m, sum_k), _ratio(unanimous, pixels), _ratio(by_k_pixels, pixels[:, None])
    classes = [dict(pixels=int(pixels[c]), agreement=float(agreement[c]), unanimous=float(una[c]), by_k=by_k[c].tolist())
               for c in range(C)]
    ignore = set(int(i) for i in ignore_classes)
    kept = [c for c in range(C) if c not in ignore and int(pixels[c]) > 0]
    total = int(A.sum())
    S = F + F.T - np.diag(np.diagonal(F))
    involved = S.sum(1)
    flips = [dict(a=a, b=b, pairs=n, share_a=n / int(involved[a]), share_b=n / int(involved[b]))
             for n, a, b in _largest_entries(S, ignore, top, upper=True)]
    views = [dict(coverage=_ratio(int(V[t, 0]), total), agreement=_ratio(int(V[t, 1]), int(V[t, 0]))) for t in range(T)]
    return dict(classes=classes,
                agreement=_ratio(sum(int(pixels[c]) * float(agreement[c]) for c in kept), sum(int(pixels[c]) for c in kept)),
                class_mean_agreement=_ratio(sum(float(agreement[c]) for c in kept), len(kept)),
                classes_present=len(kept), uncovered_share=_ratio(int(A[C, 0, 0]), total), flips=flips, views=views)


def format_consistency(summary, names):
    """Fixed-width text table of a `summarise_consistency` result for the log: the scores, one row per class (`names`, C of them),
    the most frequent flips and one row per view slot."""
    names = [str(n) for n in names]
    assert len(names) == len(summary["classes"]), (len(names), len(summary["classes"]))
    n_k = len(summary["classes"][0]["by_k"]) if names else 0
    lines = ["view agreement {:.4f} (class mean {:.4f}, {} of {} classes present), uncovered {:.4f}".format(
        summary["agreement"], summary["class_mean_agreement"], summary["classes_present"], len(names), summary["uncovered_share"])]
    cells = [[str(row["pixels"]), "{:.4f}".format(row["agreement"]), "{:.4f}".format(row["unanimous"])] +
             ["{:.3f}".format(v) for v in row["by_k"][2:]] for row in summary["classes"]]
    lines += _table("class", ["pixels", "agree", "unanim"] + ["k={}".format(k) for k in range(2, n_k)], [12, 7, 7] + [6] * max(n_k - 2, 0),
                    names, cells)
    if summary["flips"]:
        lines.append("flips: " + ", ".join("{} <-> {} {} ({:.3f} / {:.3f})".format(names[f["a"]], names[f["b"]], f["pairs"], f["share_a"],
                                                                               f["share_b"]) for f in summary["flips"]))
    lines.append("views: " + ", ".join("{}: covers {:.4f}, agrees {:.4f}".format(t, v["coverage"], v["agreement"])
                                       for t, v in enumerate(summary["views"])))
    return "\n".join(lines)


def gradient_report(net, optim, table=None, top=10):
    """Reading of a gradient health table (`optim.tensor_stats` by default, or e.g. `optim.measure_tensor_stats()`; fp64
    [n_params, 8], dasac_hip.optim.TENSOR_STATS_COLUMNS, rows in the flattened `param_groups` order).  THE ONE PLACE that copies
    the table to the host -- a synchronisation: call it when logging, not every step.  Names are those of
    `net.named_parameters()` (through `.module` if wrapped), lr is each group's.  Returns a plain dict:
      tensors     one dict per parameter, in table order: name, group, numel, grad_norm, share (of the global squared gradient
                  norm), g_maxabs, zero_share (g_zeros / numel), weight_norm, update_ratio (lr * ||g|| / ||w||, 0 where ||w|| is 0),
                  state_norm, nonfinite (count) and first_nonfinite (index tuple in the parameter's shape, or None);
      groups      the same aggregated per parameter group: group, lr, tensors, numel, grad_norm, share, g_maxabs, zero_share,
                  weight_norm, update_ratio, state_norm, nonfinite;
      grad_norm   the global L2 norm over the finite gradient entries;
      nonfinite   the names of the tensors with non-finite gradient entries;
      top         the names of the `top` tensors by share, largest first (ties by table order).
    A parameter without a pending gradient has a row of zeros: it is listed with grad_norm 0 and share 0."""
    core = net.module if hasattr(net, "module") else net
    names = {p: name for name, p in core.named_parameters()}
    T = (optim.tensor_stats if table is None else table).detach().cpu().to(torch.float64).numpy()
    params = [(gi, p) for gi, group in enumerate(optim.param_groups) for p in group["params"]]
    assert T.shape == (len(params), 8), (T.shape, len(params))
    total_sq = float(T[:, 0].sum())
    tensors = []
    for i, ((gi, p), row) in enumerate(zip(params, T.tolist())):
        g_norm, w_norm, lr = math.sqrt(row[0]), math.sqrt(row[5]), float(optim.param_groups[gi]["lr"])
        first = tuple(int(v) for v in np.unravel_index(int(row[3]) - 1, tuple(p.shape))) if row[3] > 0 else None
        tensors.append(dict(name=names.get(p, "param{}".format(i)), group=gi, numel=p.numel(), grad_norm=g_norm,
                            share=_ratio(row[0], total_sq), g_maxabs=row[1], zero_share=row[4] / max(p.numel(), 1), weight_norm=w_norm,
                            update_ratio=_ratio(lr * g_norm, w_norm), state_norm=math.sqrt(row[7]), nonfinite=int(row[2]),
                            first_nonfinite=first))
    groups = []
    for gi, group in enumerate(optim.param_groups):
        rows = T[[i for i, (g, _) in enumerate(params) if g == gi]].reshape(-1, 8)
        numel = sum(p.numel() for p in group["params"])
        g_norm, w_norm = math.sqrt(float(rows[:, 0].sum())), math.sqrt(float(rows[:, 5].sum()))
        groups.append(dict(group=gi, lr=float(group["lr"]), tensors=len(group["params"]), numel=numel, grad_norm=g_norm,
                           share=_ratio(float(rows[:, 0].sum()), total_sq), g_maxabs=float(rows[:, 1].max()) if len(rows) else 0.0,
                           zero_share=float(rows[:, 4].sum()) / max(numel, 1), weight_norm=w_norm,
                           update_ratio=_ratio(float(group["lr"]) * g_norm, w_norm), state_norm=math.sqrt(float(rows[:, 7].sum())),
                           nonfinite=int(rows[:, 2].sum())))
    return dict(tensors=tensors, groups=groups, grad_norm=math.sqrt(total_sq), nonfinite=[t["name"] for t in tensors if t["nonfinite"]],
                top=[tensors[i]["name"] for i in _by_key(tensors, "share")[:top]])


def skipped_step_report(net, optim, top=10):
    """`gradient_report` over `optim.last_skipped_stats` -- the table of the last step that `skip_nonfinite` skipped -- plus
    `captured_at`: `optim.skipped_steps` as it stood right after that step (0: no step has been skipped, the table is zeros)."""
    table, at = optim.last_skipped_stats
    report = gradient_report(net, optim, table=table, top=top)
    report["captured_at"] = int(at)
    return report


def format_gradient_report(report, top=10):
    """Fixed-width text table of a `gradient_report` for the log: the `top` tensors by share of the squared gradient norm, then
    every tensor with non-finite entries that is not among them, then one line per group and the global norm."""
    rows = _top_then_flagged(report["tensors"], "share", top)
    labels = ["group {} (lr {:.3g}, {} tensors)".format(g["group"], g["lr"], g["tensors"]) for g in report["groups"]]

    def cells(t, first):
        return [str(t["group"]), str(t["numel"]), "{:.3e}".format(t["grad_norm"]), "{:.4f}".format(t["share"]), "{:.3e}".format(t["g_maxabs"]),
                "{:.4f}".format(t["zero_share"]), "{:.3e}".format(t["weight_norm"]), "{:.3e}".format(t["update_ratio"]),
                "{:.3e}".format(t["state_norm"]), str(t["nonfinite"]), "-" if first is None else str(first)]
    lines = _table("tensor", ["group", "numel", "|g|", "share", "max|g|", "zeros", "|w|", "lr|g|/|w|", "|state|", "nonfinite", "first"],
                   [5, 9, 10, 7, 10, 7, 10, 10, 10, 9], [t["name"] for t in rows] + labels,      # the last cell is not padded
                   [cells(t, t["first_nonfinite"]) for t in rows] + [cells(g, None) for g in report["groups"]])
    lines.append("global gradient norm {:.6e}; tensors with non-finite entries: {}".format(
        report["grad_norm"], ", ".join(report["nonfinite"]) if report["nonfinite"] else "none"))
    if "captured_at" in report:
        lines.append("captured at skipped step {}".format(report["captured_at"]))
    return "\n".join(lines)


def _host_table(record):
    T = record.table
    T = T.detach().cpu().to(torch.float64).numpy() if isinstance(T, torch.Tensor) else np.asarray(T, dtype=np.float64)
    R = sum(e["C"] for e in record.layout)
    assert T.ndim == 3 and T.shape == (len(record.bounds) - 1, R, 6), (T.shape, len(record.bounds) - 1, R)
    return T


def activation_report(record, segment=0, top=10):
    """Reading of one segment of an activation table.  THE ONE PLACE that copies it to the host -- a synchronisation: call it when
    logging.  Returns a plain dict:
      layers   one dict per tensor in plan order: name, kind, shape (n, C, H, W with n the segment's samples), mean and std over
               the finite entries of all channels, maxabs, zero_share (zeros / elements), dead_channels (channels whose every
               entry is 0: a dead ReLU unit), nonfinite (count) and first_nonfinite ((n, c, y, x) in the tensor, or None);
      first_nonfinite_layer   the name of the first layer in plan order with non-finite entries, or None: where a fault began;
      top      the names of the `top` layers by maxabs, largest first (ties in plan order);
      net, segment, samples (first, one past the last)."""
    T = _host_table(record)[segment]
    lo, hi = record.bounds[segment], record.bounds[segment + 1]
    layers = []
    for e in record.layout:
        rows = T[e["row0"]:e["row0"] + e["C"]]
        per_channel = (hi - lo) * e["H"] * e["W"]
        total, finite = per_channel * e["C"], per_channel * e["C"] - float(rows[:, 3].sum())
        mean = _ratio(float(rows[:, 0].sum()), finite)
        var = max(float(rows[:, 1].sum()) / finite - mean * mean, 0.0) if finite > 0 else 0.0
        firsts = rows[:, 4][rows[:, 4] > 0]
        first = tuple(int(v) for v in np.unravel_index(int(firsts.min()) - 1, (record.N, e["C"], e["H"], e["W"]))) if len(firsts) else None
        layers.append(dict(name=e["name"], kind=e["kind"], shape=(hi - lo, e["C"], e["H"], e["W"]), mean=mean, std=math.sqrt(var),
                           maxabs=float(rows[:, 2].max()), zero_share=float(rows[:, 5].sum()) / total,
                           dead_channels=int((rows[:, 5] == per_channel).sum()), nonfinite=int(rows[:, 3].sum()), first_nonfinite=first))
    bad = [l["name"] for l in layers if l["nonfinite"]]
    return dict(layers=layers, first_nonfinite_layer=bad[0] if bad else None, top=[layers[i]["name"] for i in _by_key(layers, "maxabs")[:top]],
                net=record.net, segment=segment, samples=(lo, hi))


def moment_gap(mu_a, var_a, mu_b, var_b):
    """The per-channel distance of two sets of moments that `domain_gap_report` and `class_gap_report` share (numpy float64,
    broadcasting): num = (mu_a - mu_b)^2 + (sigma_a - sigma_b)^2, den = (var_a + var_b) / 2, 0 where num == 0, else
    num / max(den, 1e-30)."""
    num = (mu_a - mu_b) ** 2 + (np.sqrt(var_a) - np.sqrt(var_b)) ** 2
    return np.where(num == 0, 0.0, num / np.maximum(0.5 * (var_a + var_b), 1e-30))


def domain_gap_report(a, b=None, top=10):
    """Per-layer covariate shift between two domains under the same weights: two records of the same net (segment 0 of each), or
    ONE record with two segments (segments 0 and 1: `forward_fused`'s [source; target] batch).  Copies the tables to the host.
    Per channel, with n elements per domain: mu = sum / n, var = max(sumsq / n - mu^2, 0), sigma = sqrt(var),
      num = (mu_a - mu_b)^2 + (sigma_a - sigma_b)^2,  den = (var_a + var_b) / 2,  gap_c = 0 if num == 0 else num / max(den, 1e-30).
    Returns a plain dict:
      layers   one dict per tensor in plan order: name, kind, gap (mean of gap_c over the channels that are not dead -- all
               zero -- in BOTH domains; 0 if none), gap_max and gap_max_channel, mean_shift (RMS over channels of mu_a - mu_b),
               dead_only_a, dead_only_b, dead_both (channel counts);
      top      the names of the `top` layers by gap, largest first (ties in plan order).
    Refuses records whose layouts differ."""
    if b is None:
        if len(a.bounds) < 3:
            raise ValueError("domain_gap_report: one record needs two segments (got bounds {})".format(a.bounds))
        b, sa, sb = a, 0, 1
    else:
        sa = sb = 0
    same = lambda e: (e["name"], e["kind"], e["C"], e["H"], e["W"], e["row0"])
    if [same(e) for e in a.layout] != [same(e) for e in b.layout]:
        raise ValueError("domain_gap_report: the two records have different layouts")
    Ta, Tb = _host_table(a)[sa], _host_table(b)[sb]
    layers = []
    for e in a.layout:
        rows = slice(e["row0"], e["row0"] + e["C"])
        na = float((a.bounds[sa + 1] - a.bounds[sa]) * e["H"] * e["W"])
        nb = float((b.bounds[sb + 1] - b.bounds[sb]) * e["H"] * e["W"])
        mu_a, mu_b = Ta[rows, 0] / na, Tb[rows, 0] / nb
        var_a, var_b = np.maximum(Ta[rows, 1] / na - mu_a ** 2, 0.0), np.maximum(Tb[rows, 1] / nb - mu_b ** 2, 0.0)
        gap_c = moment_gap(mu_a, var_a, mu_b, var_b)
        dead_a, dead_b = Ta[rows, 5] == na, Tb[rows, 5] == nb
        alive = ~(dead_a & dead_b)
        worst = int(np.argmax(gap_c))
        layers.append(dict(name=e["name"], kind=e["kind"], gap=float(gap_c[alive].mean()) if alive.any() else 0.0,
                           gap_max=float(gap_c[worst]), gap_max_channel=worst, mean_shift=float(np.sqrt(np.mean((mu_a - mu_b) ** 2))),
                           dead_only_a=int((dead_a & ~dead_b).sum()), dead_only_b=int((dead_b & ~dead_a).sum()),
                           dead_both=int((dead_a & dead_b).sum())))
    return dict(layers=layers, top=[layers[i]["name"] for i in _by_key(layers, "gap")[:top]], net=a.net)


def format_activation_report(report, top=10):
    """Fixed-width text table of an `activation_report` for the log: the `top` layers by maxabs, then every layer with non-finite
    entries that is not among them (plan order), then one summary line."""
    rows = _top_then_flagged(report["layers"], "maxabs", top)
    cells = [[l["kind"], "x".join(str(v) for v in l["shape"]), "{:.3e}".format(l["mean"]), "{:.3e}".format(l["std"]),
              "{:.3e}".format(l["maxabs"]), "{:.4f}".format(l["zero_share"]), str(l["dead_channels"]), str(l["nonfinite"]),
              "-" if l["first_nonfinite"] is None else str(l["first_nonfinite"])] for l in rows]
    lines = _table("layer", ["kind", "shape", "mean", "std", "max|x|", "zeros", "dead", "nonfinite", "first"], [6, 18, 11, 10, 10, 7, 5, 9, 5],
                   [l["name"] for l in rows], cells)
    lines.append("{} segment {} (samples {}..{}): {} layers; first layer with non-finite entries: {}".format(
        report["net"], report["segment"], report["samples"][0], report["samples"][1] - 1, len(report["layers"]),
        report["first_nonfinite_layer"] or "none"))
    return "\n".join(lines)


def format_domain_gap_report(report, top=10):
    """Fixed-width text table of a `domain_gap_report`: the `top` layers by gap, largest first, then one summary line."""
    rows = [report["layers"][i] for i in _by_key(report["layers"], "gap")[:top]]
    cells = [[l["kind"], "{:.3e}".format(l["gap"]), "{:.3e}".format(l["gap_max"]), str(l["gap_max_channel"]), "{:.3e}".format(l["mean_shift"]),
              str(l["dead_only_a"]), str(l["dead_only_b"]), str(l["dead_both"])] for l in rows]
    lines = _table("layer", ["kind", "gap", "gap_max", "channel", "mean_shift", "dead_a", "dead_b", "dead_ab"], [6, 10, 10, 7, 10, 6, 6, 7],
                   [l["name"] for l in rows], cells)
    lines.append("{}: {} layers; largest gap: {}".format(report["net"], len(report["layers"]), rows[0]["name"] if rows else "none"))
    return "\n".join(lines)


def _class_moments(record):
    """(n [C], mu [C,Cf], var [C,Cf], dead [C,Cf]) in numpy float64 from a ClassFeatureRecord, a ClassFeatureTable or anything with
    `sums` / `counts` (torch tensors or arrays): the one host copy."""
    table = getattr(record, "table", record)
    host = lambda t, dt: t.detach().cpu().numpy().astype(dt) if isinstance(t, torch.Tensor) else np.asarray(t, dtype=dt)
    sums, counts = host(table.sums, np.float64), host(table.counts, np.int64)
    assert sums.ndim == 3 and sums.shape[2] == 2 and counts.shape == (sums.shape[0],), (sums.shape, counts.shape)
    n = np.maximum(counts, 1).astype(np.float64)[:, None]
    mu = sums[..., 0] / n
    var = np.maximum(sums[..., 1] / n - mu ** 2, 0.0)
    return counts, mu, var, sums[..., 1] == 0


def _row_distance(mu_a, var_a, dead_a, mu_b, var_b, dead_b):
    """D of two class rows: `moment_gap` averaged over the channels that are not dead (all zero) in both; 0 if there is none."""
    alive = ~(dead_a & dead_b)
    return float(moment_gap(mu_a, var_a, mu_b, var_b)[alive].mean()) if alive.any() else 0.0


def class_gap_report(a, b=None, ignore_classes=(), min_nodes=16, top=5):
    """Reads two class feature tables -- `a` (say, the source) against `b` (the target) -- or `a` alone.  Host-side float64; THE ONE
    PLACE that copies the tables to the host.  Per class c with n_c nodes: mu_c[f] = sum / n_c, var_c[f] = max(sumsq / n_c - mu^2,
    0).  D(row, row') is `domain_gap_report`'s per-channel formula (`moment_gap`) averaged over the channels not dead in both rows.
    A class counts in a table when it is not in `ignore_classes` and has at least `min_nodes` nodes there.  With `b`, per class c
    that counts in both:
      gap[c]      D(a_c, b_c): how far the class moved between the domains;
      nearest[c]  argmin over k != c (k counting in a) of D(b_c, a_k), with nearest_distance[c];
      margin[c]   nearest_distance[c] / gap[c]: below 1, b's class c lies nearer to ANOTHER class of a than to its own (inf when
                  gap is 0).
    Returns a plain dict: gap, nearest (-1: none), nearest_distance, margin (numpy [C]; NaN for the classes in `skipped`), matrix
    [C,C] = D(b_c, a_k) (NaN where c does not count in b or k not in a), counts_a, counts_b, skipped ({class: reason} -- "ignored",
    "absent" or "under min_nodes"), top (the `top` classes by margin, smallest first), layer, Cf.
    With b=None the same within `a`: matrix = D(a_c, a_k) with a zero diagonal, gap = 0, margin = inf, and top lists the classes by
    nearest_distance, smallest first -- class separability.  Refuses tables of different shapes or, for records, layers."""
    within = b is None
    if within:
        b = a
    na, mu_a, var_a, dead_a = _class_moments(a)
    nb, mu_b, var_b, dead_b = _class_moments(b)
    if mu_a.shape != mu_b.shape:
        raise ValueError("class_gap_report: tables of different shapes {} and {}".format(mu_a.shape, mu_b.shape))
    if getattr(a, "layer", None) != getattr(b, "layer", None):
        raise ValueError("class_gap_report: records of different layers {!r} and {!r}".format(getattr(a, "layer", None), getattr(b, "layer", None)))
    C, Cf = mu_a.shape
    ignored = set(int(c) for c in ignore_classes)
    in_a = [c not in ignored and na[c] >= max(int(min_nodes), 1) for c in range(C)]
    in_b = [c not in ignored and nb[c] >= max(int(min_nodes), 1) for c in range(C)]
    skipped = {}
    for c in range(C):
        if not (in_a[c] and in_b[c]):
            skipped[c] = "ignored" if c in ignored else ("absent" if min(na[c], nb[c]) == 0 else "under min_nodes")
    matrix = np.full((C, C), np.nan)
    for c in range(C):
        for k in range(C):
            if in_b[c] and in_a[k]:
                matrix[c, k] = 0.0 if (within and c == k) else _row_distance(mu_b[c], var_b[c], dead_b[c], mu_a[k], var_a[k], dead_a[k])
    gap, dist, margin = np.full(C, np.nan), np.full(C, np.nan), np.full(C, np.nan)
    nearest = np.full(C, -1, dtype=np.int64)
    for c in range(C):
        if c in skipped:
            continue
        gap[c] = matrix[c, c]
        others = [k for k in range(C) if k != c and in_a[k]]
        if others:
            nearest[c] = min(others, key=lambda k: (matrix[c, k], k))
            dist[c] = matrix[c, nearest[c]]
            margin[c] = dist[c] / gap[c] if gap[c] > 0 else (np.inf if dist[c] > 0 or within else np.nan)
    key = dist if within else margin
    order = sorted([c for c in range(C) if c not in skipped and nearest[c] >= 0], key=lambda c: (key[c], c))
    return dict(gap=gap, nearest=nearest, nearest_distance=dist, margin=margin, matrix=matrix, counts_a=na, counts_b=nb,
                skipped=skipped, top=order[:top], layer=getattr(a, "layer", None), Cf=Cf, within=within)


def format_class_gap_report(report, names=None):
    """Fixed-width text table of a `class_gap_report`: one line per class that counts, by margin (alone: by nearest distance),
    smallest first, then one summary line.  names: class names (default: the indices)."""
    C = len(report["gap"])
    name = lambda c: str(c) if c < 0 or names is None else str(names[c])
    key = report["nearest_distance"] if report["within"] else report["margin"]
    rows = sorted([c for c in range(C) if c not in report["skipped"]], key=lambda c: (key[c] != key[c], key[c], c))
    nearest = [int(report["nearest"][c]) for c in rows]
    cells = [[str(int(report["counts_a"][c])), str(int(report["counts_b"][c])), "{:.3e}".format(report["gap"][c]), name(k) if k >= 0 else "-",
              "{:.3e}".format(report["nearest_distance"][c]), "{:.3e}".format(report["margin"][c])] for c, k in zip(rows, nearest)]
    lines = _table("class", ["n_a", "n_b", "gap", "nearest", "distance", "margin"],
                   [9, 9, 10, max([len("nearest")] + [len(name(k)) for k in nearest]), 10, 10], [name(c) for c in rows], cells)
    below = [c for c in rows if report["margin"][c] < 1]
    lines.append("{}: {} channels, {} of {} classes compared, {} skipped; margin below 1: {}".format(
        report["layer"] or "table", report["Cf"], len(rows), C, len(report["skipped"]), ", ".join(name(c) for c in below) or "none"))
    return "\n".join(lines)


def stat_mean(values):
    """`StatManager.update_stats` + `summarize_key` (utils/stat_manager.py:40-61) over one key's values: python-float sum
    divided by the count, and 0 when there is no value or the sum is exactly 0."""
    total = 0.0
    for v in values:
        total += v
    return total / len(values) if len(values) > 0 and abs(total) > 0. else 0


def class_subset_mean(values, ignore_classes=()):
    """train.py:370-371,447-460: float32 mean over the classes NOT listed in VAL.IGNORE_CLASS."""
    ignore = set(int(i) for i in ignore_classes)
    return torch.Tensor([float(v) for i, v in enumerate(values) if i not in ignore]).mean().item()


def summarise_validation(counts, ignore_classes=()):
    """counts {layer: int64 [3,C]} -> (per_class {layer: (jaccard, precision, recall)}, mean {layer: (mIoU, precision,
    recall)} over the kept classes, checkpoint_score = max over layers of mIoU, starting from 0.0: train.py:408,430-464)."""
    per_class, mean, score = {}, {}, 0.0
    for layer, table in counts.items():
        per_class[layer] = summarise_iou(table)
        mean[layer] = tuple(class_subset_mean(v, ignore_classes) for v in per_class[layer])
        score = max(mean[layer][0], score)
    return per_class, mean, score
