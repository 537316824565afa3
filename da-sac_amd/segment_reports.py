"""Host-side reader and renderer of the segment tables (`driver.validation(..., segment_tables=True).segments`; include/dasac_hip.h:
dasac_segment_counts): pure numpy arithmetic and string formatting, no network, no kernels.  reports.py and driver.py re-export
`summarise_segments` and `format_segments`; callers use `driver.<name>` as for every other reader."""
import numpy as np


def _nan_ratio(num, den):
    """num / den in float64, NaN where den is 0 (numpy arrays or numbers)."""
    num, den = np.asarray(num, np.float64), np.asarray(den, np.float64)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), np.nan)


def segment_groups(edges):
    """The size groups [(label, first bin, one past the last bin)] that power-of-two `edges` cut the 24 log2 bins into."""
    edges = [int(e) for e in edges]
    if any(e < 2 or e & (e - 1) for e in edges) or sorted(set(edges)) != edges or any(e >= 1 << 23 for e in edges):
        raise ValueError("summarise_segments: the edges must be increasing powers of two in 2..2^22, the bins are floor(log2(size)) "
                         "(got {})".format(edges))
    cuts = [0] + [e.bit_length() - 1 for e in edges] + [24]
    sizes = [1] + edges
    labels = ["< {}".format(edges[0])] if edges else ["all"]
    labels += ["{}-{}".format(a, b - 1) for a, b in zip(sizes[1:], edges[1:])] + ([">= {}".format(edges[-1])] if edges else [])
    return [(label, lo, hi) for label, lo, hi in zip(labels, cuts[:-1], cuts[1:])]


def summarise_segments(tables, ignore_classes=(), edges=(64, 1024, 16384)):
    """Reading of segment tables (`validation(..., segment_tables=True).segments`: {layer: int64 [2,24,4,C]}, host or device; include/
    dasac_hip.h: dasac_segment_counts).  Side 0 holds the ground truth's connected segments, side 1 the predicted map's, each in the
    bin floor(log2(size)); rows segments, pixels, matched pixels, matched segments.  The 24 bins are merged into the size groups that
    `edges` (powers of two, else ValueError) cut: "< 64", "64-1023", "1024-16383", ">= 16384" by default.  Returns
    {layer: {group: dict}}, each dict with float64 / int64 numpy arrays [C]
      gt_segments        ground-truth segments of the class and size group;
      object_recall      the share of them the prediction found (more than half of their pixels): row 3 / row 0 of side 0;
      pixel_recall       the share of their pixels it found: row 2 / row 1 of side 0;
      pred_segments      predicted segments (with any counted pixel);
      segment_precision  the share of them that are real (more than half of their counted pixels are right): row 3 / row 0 of side 1;
      unmatched_share    1 - segment_precision: spurious segments, the specks among the small ones;
      fragmentation      predicted segments / ground-truth segments of the group;
    and the same seven over all classes not in `ignore_classes` under the key with `all_` in front (python numbers).  A ratio with
    a zero denominator is NaN."""
    groups = segment_groups(edges)
    ignore = set(int(i) for i in ignore_classes)
    out = {}
    for layer, table in tables.items():
        T = table.detach().cpu().numpy().astype(np.int64)
        if T.ndim != 4 or T.shape[:3] != (2, 24, 4):
            raise ValueError("summarise_segments: a table is int64 [2,24,4,C] (got {})".format(T.shape))
        keep = [c for c in range(T.shape[3]) if c not in ignore]
        out[layer] = {}
        for label, lo, hi in groups:
            g, p = T[0, lo:hi].sum(0), T[1, lo:hi].sum(0)              # [4, C] each

            def read(g, p):
                precision = _nan_ratio(p[3], p[0])
                return dict(gt_segments=g[0], object_recall=_nan_ratio(g[3], g[0]), pixel_recall=_nan_ratio(g[2], g[1]),
                            pred_segments=p[0], segment_precision=precision, unmatched_share=1.0 - precision,
                            fragmentation=_nan_ratio(p[0], g[0]))
            entry = read(g, p)
            total = read(g[:, keep].sum(1), p[:, keep].sum(1))
            entry.update({"all_" + k: (int(v) if k.endswith("segments") else float(v)) for k, v in total.items()})
            out[layer][label] = entry
    return out


def format_segments(summary, names):
    """Fixed-width text of a `summarise_segments` result for the log: per layer a head line, one line per size group with the numbers
    over all counted classes, then one row per class (`names`, C of them) with ground-truth segments, object recall, predicted
    segments and segment precision in every group."""
    from reports import _table                     # at call time: reports.py imports this module
    names = [str(n) for n in names]
    lines = []
    for layer, by_group in summary.items():
        groups = list(by_group)
        lines.append("{}: segments by size".format(layer))
        for gname in groups:
            e = by_group[gname]
            assert len(names) == len(e["gt_segments"]), (len(names), len(e["gt_segments"]))
            lines.append("  {:<12s} gt segments {:8d}  object recall {:.4f}  pixel recall {:.4f}  predicted {:8d}  precision {:.4f}  "
                         "unmatched {:.4f}  fragmentation {:.3f}".format(
                             gname, e["all_gt_segments"], e["all_object_recall"], e["all_pixel_recall"], e["all_pred_segments"],
                             e["all_segment_precision"], e["all_unmatched_share"], e["all_fragmentation"]))
        cells = [["{:7d} {:.3f} {:7d} {:.3f}".format(int(by_group[gname]["gt_segments"][c]), float(by_group[gname]["object_recall"][c]),
                                                     int(by_group[gname]["pred_segments"][c]), float(by_group[gname]["segment_precision"][c]))
                  for gname in groups] for c in range(len(names))]
        lines += _table("class", ["gt/rec/pred/prec {}".format(gname) for gname in groups], [30] * len(groups), names, cells)
    return "\n".join(lines)
