"""Numpy model of the segment ops (include/dasac_hip.h: dasac_label_segments, dasac_segment_counts, dasac_segment_filter) and the
label-map patterns their tests run on (a helper, not a test).  Connected components by a two-pass union-find over the runs of each
row; the tables are written straight from the header's definitions.  tests/test_segments_cpu.py checks the model against
scipy.ndimage.label, tests/test_gpu_segments.py checks the kernels against the model bit for bit."""
import numpy as np

from boundary_ref import argmax_first, blocky, class_index  # noqa: F401  (re-exported for the tests)

BINS = 24
ROWS = ("segments", "pixels", "matched_pixels", "matched_segments")


def bin_of(size):
    """min(floor(log2(size)), BINS - 1) for size >= 1."""
    return min(int(size).bit_length() - 1, BINS - 1)


def _image_segments(cls, connectivity):
    """(root, size) int32 [H,W] of one image of class indices (-1 = no class)."""
    H, W = cls.shape
    reach = 1 if connectivity == 8 else 0
    parent, runs, prev = [], [], []                    # runs: (y, start, end); prev: the previous row's (start, end, class, node)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for y in range(H):
        row = cls[y]
        starts = np.flatnonzero(np.r_[True, row[1:] != row[:-1]])
        ends = np.r_[starts[1:], W]
        cur, first = [], 0                             # first: the first run of the previous row that can still reach a run here
        for s, e in zip(starts.tolist(), ends.tolist()):
            c = int(row[s])
            if c < 0:
                continue
            node = len(parent)
            parent.append(node)
            runs.append((y, s, e))
            while first < len(prev) and prev[first][1] <= s - reach:
                first += 1
            k = first
            while k < len(prev) and prev[k][0] < e + reach:
                if prev[k][2] == c:
                    a, b = find(node), find(prev[k][3])
                    if a != b:
                        parent[max(a, b)] = min(a, b)      # nodes are numbered in raster order: the root is the first run
                k += 1
            cur.append((s, e, c, node))
        prev = cur
    root = np.full((H, W), -1, np.int32)
    for node, (y, s, e) in enumerate(runs):
        ry, rs, _ = runs[find(node)]
        root[y, s:e] = ry * W + rs
    size = np.zeros((H, W), np.int32)
    inside = root >= 0
    size[inside] = np.bincount(root[inside], minlength=H * W)[root[inside]]
    return root, size


def segments(labels, C, connectivity):
    """(root map, size map) int32 [B,H,W]: the smallest y*W + x of the pixel's segment (-1: no class) and its pixel count (0)."""
    assert connectivity in (4, 8)
    cls = class_index(labels, C)
    parts = [_image_segments(cls[b], connectivity) for b in range(cls.shape[0])]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])


def filter_small(labels, min_size, C, fill=255, connectivity=8):
    """`labels` with `fill` wherever the pixel's segment has fewer than min_size pixels."""
    labels = np.asarray(labels)
    root, size = segments(labels, C, connectivity)
    return np.where((root >= 0) & (size < min_size), np.asarray(fill).astype(labels.dtype), labels)


def _per_segment(root, weights):
    """{(image, root): sum of weights over the segment's pixels} as (keys [n,2], sums [n]) over all segments of a root map."""
    B, H, W = root.shape
    key = root.astype(np.int64) + (np.arange(B, dtype=np.int64) * H * W)[:, None, None]
    inside = root >= 0
    keys, inverse = np.unique(key[inside], return_inverse=True)
    return keys, [np.bincount(inverse, w[inside].astype(np.int64), len(keys)).astype(np.int64) for w in weights]


def segment_table(pred, gt, C, connectivity, ignore_index=255, gt_segments=None):
    """The table int64 [2,BINS,4,C] of one predicted map [B,H,W] (values as they are) against gt [B,H,W]."""
    pred, gt = np.asarray(pred).astype(np.int64), np.asarray(gt).astype(np.int64)
    B, H, W = gt.shape
    keep = gt != ignore_index
    g_map = np.where(keep, gt, -1)                         # an ignored pixel is no class in the ground-truth map: checked first
    pc, gc = class_index(pred, C), class_index(g_map, C)
    hit = keep & (pc == gc) & (pc >= 0)
    out = np.zeros((2, BINS, 4, C), np.int64)
    one = np.ones(gt.shape, np.int64)

    def add(side, root, cls_flat, keys, s, n, m):
        for k, sk, nk, mk in zip(keys.tolist(), s.tolist(), n.tolist(), m.tolist()):
            if nk == 0:
                continue
            c, b = int(cls_flat[k]), bin_of(sk)
            out[side, b, 0, c] += 1
            out[side, b, 1, c] += nk
            out[side, b, 2, c] += mk
            out[side, b, 3, c] += 2 * mk > nk
    g_root = (segments(g_map, C, connectivity) if gt_segments is None else gt_segments)[0]
    keys, (s, m) = _per_segment(g_root, [one, hit])
    add(0, g_root, gc.reshape(-1), keys, s, s, m)
    p_root = segments(pred, C, connectivity)[0]            # over the whole map, ignored pixels included
    keys, (s, n, m) = _per_segment(p_root, [one, keep, hit])
    add(1, p_root, pc.reshape(-1), keys, s, n, m)
    return out


def segment_tables(scores, label_maps, gt, C, connectivity, ignore_index=255):
    """int64 [L,2,BINS,4,C] as `ops.segment_counts` returns it: score tensors [B,C,H,W] first (arg-max), then label maps."""
    gt = np.asarray(gt).astype(np.int64)
    gs = segments(np.where(gt != ignore_index, gt, -1), C, connectivity)
    preds = [argmax_first(s) for s in scores] + [np.asarray(m) for m in label_maps]
    return np.stack([segment_table(p, gt, C, connectivity, ignore_index, gs) for p in preds])


# ---- patterns: [H,W] int64 maps of the classes a (and b) ---------------------------------------------------------------------------
def uniform(H, W, a=1):
    return np.full((H, W), a, np.int64)


def checkerboard(H, W, a=0, b=1):
    yy, xx = np.mgrid[:H, :W]
    return np.where((yy + xx) % 2 == 0, a, b).astype(np.int64)


def diagonals(H, W, a=2, b=0, period=3):
    """One-pixel diagonals of class a, `period` apart, on class b: one segment each under connectivity 8, single pixels under 4."""
    yy, xx = np.mgrid[:H, :W]
    return np.where((yy + xx) % period == 0, a, b).astype(np.int64)


def serpentine(H, W, a=1, b=0):
    """Class a in every second row, joined alternately at the right and left ends: ONE segment winding through the whole image."""
    m = np.full((H, W), b, np.int64)
    m[0::2] = a
    for k, y in enumerate(range(1, H, 2)):
        if y + 1 < H:
            m[y, W - 1 if k % 2 == 0 else 0] = a
    return m


def spiral(H, W, a=1, b=0):
    """A square spiral of class a, one pixel wide with one pixel of b between its arms: the rings of `rings`, each cut open below its
    top-left corner and joined there to the next ring in."""
    yy, xx = np.mgrid[:H, :W]
    d = np.minimum(np.minimum(yy, H - 1 - yy), np.minimum(xx, W - 1 - xx))
    m = np.where(d % 2 == 0, a, b).astype(np.int64)
    for k in range(0, min(H, W) // 2 - 2, 2):
        m[k + 1, k] = b
        m[k + 2, k + 1] = a
    return m


def rings(H, W, a=1, b=2):
    """Concentric one-pixel rings, alternately a and b: nested components."""
    yy, xx = np.mgrid[:H, :W]
    d = np.minimum(np.minimum(yy, H - 1 - yy), np.minimum(xx, W - 1 - xx))
    return np.where(d % 2 == 0, a, b).astype(np.int64)


def comb(H, W, a=1, b=0, pitch=2):
    """Vertical arms of class a every `pitch` columns from the first row down, joined only by the last row (a U when two arms fit):
    a late merge, the root far from the join."""
    m = np.full((H, W), b, np.int64)
    m[:, 0::pitch] = a
    m[H - 1] = a
    return m


def row_wrap(H, W, a=1, b=0):
    """Runs of class a that end at x = W-1 of a row and start at x = 0 of the next: they must stay apart (W >= 3, H >= 2), and so
    must the last row of one image and the first row of the next, both all a here."""
    m = np.full((H, W), b, np.int64)
    m[0] = a
    m[H - 1] = a
    for y in range(2, H - 3, 4):                           # rows y, y + 1 and a free row on either side
        m[y, W - 1] = a
        m[y + 1, 0] = a
    return m


def random_map(H, W, classes, scale, rng, none_share=0.1):
    """Blocky random map of `classes` classes at `scale`, 255 sprinkled over `none_share` of the pixels."""
    m = blocky((1, H, W), list(range(classes)), scale, rng)[0].astype(np.int64)
    m[rng.random((H, W)) < none_share] = 255
    return m
