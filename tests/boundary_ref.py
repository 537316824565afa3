"""Numpy model of `dasac_boundary_counts` (include/dasac_hip.h): Chebyshev distance of every class pixel to the nearest pixel of
another class, the slots, and the int64 [R+1,5,C] tables -- built ring by ring from shifted comparisons of whole maps (no loop over
pixels).  Shared by tests/test_boundary_cpu.py, which checks it against a per-pixel brute force, and tests/test_gpu_boundary.py,
which checks the kernel against it bit for bit."""
import numpy as np

ROWS = ("tp", "fp", "fn", "pred", "both")


def class_index(labels, C):
    """int64 map of class indices; -1 where the value is no class (255, -1, anything outside [0, C))."""
    labels = np.asarray(labels).astype(np.int64)
    return np.where((labels >= 0) & (labels < C), labels, -1)


def _shifted(cls, dy, dx):
    """out[b, y, x] = cls[b, y + dy, x + dx], -1 outside the image."""
    B, H, W = cls.shape
    out = np.full_like(cls, -1)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    if abs(dy) < H and abs(dx) < W:
        out[:, yd, xd] = cls[:, ys, xs]
    return out


def distances(labels, C, R):
    """d_L(p) for every pixel of maps [B,H,W]: 1..R, and R + 1 for "further than R", "no other class in reach" and "no class"."""
    cls = class_index(labels, C)
    d = np.full(cls.shape, R + 1, np.int64)
    for r in range(1, R + 1):
        found = np.zeros(cls.shape, bool)
        ring = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if max(abs(dy), abs(dx)) == r]
        for dy, dx in ring:
            other = _shifted(cls, dy, dx)
            found |= (other >= 0) & (other != cls)
        d = np.where((d > R) & found & (cls >= 0), r, d)
    return d


def slots(labels, C, R):
    d = distances(labels, C, R)
    return np.where(d <= R, d - 1, R)


def argmax_first(scores):
    """arg-max over axis 1 of [B,C,H,W], the first maximum wins (numpy's rule, and torch.argmax's)."""
    return np.argmax(np.asarray(scores), axis=1).astype(np.int64)


def mask_counts_ref(pred, gt, C, ignore_index=255):
    """Plain `dasac_mask_counts` counts int64 [3,C] = (tp, fp, fn) of a predicted map against the ground truth."""
    pred, gt = np.asarray(pred).astype(np.int64).ravel(), np.asarray(gt).astype(np.int64).ravel()
    keep = gt != ignore_index
    pred, gt = pred[keep], gt[keep]
    pc, gc = class_index(pred, C), class_index(gt, C)
    hit = pred == gt
    out = np.zeros((3, C), np.int64)
    np.add.at(out[0], gc[hit & (gc >= 0)], 1)
    np.add.at(out[1], pc[~hit & (pc >= 0)], 1)
    np.add.at(out[2], gc[~hit & (gc >= 0)], 1)
    return out


def boundary_table(pred, gt, C, R, ignore_index=255, gt_slots=None):
    """The table int64 [R+1,5,C] of one predicted map [B,H,W] (values as they are: 255 = no label) against gt [B,H,W]."""
    pred, gt = np.asarray(pred).astype(np.int64), np.asarray(gt).astype(np.int64)
    sg = slots(gt, C, R) if gt_slots is None else gt_slots
    sa = slots(pred, C, R)                                 # over the whole map, ignored pixels included as neighbours
    keep = gt != ignore_index
    pc, gc = class_index(pred, C), class_index(gt, C)
    hit = keep & (pred == gt) & (gc >= 0)
    miss = keep & (pred != gt)
    out = np.zeros((R + 1, 5, C), np.int64)
    np.add.at(out[:, 0], (sg[hit], gc[hit]), 1)
    sel = miss & (pc >= 0)
    np.add.at(out[:, 1], (sg[sel], pc[sel]), 1)
    sel = miss & (gc >= 0)
    np.add.at(out[:, 2], (sg[sel], gc[sel]), 1)
    sel = keep & (pc >= 0)
    np.add.at(out[:, 3], (sa[sel], pc[sel]), 1)
    np.add.at(out[:, 4], (np.maximum(sg, sa)[hit], pc[hit]), 1)
    return out


def boundary_tables(scores, label_maps, gt, C, R, ignore_index=255):
    """int64 [L,R+1,5,C] as `ops.boundary_counts` returns it: score tensors [B,C,H,W] first (arg-max), then label maps."""
    sg = slots(gt, C, R)
    preds = [argmax_first(s) for s in scores] + [np.asarray(m) for m in label_maps]
    return np.stack([boundary_table(p, gt, C, R, ignore_index, sg) for p in preds])


def brute_force_distances(labels, C, R):
    """The definition, pixel by pixel (small maps only)."""
    cls = class_index(labels, C)
    B, H, W = cls.shape
    d = np.full(cls.shape, R + 1, np.int64)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                if cls[b, y, x] < 0:
                    continue
                for qy in range(max(0, y - R), min(H, y + R + 1)):
                    for qx in range(max(0, x - R), min(W, x + R + 1)):
                        q = cls[b, qy, qx]
                        if q >= 0 and q != cls[b, y, x]:
                            d[b, y, x] = min(d[b, y, x], max(abs(qy - y), abs(qx - x)))
    return d


def blocky(shape, values, block, rng):
    """[B,H,W] map of constant block x block squares with values drawn from `values`."""
    B, H, W = shape
    small = np.asarray(values)[rng.integers(0, len(values), (B, (H + block - 1) // block, (W + block - 1) // block))]
    return np.repeat(np.repeat(small, block, 1), block, 2)[:, :H, :W].copy()
