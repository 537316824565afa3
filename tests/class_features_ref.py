"""numpy restatement of the class feature tables' contract (include/dasac_hip.h: dasac_label_nodes, dasac_class_feature_stats),
independent of the kernels: shared by tests/test_class_features_cpu.py and tests/test_gpu_class_features.py."""
import numpy as np

COLUMNS = ("sum", "sumsq")


def node_pixel(i, n_out, n_in):
    """Where align_corners=True upsampling puts node i of n_out on an axis of n_in pixels: i * (n_in - 1) / (n_out - 1), halves
    rounded up, in integers."""
    return (2 * i * (n_in - 1) + (n_out - 1)) // (2 * (n_out - 1)) if n_out > 1 else 0


def label_nodes(lab, h, w, C, r):
    """lab: integer array [N,H,W] (any integer dtype).  uint8 [N,h,w]: the label at the node's pixel if it is a class (0 <= v < C)
    and the whole window of radius r around the pixel, clipped to the image, holds it; 255 otherwise."""
    lab = np.asarray(lab).astype(np.int64)
    N, H, W = lab.shape
    out = np.full((N, h, w), 255, dtype=np.uint8)
    for i in range(h):
        Y = node_pixel(i, h, H)
        for j in range(w):
            X = node_pixel(j, w, W)
            win = lab[:, max(Y - r, 0):min(Y + r, H - 1) + 1, max(X - r, 0):min(X + r, W - 1) + 1].reshape(N, -1)
            v = lab[:, Y, X]
            keep = (v >= 0) & (v < C) & (win == v[:, None]).all(axis=1)
            out[keep, i, j] = v[keep]
    return out


def table(x, nodes, C):
    """x: float array [N,Cf,...], nodes: uint8 [N,...] with as many positions per sample.  Returns (sums float64 [C,Cf,2], counts
    int64 [C], abs_sum float64 [C,Cf] = sum |x| per cell, entries int64 [C] = the values summed into each cell of a class), every x
    widened to float64 first."""
    x = np.asarray(x)
    N, Cf = x.shape[:2]
    xd = x.reshape(N, Cf, -1).astype(np.float64)
    nodes = np.asarray(nodes).reshape(N, -1)
    assert nodes.shape[1] == xd.shape[2]
    sums, counts, abs_sum = np.zeros((C, Cf, 2)), np.zeros(C, dtype=np.int64), np.zeros((C, Cf))
    for c in range(C):
        sel = nodes == c                                            # [N, HW]
        counts[c] = sel.sum()
        if counts[c]:
            picked = np.transpose(xd, (1, 0, 2))[:, sel]            # [Cf, count]
            sums[c, :, 0] = picked.sum(axis=1)
            sums[c, :, 1] = (picked * picked).sum(axis=1)
            abs_sum[c] = np.abs(picked).sum(axis=1)
    return sums, counts, abs_sum, counts.copy()


def blocks(N, H, W, C, seed):
    """int64 [N,H,W] label maps: per image 11 x 7-pixel blocks (height x width) of classes drawn uniformly from [0, C), one 6 x 9
    rectangle of 255 and three pixels of -1."""
    rng = np.random.RandomState(seed)
    out = np.empty((N, H, W), dtype=np.int64)
    for n in range(N):
        coarse = rng.randint(0, C, size=((H + 10) // 11, (W + 6) // 7))
        out[n] = np.repeat(np.repeat(coarse, 11, axis=0), 7, axis=1)[:H, :W]
        y, x = rng.randint(0, max(H - 6, 0) + 1), rng.randint(0, max(W - 9, 0) + 1)
        out[n, y:y + 6, x:x + 9] = 255
        for _ in range(3):
            out[n, rng.randint(0, H), rng.randint(0, W)] = -1
    return out


def kept_share(nodes):
    """share of nodes that keep a class"""
    return float((np.asarray(nodes) != 255).mean())
