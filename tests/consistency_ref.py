"""numpy reference of `dasac_view_consistency` (include/dasac_hip.h) in the kernel's own prescribed order, and the exactly summable
lattice its GPU tests draw from.  No test lives here.

Order.  z_t is a float32 sum over the classes in ascending c, the consensus sum a float32 sum over the views in ascending t, both
added one term after another; every arg-max takes the first maximum (strict >).  IEEE addition in a fixed order is
bit-reproducible, so the integer tables agree exactly even on real soft-max outputs -- no tolerance anywhere.  (Both sums start
from +0: the kernel starts from the first term, which differs for a first term of -0 only, and no comparison sees the sign of a
zero.)  Vectorised over pixels; loops over t and c."""
import numpy as np


def view_consistency_ref(aligned, T, cover=0.5):
    """aligned: float32 [N*T, C, ...] -> (agree int64 [C+1,T+1,T+1], flips [C,C], per_view [T,2])."""
    a = np.ascontiguousarray(np.asarray(aligned, dtype=np.float32))
    NT, C = a.shape[:2]
    assert NT % T == 0
    a = a.reshape(NT // T, T, C, -1)
    N, HW = a.shape[0], a.shape[3]
    z = np.zeros((N, T, HW), np.float32)
    best, arg = a[:, :, 0].copy(), np.zeros((N, T, HW), np.int64)
    for c in range(C):
        z = z + a[:, :, c]                                   # float32 + float32, ascending c
        if c:
            gt = a[:, :, c] > best
            best, arg = np.where(gt, a[:, :, c], best), np.where(gt, c, arg)
    cmax, cstar = None, np.zeros((N, HW), np.int64)
    for c in range(C):
        s = np.zeros((N, HW), np.float32)
        for t in range(T):
            s = s + a[:, t, c]                               # ascending t, every view
        if c == 0:
            cmax = s
        else:
            gt = s > cmax
            cmax, cstar = np.where(gt, s, cmax), np.where(gt, c, cstar)
    cov = z >= np.float32(cover)
    hit = cov & (arg == cstar[:, None])
    k, m = cov.sum(1), hit.sum(1)
    agree = np.zeros((C + 1, T + 1, T + 1), np.int64)
    np.add.at(agree, (np.where(k > 0, cstar, C).ravel(), k.ravel(), m.ravel()), 1)
    flips = np.zeros((C, C), np.int64)
    for t in range(T):
        for u in range(t + 1, T):
            both = cov[:, t] & cov[:, u]
            np.add.at(flips, (arg[:, t][both], arg[:, u][both]), 1)
    per_view = np.stack([cov.sum((0, 2)), hit.sum((0, 2))], 1).astype(np.int64)
    return agree, flips, per_view


COVERAGES = (0, 1, 3, 4)          # quarters: 0, 0.25, 0.75, 1 -- none on the cover = 0.5 (or 0.2) boundary


def lattice(rng, N, T, C, H, W, labels=None, coverage=None):
    """float32 [N*T, C, H, W] on an exactly summable lattice: per (view, pixel) a probability vector of integer multiples of 2^-10
    that sums to exactly 1, scaled by a coverage of 0, 1/4, 3/4 or 1 -- every value a multiple of 2^-12 no larger than 1, so every
    float32 sum of up to 32 (or 8) of them is exact in any order.  labels int [N,T,H,W] or None: the class that gets 513 / 1024
    on top of its share of a random split of the rest (it wins outright); None: a random split of all of it (ties happen, the first maximum wins).
    coverage: int quarters [N,T,H,W] or None (random from COVERAGES)."""
    mass = 511 if labels is not None else 1024
    if C > 1:
        cuts = np.sort(rng.integers(0, mass + 1, (N, T, H, W, C - 1)), -1)
        parts = np.diff(np.concatenate([np.zeros_like(cuts[..., :1]), cuts, np.full_like(cuts[..., :1], mass)], -1), axis=-1)
    else:
        parts = np.full((N, T, H, W, 1), mass)
    if labels is not None:
        np.put_along_axis(parts, np.asarray(labels)[..., None], np.take_along_axis(parts, np.asarray(labels)[..., None], -1) + 513, -1)
    assert (parts.sum(-1) == 1024).all()
    if coverage is None:
        coverage = np.asarray(COVERAGES)[rng.integers(0, len(COVERAGES), (N, T, H, W))]
    q = parts * np.asarray(coverage)[..., None]              # integer multiples of 2^-12
    return np.ascontiguousarray(np.moveaxis(q, -1, 2).reshape(N * T, C, H, W).astype(np.float32) / np.float32(4096.0))
