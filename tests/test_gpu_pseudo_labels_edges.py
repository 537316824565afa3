"""Pseudo-label extraction (pseudo_labels.hip: pl_argmax_peaks<19>, pl_argmax_peaks<0>, pl_threshold) at its edges, bit for bit
against oracle.head_ref.pseudo_labels on the CPU: labels, max_conf and max_idx, with and without `disc`, with and without
`ignore`.

Inputs are QUANTISED probabilities, multiples of 1/16 that sum to 1 in every pixel (C = 1 cannot be normalised and tied at once:
its single plane takes 16, 9, 8 or 4 sixteenths), so that exact ties are frequent: two-way ties, ties between class 0 and the last
class, three- and four-way ties (C >= 4).  The reference's own tie rule is pinned first, on the CPU: on every input used here its
max_idx equals numpy.argmax over the class axis (the first maximum).  At least a quarter of the pixels of every C >= 2 are ties
(a condition on the generator, counted on the CPU).

Threshold ties: upper = 1.0 without disc makes every pixel that IS its (image, class) peak sit exactly on its threshold, and the
strict compare must drop it (no pixel survives); upper = 0.5 with planted pixels (class 0: 16/16, 8/16 tied with the last class,
9/16) has, in every case of HW >= 1023, a pixel with m == thr exactly and one a sixteenth above (counted on the CPU).  Also: classes
that never win in an image (peak 0, thr = lower), an image where everything is ignored, a pixel whose probabilities are all zero.

Shapes: HW in {1, 2, 3, 4, 5, 6, 7, 1023, 1024, 1026} (HW % 4 = 0..3; odd HW puts image and plane bases on every 4-byte phase)
x B in {1, 3} x C in {1, 2, 3, 4, 5, 19, 20, 64}; C = 19 takes pl_argmax_peaks<19>, the others <0>.  C = 65 is refused, a workspace
one byte short is DASAC_EWORKSPACE, want_idx=False returns the same labels and confidences.  (lower = 0 is refused in
test_gpu_pseudo_labels.py.)  The second grid pass of the quad kernel (grid cap 4096 blocks of 1024 pixels over the batch) runs at
B = 1, HW = 4096*1024 + 6 with C = 2 and C = 19 on continuous device-generated probabilities without ties, against torch's
max / scatter_reduce(amax) / threshold composition on the device.

Everything is an equality: no tolerance, no ratio.  On the MI355X every case matched; tie pixels were 34 % (C = 3, 4) to 50 %
(C = 2, 19, 64) of the 12404 pixels of every C >= 2.  Both second-pass cases take well under a second."""
import numpy as np
import pytest
import torch

from oracle import head_ref as H

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (3, 1), (2, 2), (1, 5), (2, 3), (7, 1), (33, 31), (32, 32), (27, 38)]
CS = [1, 2, 3, 4, 5, 19, 20, 64]
LOWER = 0.2
TIE_PATTERNS = [[8, 8], [6, 6, 4], [4, 4, 4, 4], [5, 5, 5, 1], [4, 4, 4, 2, 2]]
UNIQUE_PATTERNS = [[16], [9, 7], [10, 6], [15, 1], [7, 5, 4], [8, 4, 2, 2]]
EWORKSPACE = -2


def quantised(B, C, Hh, W, seed):
    """[B,C,H,W] fp32 multiples of 1/16.  Half of the pixels take a tie pattern; in 30 % of the pixels the first two slots of the
    pattern go to class 0 and the last class.  HW >= 8: class 1 has no mass in image 0 (C >= 3), pixel 0 of image 0 is all zero,
    and pixels 1, 2, 3 of every image give class 0 the values 16/16, 8/16 (tied with the last class) and 9/16."""
    rng = np.random.RandomState(seed)
    P = B * Hh * W
    if C == 1:
        units = rng.choice([16, 9, 8, 4], size=(P, 1)).astype(np.int64)
    else:
        ties = [p for p in TIE_PATTERNS if len(p) <= C]
        uniq = [p for p in UNIQUE_PATTERNS if len(p) <= C]
        pats = ties + uniq
        which = np.where(rng.rand(P) < 0.5, rng.randint(0, len(ties), P), len(ties) + rng.randint(0, len(uniq), P))
        keys = rng.rand(P, C)
        forced = rng.rand(P) < 0.3
        first_is_last = forced & (rng.rand(P) < 0.5)
        keys[forced, 0], keys[forced, C - 1] = -2.0, -1.0
        keys[first_is_last, 0], keys[first_is_last, C - 1] = -1.0, -2.0
        perm = np.argsort(keys, axis=1)
        units = np.zeros((P, C), np.int64)
        for i, pat in enumerate(pats):
            rows = np.flatnonzero(which == i)
            for j, u in enumerate(pat):
                units[rows, perm[rows, j]] = u
        assert (units.sum(1) == 16).all()
    units = units.reshape(B, Hh * W, C)
    if Hh * W >= 8:
        if C >= 3:                                                # class 1 never wins in image 0: its mass goes to class 2
            units[0, :, 2] += units[0, :, 1]
            units[0, :, 1] = 0
        units[0, 0, :] = 0
        for b in range(B):
            units[b, 1:4, :] = 0
            units[b, 1, 0], units[b, 2, 0], units[b, 3, 0] = 16, 8, 9
            if C > 1:
                units[b, 2, C - 1], units[b, 3, C - 1] = 8, 7
    probs = (units.astype(np.float32) / np.float32(16)).transpose(0, 2, 1).reshape(B, C, Hh, W)
    return torch.from_numpy(np.ascontiguousarray(probs))


def _disc(C, seed):
    g = torch.Generator().manual_seed(seed)
    d = torch.tensor([1.0, 0.5, 0.75, 0.875])[torch.randint(0, 4, (C,), generator=g)]
    d[0] = 1.0
    return d


def _run(probs, ignore, upper, lower, disc, want_idx=True):
    from dasac_hip import ops
    lab, conf, idx = ops.pseudo_labels(probs.cuda(), None if ignore is None else ignore.cuda(), upper, lower,
                                       None if disc is None else disc.cuda(), want_idx=want_idx)
    return lab.cpu(), conf.cpu(), None if idx is None else idx.cpu()


def _ref(probs, ignore, upper, lower, disc):
    B, _, Hh, W = probs.shape
    return H.pseudo_labels(probs, ignore if ignore is not None else torch.zeros(B, Hh, W, dtype=torch.bool), upper, lower, disc)


def _threshold_of_pixel(probs, upper, lower, disc):
    """(m, thr of the winning class) per pixel, restated with numpy (used only for the conditions on the generator)"""
    p = probs.numpy()
    B, C = p.shape[:2]
    m, k = p.max(1).reshape(B, -1), p.argmax(1).reshape(B, -1)
    peak = np.zeros((B, C), np.float32)
    for b in range(B):
        np.maximum.at(peak[b], k[b], m[b])
    thr = peak * np.float32(upper)
    if disc is not None:
        thr = thr * disc.numpy()[None, :]
    thr = np.maximum(thr, np.float32(lower))
    return m, np.take_along_axis(thr, k, 1), peak


@pytest.mark.parametrize("C", CS)
def test_quantised_ties_bit_exact_vs_oracle(C):
    pixels = tie_pixels = ends_tie = multi_tie = 0
    for Hh, W in SHAPES:
        for B in (1, 3):
            what = (C, B, Hh, W)
            probs = quantised(B, C, Hh, W, seed=1000 * C + 10 * Hh + W + B)
            g = torch.Generator().manual_seed(C + Hh * W + B)
            ignore = torch.rand(B, Hh, W, generator=g) < 0.15
            if B == 3:
                ignore[2] = True                                  # an image where everything is ignored
            disc = _disc(C, C + B)
            # the reference's tie rule: the first maximum
            _, _, ri = _ref(probs, None, 0.5, LOWER, None)
            assert np.array_equal(ri[:, 0].numpy(), probs.numpy().argmax(1)), what
            at_max = (probs == probs.max(1, keepdim=True)[0]).sum(1)
            pixels += at_max.numel()
            tie_pixels += int((at_max >= 2).sum())
            multi_tie += int((at_max >= 3).sum())
            if C > 1:
                ends_tie += int(((probs[:, 0] == probs.max(1)[0]) & (probs[:, C - 1] == probs.max(1)[0])).sum())
            for d in (disc, None):
                if Hh * W >= 1023:                                # conditions on the generator, on the CPU
                    m, thr, peak = _threshold_of_pixel(probs, 0.5, LOWER, d)
                    assert ((m == thr) & (m > 0)).any() and (m == thr + np.float32(1 / 16)).any(), what
                    assert C < 3 or peak[0, 1] == 0, what         # a class that never wins in an image
                for ign in (ignore, None):
                    got = _run(probs, ign, 0.5, LOWER, d)
                    ref = _ref(probs, ign, 0.5, LOWER, d)
                    for name, a, r in zip(("labels", "max_conf", "max_idx"), got, ref):
                        assert a.dtype == r.dtype and torch.equal(a, r), (what, name, d is not None, ign is not None)
            # upper = 1: every peak pixel sits exactly on its threshold and is dropped, so nothing survives
            lab, conf, idx = _run(probs, None, 1.0, LOWER, None)
            rl, rc, rk = _ref(probs, None, 1.0, LOWER, None)
            assert torch.equal(lab, rl) and torch.equal(conf, rc) and torch.equal(idx, rk), what
            assert (rl == 255).all(), what
            # without max_idx: the same labels and confidences
            lab2, conf2, none = _run(probs, ignore, 0.5, LOWER, disc, want_idx=False)
            lab1, conf1, _ = _ref(probs, ignore, 0.5, LOWER, disc)
            assert none is None and torch.equal(lab2, lab1) and torch.equal(conf2, conf1), what
    print("pseudo labels C={}: {} pixels, {:.1%} ties, {} ties of class 0 with the last class, {} ties of three or more".format(
        C, pixels, tie_pixels / pixels, ends_tie, multi_tie))
    if C >= 2:
        assert tie_pixels >= pixels / 4 and ends_tie > 0
    if C >= 4:
        assert multi_tie > 0


def test_kept_and_dropped_on_both_sides_of_the_threshold():
    """The planted pixels, spelled out: with upper = 0.5, class 0 has peak 1 and threshold 0.5 in every image; the pixel at
    8/16 (tied with the last class, so class 0 wins it) is dropped, the pixel at 9/16 is kept."""
    for C in (2, 19, 20):
        probs = quantised(3, C, 27, 38, seed=C)
        lab, conf, idx = _run(probs, None, 0.5, LOWER, None)
        lab, conf, idx = lab.view(3, -1), conf.view(3, -1), idx.view(3, -1)
        assert (idx[:, 1:4] == 0).all()
        assert torch.equal(conf[:, 1:4], torch.tensor([[1.0, 0.5, 0.5625]] * 3))
        assert (lab[:, 1] == 0).all() and (lab[:, 2] == 255).all() and (lab[:, 3] == 0).all()
        assert lab[0, 0] == 255 and conf[0, 0] == 0 and idx[0, 0] == 0          # the all-zero pixel


def test_refusals_happen_on_the_host():
    from dasac_hip import ops, DasacError, lib as L
    lib = L.load()
    with pytest.raises(DasacError):
        ops.pseudo_labels(torch.rand(1, 65, 2, 2, device="cuda"), None, 0.75, LOWER)
    B, C, HW = 2, 19, 37
    need = lib.dasac_pseudo_labels_workspace(B, C, HW)
    probs = quantised(B, C, 1, HW, seed=4).cuda()
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    labels = torch.full((B * HW + 8,), -7, dtype=torch.int64, device="cuda")
    conf = torch.full((B * HW + 8,), float("nan"), dtype=torch.float32, device="cuda")
    idx = torch.full((B * HW + 8,), -7, dtype=torch.int64, device="cuda")
    call = lambda nbytes: lib.dasac_pseudo_labels(probs.data_ptr(), None, None, 0.5, LOWER, B, C, HW, labels.data_ptr(), conf.data_ptr(),
                                                 idx.data_ptr(), ws.data_ptr(), nbytes, L.stream_ptr())
    assert call(need - 1) == EWORKSPACE
    torch.cuda.synchronize()
    assert (labels == -7).all() and torch.isnan(conf).all() and (idx == -7).all()
    # exactly enough: runs, equals the oracle and writes nothing behind B*HW
    assert call(need) == 0
    torch.cuda.synchronize()
    rl, rc, ri = _ref(probs.cpu(), None, 0.5, LOWER, None)
    assert torch.equal(labels[:B * HW].cpu(), rl.view(-1)) and torch.equal(conf[:B * HW].cpu(), rc.view(-1))
    assert torch.equal(idx[:B * HW].cpu(), ri.view(-1))
    assert (labels[B * HW:] == -7).all() and torch.isnan(conf[B * HW:]).all() and (idx[B * HW:] == -7).all()


@pytest.mark.parametrize("C", [2, 19])
def test_second_grid_pass_of_the_quad_kernel(C):
    """B = 1, HW = 4096 * 1024 + 6: the quad kernel's grid is capped at 4096 blocks of 1024 pixels, so the last six pixels (one
    whole quad and a partial one of two) are reached only in a block's second pass."""
    from dasac_hip import ops
    Hh, W = 2, (4096 * 1024 + 6) // 2
    g = torch.Generator(device="cuda").manual_seed(5 + C)
    probs = torch.softmax(torch.randn(1, C, Hh, W, device="cuda", generator=g) * 3, 1)
    m, k = probs.max(1, keepdim=True)
    assert int(((probs == m).sum(1) > 1).sum()) == 0              # continuous inputs: no ties (a condition on the generator)
    lab, conf, idx = ops.pseudo_labels(probs, None, 0.75, LOWER, None, want_idx=True)
    assert torch.equal(conf, m) and torch.equal(idx, k)
    peak = torch.zeros(1, C, device="cuda").scatter_reduce_(1, k.view(1, -1), m.view(1, -1), reduce="amax")
    thr = (peak * 0.75).clamp_min(LOWER).gather(1, k.view(1, -1)).view_as(m)
    want = torch.where(m > thr, k, torch.full_like(k, 255))[:, 0]
    assert torch.equal(lab, want)
    tail = lab.view(-1)[-6:]
    assert torch.equal(tail, want.view(-1)[-6:]) and int((lab != 255).sum()) > 0
