"""Time of ops.infer_fuse at a full Cityscapes frame (1 x 19 x 1024 x 2048) from six sources -- the low-resolution logits the
ResNet-101 backbone (stride 8) produces for the scales 0.5 / 0.75 / 1.0, plain and mirrored -- against the ATen composition on
the same device and tensors (interpolate + flip + softmax + add + argmax), and of ops.image_pyramid for the three scales.
Algorithmic bytes (every source read once, every output written once) / time.  The two sides are timed alternately, `--rounds`
times, and every round is printed: the spread is part of the result.  Usage (GPU box): python tools/infer_fused_bw.py"""
import argparse
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "da-sac_amd"))
import torch
import torch.nn.functional as F
from dasac_hip import ops
import driver


def low_size(n):
    """Stride-8 extent of the ResNet-101 DeepLabv2 backbone: 7x7/2 conv (pad 3), 3x3/2 max-pool (pad 1, ceil_mode), one stride-2
    stage (769 -> 97)."""
    n = (n - 1) // 2 + 1
    n = -(-(n - 1) // 2) + 1
    return (n - 1) // 2 + 1


def timeit(fn, iters):
    fn(); fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e-3


def aten_fuse(sources, flips, size, want_conf):
    acc = None
    for x, flip in zip(sources, flips):
        p = F.interpolate(x, size=size, mode="bilinear", align_corners=True)
        if flip:
            p = p.flip(-1)
        p = p.softmax(1)
        acc = p if acc is None else acc.add_(p)
    if want_conf:
        conf, lab = acc.max(1)
        return lab.to(torch.uint8), conf / len(sources)
    return acc.argmax(1).to(torch.uint8), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=19)
    ap.add_argument("--scales", type=float, nargs="+", default=[0.5, 0.75, 1.0])
    ap.add_argument("--iters", type=int, default=200, help="fused launches per timed window")
    ap.add_argument("--aten-iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement on the MI355X; there is nothing to time without it"
    H, W, C = args.height, args.width, args.classes
    g = torch.Generator().manual_seed(0)
    sources, flips, shapes = [], [], []
    for s in args.scales:
        Hs, Ws = driver.scaled_size(H, W, s)
        both = (torch.randn(2, C, low_size(Hs), low_size(Ws), generator=g) * 3).cuda()       # one 2B-batch backbone output per scale
        sources += [both[:1], both[1:]]
        flips += [False, True]
        shapes.append(((Hs, Ws), tuple(both.shape[-2:])))
    P, S = H * W, len(sources)
    src_bytes = sum(x.numel() * 4 for x in sources)
    print("output 1 x {} x {} x {}, {} sources: {}".format(C, H, W, S, ", ".join("{}x{} -> {}x{}".format(*a, *b) for a, b in shapes)))

    # the two sides compute the same thing at the timed size
    lab, conf, probs = ops.infer_fuse(sources, flips, (H, W), "mean", want_conf=True, want_probs=True)
    lab_a, conf_a = aten_fuse(sources, flips, (H, W), True)
    print("fused vs ATen at this size: labels differ at {:.2e} of the pixels, max |conf - conf_aten| {:.2e}".format(
        float((lab != lab_a).float().mean()), float((conf - conf_a).abs().max())))
    del probs, lab_a, conf_a

    cases = [("labels", False, False, P), ("labels + conf", True, False, 5 * P), ("labels + conf + probs", True, True, (5 + 4 * C) * P)]
    print("{:30s} {:>6s} {:>9s} {:>10s} {:>8s} {:>6s} {:>11s} {:>8s}".format("case", "round", "MB", "fused us", "TB/s", "of 8", "ATen us", "ratio"))
    for name, want_conf, want_probs, out_bytes in cases:
        nbytes = src_bytes + out_bytes
        for r in range(args.rounds):
            t = timeit(lambda: ops.infer_fuse(sources, flips, (H, W), "mean", None, want_conf, want_probs), args.iters)
            # the ATen side keeps its fused probabilities anyway: `probs` costs it nothing more
            ta = timeit(lambda: aten_fuse(sources, flips, (H, W), want_conf), args.aten_iters)
            print("{:30s} {:6d} {:9.1f} {:10.1f} {:8.3f} {:5.1f}% {:11.1f} {:7.1f}x".format(
                name, r, nbytes / 1e6, t * 1e6, nbytes / t / 1e12, 100 * nbytes / t / 8e12, ta * 1e6, ta / t))
    t = timeit(lambda: ops.infer_fuse(sources, flips, (H, W), "max"), args.iters)
    print("{:30s} {:6d} {:9.1f} {:10.1f} {:8.3f} {:5.1f}%".format("labels, mode max", 0, (src_bytes + P) / 1e6, t * 1e6,
                                                                 (src_bytes + P) / t / 1e12, 100 * (src_bytes + P) / t / 8e12))
    one = sources[-2]
    t1 = timeit(lambda: ops.infer_labels(one, (H, W)), args.iters)
    tf = timeit(lambda: ops.infer_fuse([one], [False], (H, W)), args.iters)
    print("one source: infer_labels {:.1f} us, infer_fuse {:.1f} us".format(t1 * 1e6, tf * 1e6))

    image = torch.randn(1, 3, H, W, generator=g).cuda()
    for s in args.scales:
        Hs, Ws = driver.scaled_size(H, W, s)
        nbytes = (3 * P + 2 * 3 * Hs * Ws) * 4
        t = timeit(lambda: ops.image_pyramid(image, (Hs, Ws), True), args.iters)

        def aten_pyramid():
            y = F.interpolate(image, size=(Hs, Ws), mode="bilinear", align_corners=True)
            return torch.cat([y, y.flip(-1)])
        ta = timeit(aten_pyramid, args.aten_iters)
        print("image_pyramid {:4d}x{:4d} + mirror {:9.1f} MB {:9.1f} us {:6.3f} TB/s   ATen interpolate + flip + cat {:9.1f} us".format(
            Hs, Ws, nbytes / 1e6, t * 1e6, nbytes / t / 1e12, ta * 1e6))


if __name__ == "__main__":
    main()
