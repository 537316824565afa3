"""HIP-event times of the epoch-summary render (ops.vis_panels, one launch) and of the u8 D2H copy for the shipped target shape
(B = 8 views, 19 classes, 512 x 1024 -> 256 x 256, thirteen panels), beside the time to copy the tensors the reference route
needs (`logits_up`, `teacher_init`, `teacher_aligned`, `teacher_refined`, `frames_aligned`, both frames, labels, `teacher_conf`)
to pinned host memory -- a floor for what a caller pays without the kernel.  Same process, same run; warm-up, repeats, median and
spread reported.

    python tools/vis_bench.py [--repeats 20] [--warmup 3] [--out profiles/vis_panels.md]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "da-sac_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=(512, 1024))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import visualise as V
    B, (H, W), C = args.batch, args.size, 19
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    image, image2 = rnd(B, 3, H, W), rnd(B, 3, H, W)
    gt = torch.randint(0, C, (B, H, W), device="cuda", generator=g)
    outs = {"logits_up": rnd(B, C, H, W), "teacher_init": rnd(B, C, H, W), "teacher_aligned": torch.rand(B, C, H, W, device="cuda", generator=g),
            "teacher_refined": torch.rand(B, C, H, W, device="cuda", generator=g), "teacher_conf": torch.rand(B, 1, H, W, device="cuda", generator=g),
            "teacher_labels": torch.randint(0, C, (B, H, W), device="cuda", generator=g), "frames_aligned": rnd(B, 3, H, W),
            "running_conf": torch.rand(C, device="cuda", generator=g)}
    state = {}

    def render():
        state["rows"] = V.render(image, gt, outs, image2=image2, want_u8=True)[1]
    t_render = timed(render, args.warmup, args.repeats)
    rows = state["rows"]
    host_rows = torch.empty(rows.shape, dtype=rows.dtype, pin_memory=True)
    t_rows = timed(lambda: host_rows.copy_(rows, non_blocking=True), args.warmup, args.repeats)
    moved = [image, image2, gt] + [v for k, v in outs.items() if k != "running_conf"]
    pinned = [torch.empty(t.shape, dtype=t.dtype, pin_memory=True) for t in moved]

    def copy_all():
        for dst, src in zip(pinned, moved):
            dst.copy_(src, non_blocking=True)
    t_ref = timed(copy_all, args.warmup, args.repeats)
    nbytes = sum(t.numel() * t.element_size() for t in moved)
    fmt = lambda ts: "{:.3f} | {:.3f} | {:.3f}".format(statistics.median(ts), min(ts), max(ts))
    lines = ["# Epoch summary panels: render on the device against moving the activations",
             "",
             "`python tools/vis_bench.py --repeats {} --warmup {}` on {} ({}), B = {}, {} classes, {} x {} -> 256 x 256, 13 panels.".format(
                 args.repeats, args.warmup, torch.cuda.get_device_name(0), torch.version.hip, B, C, H, W),
             "HIP-event times in milliseconds over {} repeats after {} warm-up calls.".format(args.repeats, args.warmup),
             "",
             "| step | median | min | max |",
             "|---|---|---|---|",
             "| `visualise.render` (job table upload + ONE launch, float strip + u8 rows) | " + fmt(t_render) + " |",
             "| u8 rows [{}] to pinned host memory ({:.2f} MB) | ".format(", ".join(str(s) for s in rows.shape), rows.numel() / 1e6) + fmt(t_rows) + " |",
             "| the reference route's inputs to pinned host memory ({:.1f} MB) | ".format(nbytes / 1e6) + fmt(t_ref) + " |",
             "",
             "The last row is a floor for the reference route on one rank: its all-gather, softmax, resizing and colour mapping on the",
             "host come on top and were not measured."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
