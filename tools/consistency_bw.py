"""Streaming rate of `dasac_view_consistency` beside its yardstick, `dasac_confusion_counts` with one score layer (the same kind of
kernel over the same kind of tensor), at the cfg-3 shape (2 groups x 4 views x 19 x 769 x 769) and the cfg-5 shape (2 x 4 x 19 x
512 x 1024): algorithmic bytes (the aligned tensor once, N*T*C*HW*4) / time between two HIP events around a window of 2000 calls, the
kernels' windows alternating, the median of ROUNDS windows each (profiles/view_consistency.md).
Rows per shape: `hot` -- the same tensor call after call, whatever of it the last-level cache keeps is reused; `cold` -- three
tensors in turn, 1 GB between two reads of the same byte, more than any cache holds; each on `smooth` views (up-sampled soft-max
outputs that mostly agree: what a target step sees, merged keys) and on `random` ones (per-pixel random winners per view: every
pixel disagrees, pair-by-pair adds).  Every view has an uncovered border strip of its own, so k varies over the image.
The yardstick reads a [N*T,19,H,W] tensor of the same size against an int64 ground truth.  Afterwards tools/confusion_bw.py runs in
a process of its own on the same device, and its table is printed as it is.
Usage (GPU box): python tools/consistency_bw.py [--no-confusion-bw]"""
import json
import os
import statistics
import subprocess
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "da-sac_amd"))
import torch
from dasac_hip import ops

N, T, C = 2, 4, 19
SHAPES = {"cfg-3": (769, 769), "cfg-5": (512, 1024)}
WINDOW, ROUNDS, COPIES = 2000, 5, 3          # 0.15 s per window


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(WINDOW):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / WINDOW * 1e-3


def views(kind, H, W, gen):
    """[N*T,C,H,W] aligned views: probabilities, zero on a border strip that differs per view."""
    if kind == "smooth":
        h, w = (H + 7) // 8, (W + 7) // 8
        low = torch.randn(N, 1, C, h, w, generator=gen) * 3 + torch.randn(N, T, C, h, w, generator=gen) * 0.5
        _, probs, _ = ops.upsample_softmax(low.flatten(0, 1).cuda(), (H, W), None, want_up=False, want_probs=True)
    else:
        probs = torch.rand(N * T, C, H, W, generator=gen).cuda()
        probs /= probs.sum(1, keepdim=True)
    for t in range(T):
        probs.view(N, T, C, H, W)[:, t, :, : 24 * t] = 0
        probs.view(N, T, C, H, W)[:, t, :, :, W - 16 * (T - 1 - t):] = 0
    return probs


def main():
    gen = torch.Generator().manual_seed(0)
    rows = []
    for shape, (H, W) in SHAPES.items():
        nbytes = N * T * C * H * W * 4
        gt = torch.randint(0, C, (N * T, H, W), generator=gen).cuda()
        for kind in ("smooth", "random"):
            bufs = [views(kind, H, W, gen) for _ in range(COPIES)]
            tables = ops.consistency_tables(C, T, "cuda")
            matrix = torch.zeros(1, C + 1, C + 1, dtype=torch.int64, device="cuda")
            fns = {"hot": lambda i: ops.view_consistency(bufs[0], T, tables),
                   "cold": lambda i: ops.view_consistency(bufs[i % COPIES], T, tables),
                   "yardstick hot": lambda i: ops.confusion_counts([bufs[0]], [], gt, matrix),
                   "yardstick cold": lambda i: ops.confusion_counts([bufs[i % COPIES]], [], gt, matrix)}
            for f in fns.values():
                for i in range(2 * COPIES):
                    f(i)
            torch.cuda.synchronize()
            times = {k: [] for k in fns}
            for _ in range(ROUNDS):                      # alternating windows
                for k, f in fns.items():
                    times[k].append(window(f))
            for mode in ("hot", "cold"):
                t, y = times[mode], times["yardstick " + mode]
                rows.append(dict(shape=shape, views=kind, l2=mode, MB=nbytes / 1e6, us=statistics.median(t) * 1e6, us_min=min(t) * 1e6,
                                 us_max=max(t) * 1e6, yardstick_MB=(nbytes + gt.numel() * 8) / 1e6, yardstick_us=statistics.median(y) * 1e6))
            del bufs
    print("{:8s} {:8s} {:5s} {:>8s} {:>8s} {:>7s} {:>15s} {:>10s} {:>7s} {:>6s}".format(
        "shape", "views", "L2", "MB", "us", "TB/s", "us min..max", "yardstick", "TB/s", "ratio"))
    for r in rows:
        rate, yrate = r["MB"] / r["us"], r["yardstick_MB"] / r["yardstick_us"]
        print("{:8s} {:8s} {:5s} {:8.1f} {:8.1f} {:7.2f} {:7.1f}..{:<7.1f} {:10.1f} {:7.2f} {:6.2f}".format(
            r["shape"], r["views"], r["l2"], r["MB"], r["us"], rate, r["us_min"], r["us_max"], r["yardstick_us"], yrate, rate / yrate))
    print(json.dumps(rows))
    if "--no-confusion-bw" not in sys.argv:
        del gt
        torch.cuda.empty_cache()
        sys.stdout.flush()
        print("--- tools/confusion_bw.py, a process of its own ---", flush=True)
        subprocess.run([sys.executable, os.path.join(ROOT, "tools", "confusion_bw.py")], check=True)


if __name__ == "__main__":
    main()
