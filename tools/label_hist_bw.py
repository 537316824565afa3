"""Device time of dasac_label_hist next to the ATen composition a user would write without it, and the cost of the class
statistics inside driver.compute_sample_weights.  Usage (GPU box): python tools/label_hist_bw.py [--iters N] [--json PATH]

    kernel   ops.label_hist on 8x1024x2048 and 8x769x769 uint8 label maps: (a) uniform-random values 0..255, (b) the
             contention cases -- one constant value, and a blocky realistic map (the g18 label maps, nearest-upsampled);
             64x1024x2048 (128 MB) as well: a call on 8 images takes about as long as the host needs to issue it, so the
             streaming rate of the kernel itself only shows on the larger batch
    aten     torch.bincount(x.view(-1).long() + 256 * image_index, minlength=256 * B) on the same inputs, same run
    stage 2  wall time per image of driver.compute_sample_weights (DeepLabv2-ResNet101, synthetic weights, 1024x2048,
             batches of 2) next to the same loop with infer_label_maps alone

A 16 MB batch sits in the last-level cache when it is read again and again, so every timed call reads ANOTHER buffer of a
ring larger than that cache (`--ring-mb`, default 512): the rates are HBM rates.  Time per call from device events around
`iters` calls after warm-up, repeated `--repeats` times: median, min and max over the repeats.  Algorithmic bytes: the
label bytes, read once (the 2 KiB of counts per image are noise).  Results are compared with the ATen counts before
anything is timed."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "da-sac_amd"))
import numpy as np
import torch

from dasac_hip import ops


def dev_times(fn, iters, repeats, warmup=3):
    """us per call: [repeats] figures, each from device events around `iters` calls"""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    out, k = [], warmup
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn(k)
            k += 1
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters * 1e3)
    return out


def stats(us):
    return {"us_median": round(float(np.median(us)), 2), "us_min": round(float(min(us)), 2), "us_max": round(float(max(us)), 2)}


def blocky(B, H, W):
    g = np.load(os.path.join(ROOT, "tests", "golden", "g18_is_sampling.npz"))
    maps = [g["labels%d" % n] for n in range(len(g["names"]))]
    out = np.empty((B, H, W), np.uint8)
    for b in range(B):
        m = maps[(b * 5 + 1) % len(maps)]
        out[b] = m[(np.arange(H) * m.shape[0] // H)[:, None], (np.arange(W) * m.shape[1] // W)[None, :]]
    return torch.from_numpy(out)


def make(kind, B, H, W, seed):
    if kind == "uniform":
        return torch.randint(0, 256, (B, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    if kind == "constant":
        return torch.full((B, H, W), 13, dtype=torch.uint8)
    return blocky(B, H, W)


def aten_counts(x, offsets):
    return torch.bincount(x.view(-1).long() + offsets, minlength=256 * x.shape[0])


def kernel_rows(args):
    rows = []
    for B, H, W in ((8, 1024, 2048), (8, 769, 769), (64, 1024, 2048)):
        nbytes = B * H * W
        ring = max(2, (args.ring_mb << 20) // nbytes)
        offsets = (torch.arange(B, device="cuda") * 256).repeat_interleave(H * W)
        base = {}
        for kind in ("uniform", "constant", "blocky"):
            host = make(kind, B, H, W, 1)
            # a ring of distinct buffers with the same content statistics (rolled copies: same histogram, other addresses)
            bufs = [torch.roll(host, shifts=r, dims=0).cuda() if kind != "uniform" else make(kind, B, H, W, r).cuda() for r in range(ring)]
            counts = torch.zeros((B, 256), dtype=torch.int64, device="cuda")
            got = ops.label_hist(bufs[0])
            assert torch.equal(got.view(-1), aten_counts(bufs[0], offsets)), "label_hist differs from torch.bincount"
            ours = dev_times(lambda i: ops.label_hist(bufs[i % ring], counts), args.iters, args.repeats)
            aten = dev_times(lambda i: aten_counts(bufs[i % ring], offsets), max(2, args.iters // 4), args.repeats)
            row = {"name": "{}x{}x{} {}".format(B, H, W, kind), "bytes": nbytes, "ring_buffers": ring,
                   "label_hist": stats(ours), "aten_bincount": stats(aten)}
            row["label_hist"]["tbps"] = round(nbytes / np.median(ours) / 1e6, 3)
            row["aten_bincount"]["tbps"] = round(nbytes / np.median(aten) / 1e6, 3)
            row["speedup_vs_aten"] = round(float(np.median(aten) / np.median(ours)), 2)
            base[kind] = float(np.median(ours))
            row["time_vs_uniform"] = round(base[kind] / base["uniform"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del bufs
    return rows


def stage2_row(args):
    import torch.nn as nn
    import bench
    import driver
    import models
    net = models.get_model(bench.model_cfg(), 0, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    driver.init_synthetic_weights(net, seed=0)
    net.cuda().eval()
    n, bs = args.stage2_images, 2
    images = torch.randn(n, 3, 1024, 2048, generator=torch.Generator().manual_seed(0)).cuda()
    batches = lambda: ((images[i:i + bs], list(range(i, min(i + bs, n)))) for i in range(0, n, bs))

    def with_stats():
        return driver.compute_sample_weights(net, batches(), n)

    def maps_only():
        last = None
        for x, _ in batches():
            last = driver.infer_label_maps(net, x)[0]
        return last.cpu()

    def wall(fn):
        fn()
        out = []
        for _ in range(args.repeats):
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) / n * 1e3)
        return {"ms_per_image_median": round(float(np.median(out)), 3), "ms_per_image_min": round(min(out), 3),
                "ms_per_image_max": round(max(out), 3)}
    a, b, a2 = wall(maps_only), wall(with_stats), wall(maps_only)
    row = {"name": "stage 2, deeplabv2_resnet101 1024x2048, {} images in batches of {}".format(n, bs),
           "infer_label_maps": a, "compute_sample_weights": b, "infer_label_maps_again": a2}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--ring-mb", type=int, default=512)
    ap.add_argument("--stage2-images", type=int, default=8, help="0 skips the stage-2 rows")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "label_hist_bw.py needs the MI355X"
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "iters": args.iters, "repeats": args.repeats,
           "ring_mb": args.ring_mb, "rows": kernel_rows(args)}
    if args.stage2_images:
        out["stage2"] = stage2_row(args)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
