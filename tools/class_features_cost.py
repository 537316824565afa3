"""What the class feature tables cost (dasac_label_nodes + dasac_class_feature_stats; `driver.class_features`).
Usage (GPU box): python tools/class_features_cost.py [--iters N] [--repeats R] [--json PATH]

Two tensors: the cfg-3 teacher pass's classifier input [16, 2048, 65, 129] (1.1 GB, past the 256 MB Infinity Cache) and one
Cityscapes frame's [1, 2048, 129, 257] (272 MB).  Label maps at 8 x the feature resolution made of 64 x 64-pixel regions; per
sample the regions draw from `k` classes: k = 6 (a crop holds a handful) and k = 19 (every class present in every sample: the
worst case for the present-class mask).  Per case: `iters` calls between device events after 3 warm-up calls, `repeats` figures,
for ops.label_nodes (radius 2), ops.class_feature_stats and, on the same tensor in the same process, ops.activation_stats.
Bytes are counted from the shapes: x once, 4 bytes per element."""
import argparse
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "da-sac_amd"))
import torch

from dasac_hip import ops


def dev_time(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us


def region_labels(N, H, W, k, gen):
    """int64 [N,H,W]: 64 x 64-pixel regions, sample n drawing from k of the 19 classes; a 16-pixel border of 255."""
    gh, gw = (H + 63) // 64, (W + 63) // 64
    palette = torch.stack([torch.randperm(19, device="cuda", generator=gen)[:k] for _ in range(N)])          # [N, k]
    pick = torch.randint(0, k, (N, gh * gw), device="cuda", generator=gen)
    coarse = torch.gather(palette, 1, pick).view(N, gh, gw)
    lab = coarse.repeat_interleave(64, 1).repeat_interleave(64, 2)[:, :H, :W].contiguous()
    lab[:, :16], lab[:, -16:], lab[:, :, :16], lab[:, :, -16:] = 255, 255, 255, 255
    return lab


def main():
    assert torch.cuda.is_available(), "class_features_cost.py measures on the MI355X"
    gen = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for name, (N, Cf, h, w) in [("cfg-3 teacher pass 16x2048x65x129", (16, 2048, 65, 129)), ("Cityscapes frame 1x2048x129x257", (1, 2048, 129, 257))]:
        x = torch.randn((N, Cf, h, w), device="cuda", generator=gen).relu_()
        gb = x.numel() * 4 / 1e9
        t_act = [dev_time(lambda: ops.activation_stats([x]), args.iters) for _ in range(args.repeats)]
        for k in (6, 19):
            lab = region_labels(N, 8 * (h - 1) + 1, 8 * (w - 1) + 1, k, gen)
            t_nodes = [dev_time(lambda: ops.label_nodes(lab, (h, w), 19, 2), args.iters) for _ in range(args.repeats)]
            nodes = ops.label_nodes(lab, (h, w), 19, 2)
            table = ops.ClassFeatureTable.zeros(19, Cf, x.device)
            t_cf = [dev_time(lambda: ops.class_feature_stats(x, nodes, 19, table), args.iters) for _ in range(args.repeats)]
            kept = float((nodes != 255).float().mean())
            present = float(torch.stack([(nodes[n].view(-1, 1) == torch.arange(19, device="cuda")).any(0).sum() for n in range(N)]).float().mean())
            rows.append(dict(case=name, classes_drawn=k, classes_present_per_sample=round(present, 2), nodes_kept=round(kept, 3), gb=round(gb, 4),
                             label_nodes_us=[round(t, 1) for t in t_nodes], class_feature_stats_us=[round(t, 1) for t in t_cf],
                             activation_stats_us=[round(t, 1) for t in t_act], class_feature_stats_tb_per_s=round(gb / min(t_cf) * 1e3, 3),
                             activation_stats_tb_per_s=round(gb / min(t_act) * 1e3, 3)))
            print("{:<36} k={:<2} present/sample {:5.2f} kept {:.3f} | label_nodes {} us | class_feature_stats {} us = {:.3f} TB/s | "
                  "activation_stats {} us = {:.3f} TB/s".format(name, k, present, kept, "  ".join("%.1f" % t for t in t_nodes),
                                                                "  ".join("%.1f" % t for t in t_cf), gb / min(t_cf) * 1e3,
                                                                "  ".join("%.1f" % t for t in t_act), gb / min(t_act) * 1e3), flush=True)
        del x
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=args.iters, rows=rows), f, indent=1)


if __name__ == "__main__":
    main()
