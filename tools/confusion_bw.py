"""Streaming rate of `dasac_confusion_counts` beside its yardstick, `dasac_mask_counts` of the same library in the same process, at
the cfg-3 shape (8 crops, 19 classes, 769x769): algorithmic bytes (each operand once) / time between two HIP events around a
window of 200 calls, the two kernels' windows alternating, the median of ROUNDS windows each (profiles/confusion_counts.md).
Rows: one score layer; three score layers + one label map; the same with the reliability tables at 16 bins; one label map alone
as int64 and as uint8 -- each on random maps (scattered keys) and on blocky ones (large regions, mostly right: what validation sees).
Usage (GPU box): python tools/confusion_bw.py"""
import json
import os
import statistics
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "da-sac_amd"))
import torch
from dasac_hip import ops

B, C, h, H = 8, 19, 97, 769
WINDOW, ROUNDS, BINS = 200, 5, 16
T = B * C * H * H * 4            # one [8,19,769,769] fp32 tensor
P = B * H * H


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(WINDOW):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / WINDOW * 1e-3


def blocks(values, size, gen):
    n = (H + size - 1) // size
    small = values[torch.randint(0, len(values), (B, n, n), generator=gen)]
    return small.repeat_interleave(size, 1).repeat_interleave(size, 2)[:, :H, :H].contiguous().cuda()


gen = torch.Generator().manual_seed(0)
low = [torch.randn(B, C, h, h, generator=gen).cuda() * 3 for _ in range(2)]
up, probs, _ = ops.upsample_softmax(low[0], (H, H), None, want_probs=True)
up2, _, _ = ops.upsample_softmax(low[1], (H, H), None)
pred = up.argmax(1)
maps = {}
# random: per-pixel random ground truth and labels -- predictions mostly wrong, neighbouring keys differ
y = torch.randint(0, C, (B, H, H), generator=gen).cuda()
lab = torch.randint(0, C, (B, H, H), generator=gen).cuda()
lab[torch.rand(B, H, H, generator=gen).cuda() < 0.4] = 255
maps["random"] = (y, lab)
# blocky: the ground truth is the first layer's own prediction with a fifth of its 64 x 64 blocks replaced by one class or ignored;
# the label map is that prediction with its least confident 40 % rejected
swap = blocks(torch.cat([torch.full((16,), -2), torch.arange(C)[:3], torch.tensor([255])]), 64, gen)
y = torch.where(swap == -2, pred, swap)
conf = probs.max(1)[0]
sample = conf.flatten()[::97]
lab = torch.where(conf < sample.kthvalue(int(0.4 * sample.numel()))[0], torch.full_like(pred, 255), pred)
maps["blocky"] = (y, lab)
del swap, conf, sample

rows = []


def row(name, nbytes, yardstick, fn):
    for f in (yardstick, fn):
        f(); f()
    torch.cuda.synchronize()
    ty, tf = [], []
    for _ in range(ROUNDS):                      # alternating windows
        ty.append(window(yardstick))
        tf.append(window(fn))
    rows.append(dict(name=name, MB=nbytes / 1e6, yardstick_us=statistics.median(ty) * 1e6, us=statistics.median(tf) * 1e6,
                     us_min=min(tf) * 1e6, us_max=max(tf) * 1e6))


for kind, (y, lab) in maps.items():
    lab8 = lab.to(torch.uint8)
    scores3 = [up, probs, up2]
    mc1, mc4, mcm = (torch.zeros(n, 3, C, dtype=torch.int64, device="cuda") for n in (1, 4, 1))
    cf1, cf4, cfm = (torch.zeros(n, C + 1, C + 1, dtype=torch.int64, device="cuda") for n in (1, 4, 1))
    rel = torch.zeros(3, C, BINS, 2, dtype=torch.int64, device="cuda")
    row(kind + ": 1 score layer", T + P * 8, lambda: ops.mask_counts([up], [], y, mc1), lambda: ops.confusion_counts([up], [], y, cf1))
    row(kind + ": 3 score layers + 1 label map", 3 * T + P * 16, lambda: ops.mask_counts(scores3, [lab], y, mc4),
        lambda: ops.confusion_counts(scores3, [lab], y, cf4))
    row(kind + ": 3 + 1 with reliability, 16 bins", 3 * T + P * 16, lambda: ops.mask_counts(scores3, [lab], y, mc4),
        lambda: ops.confusion_counts(scores3, [lab], y, cf4, rel, logits_layers=[0, 2]))
    row(kind + ": 1 label map, int64", P * 16, lambda: ops.mask_counts([], [lab], y, mcm), lambda: ops.confusion_counts([], [lab], y, cfm))
    row(kind + ": 1 label map, uint8", P * 9, lambda: ops.mask_counts([], [lab], y, mcm), lambda: ops.confusion_counts([], [lab8], y, cfm))

print("{:46s} {:>8s} {:>10s} {:>8s} {:>7s} {:>6s} {:>15s}".format("row", "MB", "yardstick", "us", "TB/s", "ratio", "us min..max"))
for r in rows:
    print("{:46s} {:8.1f} {:10.1f} {:8.1f} {:7.2f} {:6.2f} {:7.1f}..{:.1f}".format(
        r["name"], r["MB"], r["yardstick_us"], r["us"], r["MB"] / r["us"], r["us"] / r["yardstick_us"], r["us_min"], r["us_max"]))
print(json.dumps(rows))
