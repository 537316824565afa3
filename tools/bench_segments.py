"""Times of the segment ops (`ops.label_segments`, `ops.segment_counts` with one score and one label layer, `ops.segment_filter`) on
one 1024 x 2048 frame and on 16 crops of 769 x 769, 19 classes (profiles/segment_tables.md): HIP events around single calls after
WARMUP calls, the median of RUNS calls, min and max beside it.  The map is synthetic -- blocky regions at scale 32 with 2 % of the
pixels replaced by single-pixel specks of a random class -- and the serpentine of tests/segments_ref.py at 1024 x 2048 is timed as
the adversarial input (one segment winding through every tile: the longest parent chains).  For context `ops.boundary_counts` at
R = 8 with the same layers on the same frame is timed in the same run.
Bytes are computed from the shapes, per launch, as the least each kernel has to move (every operand once; chases and atomics not
counted), and the rate is those bytes over the call's time -- a whole-call figure, not a kernel's.
Usage (GPU box): python tools/bench_segments.py"""
import json
import os
import statistics
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "da-sac_amd")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from dasac_hip import ops

C = 19
SHAPES = [(1, 1024, 2048), (16, 769, 769)]
WARMUP, RUNS = 3, 25
TH, TW = ops.SEGMENT_TILE


def timed(fn):
    """(median, min, max) seconds of RUNS single calls, each between two HIP events."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(times), min(times), max(times)


def synthetic(B, H, W, gen):
    """int64 [B,H,W]: blocky regions at scale 32, 2 % single-pixel specks."""
    small = torch.randint(0, C, (B, (H + 31) // 32, (W + 31) // 32), generator=gen)
    m = small.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :H, :W].contiguous()
    specks = torch.rand(B, H, W, generator=gen) < 0.02
    m[specks] = torch.randint(0, C, (int(specks.sum()),), generator=gen)
    return m


def launch_bytes(op, B, H, W, label_bytes):
    """{launch: least bytes moved}: P pixels, int32 maps of 4 P bytes, the border items of seg_merge at 4 + label bytes each."""
    P = B * H * W
    border = B * (((H + TH - 1) // TH - 1) * W + ((W + TW - 1) // TW - 1) * H)
    local = lambda src, zeroed: P * (src + 4 + 4 * zeroed)              # labels in, parents and zeroed counters out
    merge = lambda src: border * 4 * (src + 4)                          # the pixel and up to three neighbours: class and parent
    if op == "label_segments":
        return {"seg_local": local(label_bytes, 1), "seg_merge": merge(label_bytes), "seg_resolve": 8 * P, "seg_broadcast": 12 * P}
    if op == "segment_filter":
        return {"seg_local": local(label_bytes, 1), "seg_merge": merge(label_bytes), "seg_resolve": 8 * P,
                "seg_filter_apply": P * (2 * label_bytes + 8)}
    assert op == "segment_counts"                                       # one score layer (a u8 map in the workspace) + one label map
    out = {"seg_prepare": P * (4 * C + 8 + 2), "gt seg_local": local(1, 2), "gt seg_merge": merge(1), "gt seg_resolve": 8 * P}
    for name, src in (("score", 1), ("label", label_bytes)):
        out.update({name + " seg_local": local(src, 3), name + " seg_merge": merge(src), name + " seg_resolve": P * (8 + 1 + src + 4),
                    name + " seg_tabulate": 8 * P})
    return out


rows = []
gen = torch.Generator().manual_seed(0)


def bench(name, B, H, W, labels):
    P = B * H * W
    labels = labels.cuda()
    u8 = labels.to(torch.uint8)
    pred = labels.clone()
    flip = torch.rand(B, H, W, generator=gen).cuda() < 0.1
    pred[flip] = (pred[flip] + 1) % C
    scores = torch.zeros(B, C, H, W, device="cuda").scatter_(1, pred[:, None], 1.0)
    table = torch.zeros(2, 2, ops.SEGMENT_BINS, 4, C, dtype=torch.int64, device="cuda")
    calls = [("label_segments int64", "label_segments", 8, lambda: ops.label_segments(labels, C)),
             ("label_segments uint8", "label_segments", 1, lambda: ops.label_segments(u8, C)),
             ("segment_counts 1 score + 1 uint8 map", "segment_counts", 1, lambda: ops.segment_counts([scores], [u8], labels, table)),
             ("segment_filter uint8, min_size 16", "segment_filter", 1, lambda: ops.segment_filter(u8, 16, C))]
    for what, op, label_bytes, fn in calls:
        med, lo, hi = timed(fn)
        per_launch = launch_bytes(op, B, H, W, label_bytes)
        moved = sum(per_launch.values())
        rows.append(dict(input=name, call=what, ms=med * 1e3, ms_min=lo * 1e3, ms_max=hi * 1e3, moved_MB=moved / 1e6,
                         GB_per_s=moved / med / 1e9, launches={k: round(v / 1e6, 2) for k, v in per_launch.items()}))
    if B == 1:                                                          # the context: boundary_counts at R = 8, the same layers
        bt = torch.zeros(2, 9, 5, C, dtype=torch.int64, device="cuda")
        med, lo, hi = timed(lambda: ops.boundary_counts([scores], [u8], labels, bt))
        rows.append(dict(input=name, call="boundary_counts R=8, 1 score + 1 uint8 map", ms=med * 1e3, ms_min=lo * 1e3, ms_max=hi * 1e3,
                         moved_MB=float("nan"), GB_per_s=float("nan"), launches={}))
    seg, size = ops.label_segments(labels, C)
    return int((seg == torch.arange(H * W, device="cuda", dtype=torch.int32).view(1, H, W)).sum()), int(size.max())


for B, H, W in SHAPES:
    n, largest = bench("{}x{}x{} blocky32 + 2% specks".format(B, H, W), B, H, W, synthetic(B, H, W, gen))
    print("{}x{}x{}: {} segments, the largest of {} pixels".format(B, H, W, n, largest), flush=True)
import segments_ref
n, largest = bench("1x1024x2048 serpentine", 1, 1024, 2048, torch.from_numpy(segments_ref.serpentine(1024, 2048)[None]))
print("serpentine: {} segments, the largest of {} pixels".format(n, largest), flush=True)

print("{:34s} {:44s} {:>9s} {:>19s} {:>9s} {:>8s}".format("input", "call", "ms", "ms min..max", "moved MB", "GB/s"))
for r in rows:
    print("{:34s} {:44s} {:9.3f} {:9.3f}..{:<9.3f} {:9.1f} {:8.1f}".format(r["input"], r["call"], r["ms"], r["ms_min"], r["ms_max"],
                                                                         r["moved_MB"], r["GB_per_s"]))
for r in rows:
    if r["launches"]:
        print("{} | {}: MB per launch {}".format(r["input"], r["call"], r["launches"]))
print(json.dumps(rows))
