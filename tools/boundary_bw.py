"""Time of one `dasac_boundary_counts` call beside its yardstick, `dasac_mask_counts` of the same library in the same process on the
same tensors, at the two validation shapes (4 score layers + 1 label map, 19 classes: 1 x 1024 x 2048 and 2 x 769 x 769) and the
radii 4, 8 and 16: time between two HIP events around a window of WINDOW calls, the two passes' windows alternating, the median of
ROUNDS windows each (profiles/boundary_counts.md).  Bytes are computed from the shapes: `read` = each operand once (what
mask_counts moves); `moved` adds what the boundary pass writes to and reads back from its workspace -- one u8 map per score layer,
int64 label map and the ground truth, read back once per 32 x 64 tile with its R-wide halo.
Maps: `blocky` -- the layers' own arg-max of upsampled low-resolution logits (large regions), the ground truth that prediction with a
fifth of its 64 x 64 blocks replaced, the label map with its least confident 40 % rejected; `random` -- per-pixel random ground truth
and labels (every pixel beside a contour: the row scans end at once, the histogram keys do not merge).
Usage (GPU box): python tools/boundary_bw.py [--rocprof-once]   (--rocprof-once: one call per row, no timing, for a kernel trace)"""
import json
import os
import statistics
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "da-sac_amd"))
import torch
from dasac_hip import ops

C = 19
SHAPES = [(1, 1024, 2048), (2, 769, 769)]
RADII = (4, 8, 16)
WINDOW, ROUNDS = 50, 5
TILE_H, TILE_W = 32, 64                      # csrc/boundary.hip: kBdTileH, kBdTileW
ONCE = "--rocprof-once" in sys.argv
if ONCE:
    RADII = (8,)


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(WINDOW):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / WINDOW * 1e-3


def blocks(values, size, shape, gen):
    B, H, W = shape
    small = values[torch.randint(0, len(values), (B, (H + size - 1) // size, (W + size - 1) // size), generator=gen)]
    return small.repeat_interleave(size, 1).repeat_interleave(size, 2)[:, :H, :W].contiguous().cuda()


def moved_bytes(B, H, W, R, n_scores, n_i64, n_u8):
    """(read, moved): operands once; plus the workspace maps written and staged back tile by tile with their halo."""
    P = B * H * W
    read = n_scores * P * C * 4 + (n_i64 + 1) * P * 8 + n_u8 * P
    ws_maps = 1 + n_scores + n_i64
    tiles = B * ((H + TILE_H - 1) // TILE_H) * ((W + TILE_W - 1) // TILE_W)
    staged = tiles * (TILE_H + 2 * R) * (TILE_W + 2 * R)             # an upper bound: the part outside the image is not loaded
    return read, read + ws_maps * P + (ws_maps + n_u8) * staged


rows = []
gen = torch.Generator().manual_seed(0)
for B, H, W in SHAPES:
    low = [torch.randn(B, C, (H + 7) // 8, (W + 7) // 8, generator=gen).cuda() * 3 for _ in range(4)]
    ups = [ops.upsample_softmax(l, (H, W), None, want_probs=True) for l in low]
    scores = [ups[0][0], ups[1][0], ups[2][1], ups[3][0]]            # logits, logits, probabilities, logits
    pred = scores[0].argmax(1)
    conf = ups[0][1].max(1)[0]
    sample = conf.flatten()[::97]
    lab_blocky = torch.where(conf < sample.kthvalue(int(0.4 * sample.numel()))[0], torch.full_like(pred, 255), pred)
    swap = blocks(torch.cat([torch.full((16,), -2), torch.arange(C)[:3], torch.tensor([255])]), 64, (B, H, W), gen)
    y_blocky = torch.where(swap == -2, pred, swap)
    y_random = torch.randint(0, C, (B, H, W), generator=gen).cuda()
    lab_random = torch.randint(0, C, (B, H, W), generator=gen).cuda()
    lab_random[torch.rand(B, H, W, generator=gen).cuda() < 0.4] = 255
    del ups, conf, sample, swap
    for kind, y, lab in (("blocky", y_blocky, lab_blocky), ("random", y_random, lab_random)):
        mc = torch.zeros(5, 3, C, dtype=torch.int64, device="cuda")
        yard = lambda: ops.mask_counts(scores, [lab], y, mc)
        for R in RADII:
            table = torch.zeros(5, R + 1, 5, C, dtype=torch.int64, device="cuda")
            fn = lambda: ops.boundary_counts(scores, [lab], y, table)
            mc.zero_()
            for f in (yard, fn):
                f(); f()
            torch.cuda.synchronize()
            assert torch.equal(table.sum(1)[:, :3], mc)              # the same counts, summed over the slots
            if ONCE:
                continue
            ty, tf = [], []
            for _ in range(ROUNDS):                                  # alternating windows
                ty.append(window(yard))
                tf.append(window(fn))
            read, moved = moved_bytes(B, H, W, R, 4, 1, 0)
            far = float(table[:, R, :3].sum()) / max(1.0, float(table[:, :, :3].sum()))
            rows.append(dict(name="{}x{}x{} {} R={}".format(B, H, W, kind, R), read_MB=read / 1e6, moved_MB=moved / 1e6,
                             yardstick_us=statistics.median(ty) * 1e6, us=statistics.median(tf) * 1e6, us_min=min(tf) * 1e6,
                             us_max=max(tf) * 1e6, far_share=far))
    # the label-map form of validation_iou's multi-scale path: one uint8 map, staged from where it is
    lab8 = lab_blocky.to(torch.uint8)
    mc1 = torch.zeros(1, 3, C, dtype=torch.int64, device="cuda")
    table1 = torch.zeros(1, 9, 5, C, dtype=torch.int64, device="cuda")
    yard, fn = (lambda: ops.mask_counts([], [lab_blocky], y_blocky, mc1)), (lambda: ops.boundary_counts([], [lab8], y_blocky, table1))
    for f in (yard, fn):
        f(); f()
    torch.cuda.synchronize()
    if not ONCE:
        ty, tf = [], []
        for _ in range(ROUNDS):
            ty.append(window(yard))
            tf.append(window(fn))
        read, moved = moved_bytes(B, H, W, 8, 0, 0, 1)
        rows.append(dict(name="{}x{}x{} blocky R=8, 1 uint8 map".format(B, H, W), read_MB=read / 1e6, moved_MB=moved / 1e6,
                         yardstick_us=statistics.median(ty) * 1e6, us=statistics.median(tf) * 1e6, us_min=min(tf) * 1e6,
                         us_max=max(tf) * 1e6, far_share=float(table1[:, 8, :3].sum()) / max(1.0, float(table1[:, :, :3].sum()))))

print("{:40s} {:>8s} {:>9s} {:>10s} {:>8s} {:>6s} {:>6s} {:>17s}".format("row", "read MB", "moved MB", "yardstick", "us", "ratio", "far", "us min..max"))
for r in rows:
    print("{:40s} {:8.1f} {:9.1f} {:10.1f} {:8.1f} {:6.2f} {:6.2f} {:8.1f}..{:.1f}".format(
        r["name"], r["read_MB"], r["moved_MB"], r["yardstick_us"], r["us"], r["us"] / r["yardstick_us"], r["far_share"], r["us_min"], r["us_max"]))
print(json.dumps(rows))
