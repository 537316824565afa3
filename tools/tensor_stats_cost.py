"""What the per-tensor gradient health table costs (`track_tensor_stats`, dasac_tensor_stats), over the RN101-DeepLabv2 + SAC
student's parameters.  Usage (GPU box): python tools/tensor_stats_cost.py [--iters N] [--repeats R] [--json PATH]

For the 48-byte table (FusedSGD) and the 64-byte table (FusedAdam), with and without a stashed source-pass gradient: two steps of
a tracking optimiser build the state and the uploaded table of a later step; dasac_grad_norm and dasac_tensor_stats are then
launched `iters` times each over that same table between device events (kernel time and launch gaps, no table upload), in turn,
`repeats` times.  Bytes are counted from the shapes: the norm pass reads g (and g2), the stats pass g (and g2), p and the state."""
import argparse
import json
import os
import sys
from types import SimpleNamespace as NS

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--json", default=None)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "da-sac_amd"))
import torch
import torch.nn as nn

import driver
import models
from oracle import nets_ref
from oracle.step_ref import DEFAULT_CFG


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


def main():
    assert torch.cuda.is_available(), "tensor_stats_cost.py measures on the MI355X"
    cfg = NS(**dict(DEFAULT_CFG, INIT_MODEL="", OPT_NESTEROV=False))
    net = models.get_model(cfg, 0, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    net.backbone.load_state_dict(nets_ref.resnet101_state(seed=3, randomize_bn=True, he_init=True, residual_gain=0.25, aspp_gain=0.2), strict=True)
    net.cuda().train()
    rows = []
    for name, row_bytes, slot, c in [("FusedSGD", 48, "ctl", cfg), ("FusedAdam", 64, 0, NS(**dict(vars(cfg), OPT="Adam", BETA1=0.5)))]:
        for stash in (True, False):
            opt = driver.make_optimizer(net, c, tensor_stats=True, skip_nonfinite=True)
            ps = [p for g in opt.param_groups for p in g["params"]]
            gen = torch.Generator(device="cuda").manual_seed(1)
            sets = [[torch.randn(p.shape, device="cuda", generator=gen) * 1e-3 for p in ps] for _ in range(2)]      # kept alive: the table holds raw pointers
            for _ in range(2):                       # the second step's table has no first-step rows: the state is read
                if stash:
                    for p, g in zip(ps, sets[0]):
                        p.grad = g
                    opt.stash_grads()
                for p, g in zip(ps, sets[1]):
                    p.grad = g
                opt.step()
            _, tab, chunks, nt, nc, row_of = opt._tables[slot]
            ctl = opt._control()
            elements = sum(p.numel() for p in ps)
            norm = lambda: opt._norm_pass(tab, row_bytes, nt, chunks, nc, ctl[1], 0.0, None)
            stats = lambda: opt._stats_pass(tab, row_bytes, nt, chunks, nc, row_of, opt._stats_tables()[0], True)
            times = {"dasac_grad_norm": [], "dasac_tensor_stats": []}
            for _ in range(args.repeats):
                times["dasac_grad_norm"].append(dev_time(norm, args.iters))
                times["dasac_tensor_stats"].append(dev_time(stats, args.iters))
            for what, streams in (("dasac_grad_norm", 1 + stash), ("dasac_tensor_stats", 3 + stash)):
                gb = 4 * elements * streams / 1e9
                best = min(times[what])
                rows.append(dict(table=name, row_bytes=row_bytes, stash=stash, entry=what, tensors=len(ps), chunks=nc, elements=elements, gb=round(gb, 4),
                                 us=[round(t, 1) for t in times[what]], tb_per_s=round(gb / best * 1e3, 3)))
                print("{:<10} stash={!s:<5} {:<19} {:.3f} GB  us per call: {}  -> {:.2f} TB/s at the best".format(
                    name, stash, what, gb, "  ".join("%.1f" % t for t in times[what]), gb / best * 1e3), flush=True)
            report = driver.gradient_report(net, opt)
            assert report["nonfinite"] == [] and report["grad_norm"] > 0.0
            del sets
    info = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=args.iters, rows=rows)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(info, f, indent=1)


if __name__ == "__main__":
    main()
