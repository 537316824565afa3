"""What the per-layer activation tables cost (`driver.activation_probe`, dasac_activation_stats).
Usage (GPU box): python tools/activation_stats_cost.py [--iters N] [--repeats R] [--steps K] [--size 769] [--json PATH]

1. Synthetic planes, one tensor [16, C, HW] of ~1.2 GB each (past the 256 MB Infinity Cache): aligned planes (HW = 96 * 96, every
   plane on a 16-byte boundary), misaligned planes (HW = 97 * 97, planes on every 4-byte phase) and long planes (HW = 385 * 385, 64
   channels: the first convolution's output, 145 sweeps per block).
2. The RN101-DeepLabv2 cfg-3 shapes: every activation of ONE student pass over 8 source + 8 target crops at size^2 (slot 0 and
   every op's output, as the engine's probe hands them over), two segments.
   Both: `iters` calls between device events after 3 warm-up calls, `repeats` figures; kernel time and launch gaps of both
   kernels plus the pinned descriptor upload of a call.  Bytes are counted from the shapes: every activation once.
3. The cfg-3 training step (two-pass schedule, as bench.py times it) with a probe on EVERY pass of an iteration (student source,
   student target, teacher) against the same step without one: `steps` steps each between synchronisations, alternating, `repeats`
   rounds."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace as NS

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--size", type=int, default=769)
ap.add_argument("--json", default=None)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "da-sac_amd"))
import torch
import torch.nn as nn

import driver
import models
from dasac_hip import ops
from oracle.step_ref import DEFAULT_CFG

YARDSTICK_TB_S = 5.1          # dasac_tensor_stats on this hardware (profiles/tensor_stats.md)


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


def rate(name, tensors, bounds, rows):
    plan = ops.activation_stats_plan([tuple(t.shape[1:]) for t in tensors], tensors[0].shape[0], bounds)
    times = [dev_time(lambda: plan.run(tensors), args.iters) for _ in range(args.repeats)]
    gb, best = plan.bytes_read / 1e9, min(times)
    tb = gb / best * 1e3
    rows.append(dict(case=name, tensors=len(tensors), planes=plan.n_planes, rows=plan.R, gb=round(gb, 4), us=[round(t, 1) for t in times],
                     tb_per_s=round(tb, 3), of_yardstick=round(tb / YARDSTICK_TB_S, 3)))
    print("{:<28} {:>4} tensors {:>8} planes {:.3f} GB  us per call: {}  -> {:.2f} TB/s at the best = {:.2f} of {} TB/s".format(
        name, len(tensors), plan.n_planes, gb, "  ".join("%.1f" % t for t in times), tb, tb / YARDSTICK_TB_S, YARDSTICK_TB_S), flush=True)


def main():
    assert torch.cuda.is_available(), "activation_stats_cost.py measures on the MI355X"
    rows = []
    gen = torch.Generator(device="cuda").manual_seed(1)
    for name, shape in [("aligned planes 96x96", (16, 2048, 96, 96)), ("misaligned planes 97x97", (16, 2048, 97, 97)),
                        ("long planes 385x385", (16, 64, 385, 385))]:
        x = torch.randn(shape, device="cuda", generator=gen).relu_()
        rate(name, [x], None, rows)
        del x
    cfg = NS(**dict(DEFAULT_CFG, INIT_MODEL="", OPT_NESTEROV=False))
    net = models.get_model(cfg, 0, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    driver.init_synthetic_weights(net, seed=0)
    net.cuda().train()
    net.running_conf.fill_(0.05)
    optim = driver.make_optimizer(net, cfg)
    hw = (args.size, args.size)
    src, tgt = driver.synthetic_batches(8, 2, 4, hw, "cuda", seed=0)
    src = (src[0], driver.self_consistent_labels(net, src[0]))

    # 2. one student pass over [source; target]
    with torch.no_grad():
        rec = driver.activation_stats(net, torch.cat([src[0], tgt[0]], 0), bounds=(8,))
        eng = net.backbone._engine
        _, saved = eng.forward(torch.cat([src[0], tgt[0]], 0), keep=True)
    held = [saved["acts"][e["slot"]] for e in rec.layout]
    rate("RN101 cfg-3 pass, 16 x {}^2".format(args.size), held, (8,), rows)
    report = driver.activation_report(rec)
    assert report["first_nonfinite_layer"] is None
    print(driver.format_domain_gap_report(driver.domain_gap_report(rec), top=5), flush=True)
    del held, saved, rec

    # 3. the training step with and without the probe
    def step(i):
        tgt_i = (tgt[0], tgt[1].clone(), tgt[2], tgt[3], tgt[4])
        return driver.sac_train_iteration(net, optim, src, tgt_i, 4, update_teacher=(i == 0), lr_target=cfg.LR_TARGET)

    def probed(i):
        with driver.activation_probe(net) as probe:
            out = step(i)
        assert [r.net for r in probe.passes] == ["backbone", "backbone", "slow_net"]
        return out

    def wall(fn, first):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(args.steps):
            fn(first + i)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    for i in range(2):
        step(i)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    step(2)
    torch.cuda.synchronize()
    peak = {"off": torch.cuda.max_memory_allocated() / 1e9}
    torch.cuda.reset_peak_memory_stats()
    probed(2)
    torch.cuda.synchronize()
    peak["on"] = torch.cuda.max_memory_allocated() / 1e9
    steps = {"off": [], "on": []}
    for _ in range(args.repeats):
        steps["off"].append(wall(step, 3))
        steps["on"].append(wall(probed, 3))
    mean = lambda v: sum(v) / len(v)
    print("cfg-3 step, probe off: {}  mean {:.3f} ms".format("  ".join("%.3f" % t for t in steps["off"]), mean(steps["off"])))
    print("cfg-3 step, probe on : {}  mean {:.3f} ms  (+{:.3f} ms, {:+.2f} %)".format(
        "  ".join("%.3f" % t for t in steps["on"]), mean(steps["on"]), mean(steps["on"]) - mean(steps["off"]),
        (mean(steps["on"]) / mean(steps["off"]) - 1) * 100), flush=True)
    print("peak memory of a step: probe off {:.2f} GB, probe on {:.2f} GB".format(peak["off"], peak["on"]))
    info = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=args.iters, size=args.size, rows=rows,
                step_ms=steps, peak_gb={k: round(v, 2) for k, v in peak.items()})
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(info, f, indent=1)


if __name__ == "__main__":
    main()
