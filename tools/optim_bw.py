"""Device time of one optimiser step over the RN101-DeepLabv2 + SAC student's parameters: the fused HIP optimisers next to the
torch classes the reference's factory builds (base_trainer.py:47-73).  Usage (GPU box): python tools/optim_bw.py [--iters N] [--json PATH]

    FusedAdam                      against torch.optim.Adam (foreach), betas = (0.5, 0.999), the four parameter groups
    FusedAdam with a stash         the source-pass gradient set aside, summed inside the update (driver.sac_train_iteration)
    FusedSGD(nesterov=True)        against torch.optim.SGD(nesterov=True) (foreach), momentum 0.9

Gradients are present and the state is warm (three steps before the timed window).  Two gradient sets alternate from call to
call, so every step sees new gradient pointers, as after a backward pass: the fused optimisers rebuild and upload their
pointer table every step, which is part of what is timed.  Time per step from device events around `iters` calls; it includes
the host side of each call.  Launches per step: device kernels seen by torch.profiler over one step (memory copies listed
apart).  Algorithmic bytes per element: Adam 4 reads + 3 writes (5 reads with a stash), Nesterov 3 reads + 2 writes, fp32."""
import argparse
import json
import os
import sys
from types import SimpleNamespace as NS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "da-sac_amd"))
import torch
import torch.nn as nn

import driver
import models
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


def launches(fn):
    """(kernels, memory copies) the device ran for one call."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    dev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    copies = [e for e in dev if "memcpy" in e.name.lower() or "copy" in e.name.lower() and "kernel" not in e.name.lower()]
    return len(dev) - len(copies), len(copies)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "optim_bw.py measures on the MI355X"
    cfg = NS(**dict(DEFAULT_CFG, INIT_MODEL="", OPT_NESTEROV=False))
    net = models.get_model(cfg, 0, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    net.cuda().train()
    with_cfg = lambda **kw: NS(**dict(vars(cfg), **kw))
    cases = [("FusedAdam", with_cfg(OPT="Adam", BETA1=0.5), "all", False, 7),
             ("FusedAdam, stashed source gradients", with_cfg(OPT="Adam", BETA1=0.5), "all", True, 8),
             ("torch.optim.Adam (foreach)", with_cfg(OPT="Adam", BETA1=0.5), False, False, 7),
             ("FusedSGD(nesterov=True)", with_cfg(OPT_NESTEROV=True), "all", False, 5),
             ("FusedSGD(nesterov=True), stashed source gradients", with_cfg(OPT_NESTEROV=True), "all", True, 6),
             ("torch.optim.SGD(nesterov=True) (foreach)", with_cfg(OPT_NESTEROV=True), False, False, 5)]
    rows = []
    for name, c, fused, stash, words in cases:
        opt = driver.make_optimizer(net, c, fused=fused)
        ps = [p for g in opt.param_groups for p in g["params"]]
        gen = torch.Generator(device="cuda").manual_seed(1)
        sets = [[torch.randn(p.shape, device="cuda", generator=gen) * 1e-3 for p in ps] for _ in range(3 if stash else 2)]
        n_elem, turn = sum(p.numel() for p in ps), [0]

        def step():
            turn[0] += 1
            if stash:
                for p, g in zip(ps, sets[2]):
                    p.grad = g
                opt.stash_grads()
            for p, g in zip(ps, sets[turn[0] % 2]):
                p.grad = g
            opt.step()
        us = dev_time(step, args.iters)
        try:
            kernels, copies = launches(step)
        except Exception as exc:                      # the profiler is not what is measured here
            print("launch count not measured for {}: {!r}".format(name, exc))
            kernels = copies = None
        nbytes = words * 4 * n_elem
        rows.append(dict(name=name, us=round(us, 1), kernels=kernels, copies=copies, tensors=len(ps), elements=n_elem, bytes=nbytes,
                         tbps=round(nbytes / us * 1e-6, 3)))
        del opt, sets
    print("{:<52} {:>10} {:>9} {:>8} {:>9}".format("one step over %d tensors, %.1f M elements" % (rows[0]["tensors"], rows[0]["elements"] / 1e6),
                                                  "us", "kernels", "copies", "TB/s"))
    for r in rows:
        print("{:<52} {:>10.1f} {:>9} {:>8} {:>9.3f}".format(r["name"], r["us"], str(r["kernels"]), str(r["copies"]), r["tbps"]))
    info = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, iters=args.iters, rows=rows)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(info, f, indent=1)


if __name__ == "__main__":
    main()
