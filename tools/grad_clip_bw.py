"""What gradient-norm clipping inside the fused optimisers costs, over the RN101-DeepLabv2 + SAC student's parameters (the set of
tools/optim_bw.py).  Usage (GPU box): python tools/grad_clip_bw.py [--iters N] [--repeats R] [--offset-grads] [--tree PATH] [--json PATH]

For FusedSGD, FusedSGD(nesterov=True) and FusedAdam, with the source-pass gradients stashed as driver.sac_train_iteration
leaves them, one step as
    default      all keywords at their defaults: the plain entry point, one kernel
    clipped      max_grad_norm=1.0, skip_nonfinite=True: dasac_grad_norm (two kernels) + the _ctl update
    by hand      what it replaces: full_grads() (one ATen add per tensor), clip_grad_norm_, step() of the default optimiser
--offset-grads hands every gradient over as a view one element into its buffer, as a slice of a flat reduction buffer may lie
(no 16-byte alignment: grad_sq_chunks and adam_chunks then use 4-byte loads).  --tree PATH imports the project from another
checkout (one without the keywords measures `default` only: the parent commit).
Gradients alternate between two sets from call to call, so every step sees new pointers and rebuilds its table, as after a
backward pass.  Time per call from device events around `iters` calls, host side included; the cases are measured `repeats`
times in turn (a, b, c, a, b, c ...) so that the spread between equal runs shows.  Kernel times: run this under
`rocprofv3 --kernel-trace --stats` in a run of its own."""
import argparse
import json
import os
import sys
from types import SimpleNamespace as NS

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--offset-grads", action="store_true",
                help="every gradient is a view 4 bytes into a buffer of its own: the norm pass and Adam take their scalar-load paths")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--json", default=None)
args = ap.parse_args()
ROOT = os.path.abspath(args.tree)
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


def main():
    assert torch.cuda.is_available(), "grad_clip_bw.py measures on the MI355X"
    import inspect
    has_keywords = "max_grad_norm" in inspect.signature(driver.make_optimizer).parameters
    cfg = NS(**dict(DEFAULT_CFG, INIT_MODEL="", OPT_NESTEROV=False))
    net = models.get_model(cfg, 0, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    net.cuda().train()
    with_cfg = lambda **kw: NS(**dict(vars(cfg), **kw))
    kinds = [("FusedSGD", cfg), ("FusedSGD(nesterov=True)", with_cfg(OPT_NESTEROV=True)), ("FusedAdam", with_cfg(OPT="Adam", BETA1=0.5))]
    rows = []
    for name, c in kinds:
        ps = [p for g in driver.make_optimizer(net, c, fused="all").param_groups for p in g["params"]]
        gen = torch.Generator(device="cuda").manual_seed(1)

        def grad_like(p):
            if not args.offset_grads:
                return torch.randn(p.shape, device="cuda", generator=gen) * 1e-3
            flat = torch.randn(p.numel() + 1, device="cuda", generator=gen) * 1e-3
            return flat[1:].view(p.shape)
        sets = [[grad_like(p) for p in ps] for _ in range(3)]
        turn = [0]

        def two_passes(opt):
            turn[0] += 1
            for p, g in zip(ps, sets[2]):
                p.grad = g
            opt.stash_grads()
            for p, g in zip(ps, sets[turn[0] % 2]):
                p.grad = g

        def fused_step(opt):
            def step():
                two_passes(opt)
                opt.step()
            return step

        def by_hand(opt):
            def step():
                two_passes(opt)
                full = opt.full_grads()
                opt.zero_grad()
                for p in ps:
                    p.grad = full[p]
                torch.nn.utils.clip_grad_norm_(ps, 1.0)
                opt.step()
            return step
        cases = [("default", fused_step(driver.make_optimizer(net, c, fused="all")))]
        if has_keywords:
            cases.append(("clipped", fused_step(driver.make_optimizer(net, c, max_grad_norm=1.0, skip_nonfinite=True))))
            cases.append(("by hand", by_hand(driver.make_optimizer(net, c, fused="all"))))
        times = {case: [] for case, _ in cases}
        for _ in range(args.repeats):
            for case, fn in cases:
                times[case].append(round(dev_time(fn, args.iters), 1))
        for case, _ in cases:
            rows.append(dict(optimiser=name, case=case, us=times[case], tensors=len(ps), elements=sum(p.numel() for p in ps)))
            print("{:<26} {:<8} us per call: {}".format(name, case, "  ".join("%.1f" % t for t in times[case])), flush=True)
        del cases, sets
    info = dict(offset_grads=args.offset_grads, device=torch.cuda.get_device_name(0), torch=torch.__version__, tree=ROOT, iters=args.iters, rows=rows)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(info, f, indent=1)


if __name__ == "__main__":
    main()
