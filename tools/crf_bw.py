"""Time per mean-field iteration of ops.crf_meanfield (dasac_crf_meanfield) at a full Cityscapes frame (1 x 19 x 1024 x 2048) and at a
validation batch (8 x 19 x 769 x 769), and beside it, on the same tensors, what a refined frame also pays: the ops.infer_fuse launch
that makes the probabilities and the backbone's `_logits` call.  HIP events on the launch stream; the per-iteration time is the
difference of a call with 1 + `--iters` iterations and a call with 1, over `--iters` (so the launch that fuses arg-max and LUT is
in both).  Algorithmic bytes per iteration: Q read, P read, I read, Q written, every tensor once.  Every round is printed: the
spread is part of the result.  Usage (GPU box): python tools/crf_bw.py"""
import argparse
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "da-sac_amd"))
from types import SimpleNamespace as NS
import torch
import torch.nn as nn
from dasac_hip import ops
from crf import CrfParams
import driver


def timeit(fn, calls):
    fn(); fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e-3


def build_net():
    import models
    from oracle.step_ref import DEFAULT_CFG
    cfg = dict(DEFAULT_CFG)
    cfg.update(INIT_MODEL="", OPT_NESTEROV=False)
    net = models.get_model(NS(**cfg), 0, num_classes=19, criterion=nn.CrossEntropyLoss(ignore_index=255, reduction="none"))
    driver.init_synthetic_weights(net, seed=0)
    return net.cuda().eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", type=str, nargs="+", default=["1x1024x2048", "8x769x769"])
    ap.add_argument("--classes", type=int, default=19)
    ap.add_argument("--iters", type=int, default=5, help="mean-field iterations the per-iteration time is taken over")
    ap.add_argument("--calls", type=int, default=10, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-backbone", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this is a measurement on the MI355X; there is nothing to time without it"
    C, base = args.classes, CrfParams()
    print(base.describe())
    net = None if args.no_backbone else build_net()
    g = torch.Generator().manual_seed(0)
    print("{:14s} {:>5s} {:>12s} {:>12s} {:>10s} {:>8s} {:>12s} {:>12s}".format(
        "shape", "round", "1 iter us", "1+{} iter us".format(args.iters), "us / iter", "TB/s", "infer_fuse us", "_logits us"))
    for shape in args.shapes:
        B, H, W = (int(v) for v in shape.split("x"))
        image = torch.randn(B, 3, H, W, generator=g).cuda()
        with torch.no_grad():
            if net is not None:
                logits = net.backbone._logits(image)
            else:
                logits = (torch.randn(B, C, (H + 7) // 8, (W + 7) // 8, generator=g) * 3).cuda()
            _, _, probs = ops.infer_fuse([logits], [False], (H, W), want_probs=True)
            nbytes = (3 * C + image.shape[1]) * B * H * W * 4
            one, many = base.replace(n_iter=1), base.replace(n_iter=1 + args.iters)
            for r in range(args.rounds):
                t1 = timeit(lambda: ops.crf_meanfield(probs, image, one), args.calls)
                tn = timeit(lambda: ops.crf_meanfield(probs, image, many), args.calls)
                tf = timeit(lambda: ops.infer_fuse([logits], [False], (H, W), want_probs=True), args.calls)
                tl = timeit(lambda: net.backbone._logits(image), 3) if net is not None else float("nan")
                per = (tn - t1) / args.iters
                print("{:14s} {:5d} {:12.1f} {:12.1f} {:10.1f} {:8.3f} {:12.1f} {:12.1f}".format(
                    shape, r, t1 * 1e6, tn * 1e6, per * 1e6, nbytes / per / 1e12, tf * 1e6, tl * 1e6))
            print("{:14s} algorithmic bytes per iteration {:.1f} MB; pixel updates per second at the last round {:.2f} G".format(
                shape, nbytes / 1e6, B * H * W / per / 1e9))
        del image, probs, logits
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
