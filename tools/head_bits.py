"""SHA-256 of every output of the SAC head's kernels (upsample.hip, cross_entropy.hip, warp.hip) on the cases of their float64 tests:
CE_CASES, LOW_CASES, WARP_CASES, POOL_CASES of tests/test_gpu_head_fp64.py and CASES of tests/test_gpu_upsample_fp64.py, inputs
from those tests' own seeded generators.  One line `name sha256` per output.

    python tools/head_bits.py > branch.txt;  DASAC_LIB=/path/to/older/libdasac_hip.so python tools/head_bits.py > parent.txt

With DASAC_LIB naming another build of the library the hashes are that build's: two fresh processes and a diff are the "same bits
as the parent" check of a change that must not alter what these kernels compute (profiles/head_split.md)."""
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "da-sac_amd"), ROOT):
    sys.path.insert(0, p)

from dasac_hip import ops  # noqa: E402
import test_gpu_head_fp64 as HT  # noqa: E402
import test_gpu_upsample_fp64 as UT  # noqa: E402


def show(name, t):
    if t is not None:
        t = t.detach().contiguous().cpu()
        print("{} {}".format(name, hashlib.sha256(t.numpy().tobytes()).hexdigest()))


def main():
    cuda = lambda t: None if t is None else t.cuda()
    gs = torch.tensor([HT.GSCALE]).cuda()
    for (B, C, H, W), scale in HT.CE_CASES:
        for mode in (0, 1):
            x, y, cw, conf = HT._ce_inputs(B, C, H, W, mode, scale, seed=B + C + H + W + mode)
            tag = "ce_loss/{}x{}x{}x{}/s{:g}/m{}".format(B, C, H, W, scale, mode)
            for name, t in zip(("loss", "dlogits", "per_class"), HT._ce_on_gpu(x, y, cw, conf)):
                show(tag + "/" + name, t)
            show(tag + "/loss_only", ops.ce_loss(x.cuda(), y.cuda(), cw.cuda(), cuda(conf))[0])
    for shape, mode in HT.LOW_CASES:
        B, C, h, w, H, W = shape
        _, y, cw, conf = HT._ce_inputs(B, C, H, W, mode, 3.0, seed=sum(shape))
        low = torch.randn(B, C, h, w, generator=torch.Generator().manual_seed(sum(shape) + 1)) * 3
        up, _, _ = ops.upsample_softmax(low.cuda(), (H, W))
        tag = "ce_loss_bwd_low/{}/m{}".format("x".join(map(str, shape)), mode)
        show(tag + "/dlow", ops.ce_loss_bwd_low(up, y.cuda(), (h, w), cw.cuda(), cuda(conf), gscale=gs))
        show(tag + "/dlow_no_gscale", ops.ce_loss_bwd_low(up, y.cuda(), (h, w), cw.cuda(), cuda(conf)))
    for shape in HT.WARP_CASES:
        B, C, H, W = shape
        for kind in ("random", "mirrored"):
            g = torch.Generator().manual_seed(sum(shape))
            x = torch.randn(B, C, H, W, generator=g)
            theta = HT._random_thetas(B, g) if kind == "random" else HT._mirrored_thetas(B, H, W)
            show("warp_affine/{}/{}".format("x".join(map(str, shape)), kind), ops.warp_affine(x.cuda(), theta.cuda()))
    for shape, modes in HT.POOL_CASES:
        N, Tn, C, H, W = shape
        probs, theta, theta_inv = HT._pool_inputs(shape)
        for mode in modes:
            tag = "warp_pool/{}/{}".format("x".join(map(str, shape)), mode)
            pooled, mask, aligned = ops.warp_pool(probs.cuda(), theta.cuda(), theta_inv.cuda(), Tn, mode, 0.1)
            show(tag + "/pooled", pooled)
            show(tag + "/mask", mask)
            show(tag + "/aligned", aligned)
            show(tag + "/warp_back", ops.warp_back(pooled, mask, theta_inv.cuda(), Tn))
    for case in UT.CASES:
        shape = case[0]
        B, C, h, w, H, W = shape
        for scale in (3.0, 50.0):
            tag = "upsample/{}/s{:g}".format("x".join(map(str, shape)), scale)
            x = UT._logits(shape, scale, sum(shape)).cuda()
            ign = (torch.rand(B, H, W, generator=torch.Generator().manual_seed(sum(shape) + 1)) < 0.2).cuda()
            show(tag + "/up", ops.upsample_softmax(x, (H, W))[0])
            for name, t in zip(("up", "probs", "sums"), ops.upsample_softmax(x, (H, W), ign, want_probs=True, want_sums=True)):
                show(tag + "/softmax/" + name, t)
            for name, t in zip(("up", "probs", "sums"), ops.upsample_softmax(x, (H, W), None, want_up=False, want_probs=True, want_sums=True)):
                show(tag + "/softmax_no_mask/" + name, t)
        g = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(sum(shape) + 2)).cuda()
        tag = "upsample_bwd/{}".format("x".join(map(str, shape)))
        show(tag + "/plain", ops.upsample_bwd(g, (h, w)))
        show(tag + "/scaled", ops.upsample_bwd(g, (h, w), gs))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
