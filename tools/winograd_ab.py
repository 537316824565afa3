"""A/B of ONE layer4 conv2 (512 -> 512, 3x3, dilation 4, 8 crops of 97 x 97; with --channels 256 --dilation 2 one of layer3): the
direct implicit GEMM against the Winograd F(2x2,3x3) path, forward (shift + ReLU + recorded bits), data gradient (masked with
recorded bits) and weight gradient (scaled, with the frozen BN's dot rows and channel sums), as the engine issues them.

    python tools/winograd_ab.py [--reps 3] [--iters 10] [--direct-only] [--gemm-schedule -1 1 2]

Per repetition: `iters` back-to-back evaluations between one HIP event pair -> ms per conv, summing every launch that replaces
the direct one (input transform + the 16 point GEMMs, as one batched launch or as 16 + output transform; weight gradient: both
transforms + the batched point contraction + finish, against conv_wgrad + its finish).  A second pass splits
the Winograd time per kernel with an event pair per launch (ops.PROFILE; median and max - min of `reps` repetitions); the weight gradient has a second Winograd leg, F(4x4,3x3)
(ops.winograd4_wgrad), with its own split, and so have the forward and the data gradient (ops.winograd4_conv; the forward also
without recorded bits, as a no-grad pass runs it).  With DASAC_LIB naming an older build of the library
the figures are that build's (the A/B against the parent commit on the same box): --direct-only for its direct GEMM,
--gemm-schedule 2 for the 16-launch form an older build has."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "da-sac_amd"))

from dasac_hip import ops  # noqa: E402
from dasac_hip import lib as L  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--channels", type=int, default=512)
    ap.add_argument("--size", type=int, default=97)
    ap.add_argument("--dilation", type=int, default=4)
    ap.add_argument("--direct-only", action="store_true")
    ap.add_argument("--gemm-schedule", type=int, nargs="+", default=[-1],
                    help="the 16 point GEMMs: -1 what the engine uses, one batched launch (default); as 16 launches: 0 the library's choice, "
                         "1 one block per tile, 2 stream-K; several values are measured one after the other in this process")
    args = ap.parse_args()
    scheds = [(v, {-1: "auto", 0: None}.get(v, v)) for v in args.gemm_schedule]
    dev = torch.device("cuda", 0)
    N, C, S, d = args.batch, args.channels, args.size, args.dilation
    torch.manual_seed(0)
    spec = ops.ConvSpec(C, C, [(3, 3, d, d)])
    x = torch.randn(N, C, S, S, device=dev)
    dz = torch.randn(N, C, S, S, device=dev)
    w = torch.randn(C, C, 3, 3, device=dev) * (2.0 / (9 * C)) ** 0.5
    scale, shift = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev) * 0.1
    out, dx = torch.empty_like(x), torch.empty_like(x)
    bits, mask = ops.ReluBits(N, C, S, S, dev), ops.ReluBits(N, C, S, S, dev)
    mask.words.random_(-2 ** 31, 2 ** 31 - 1)

    of, ot = ops.gemm_order(spec, False), ops.gemm_order(spec, True)
    tab_f, tab_t = ops.conv_table(spec, S, S, False, dev, of), ops.conv_table(spec, S, S, True, dev, ot)
    pk_f, pk_t = ops.conv_pack(spec, [w], False, scale, order=of), ops.conv_pack(spec, [w], True, scale, order=ot)
    # weight gradient as the engine issues it behind a frozen BN: scaled, with the partial dot rows and the channel sums of dz
    tab_w = ops.conv_table(spec, S, S, False, dev)
    dw, dot, sums = torch.empty_like(w), torch.empty(ops.dot_rows(spec), C, device=dev), torch.empty(C, device=dev)
    legs = {
        "forward direct": lambda: ops.conv_gemm(x, pk_f, tab_f, out, (S, S), 1, C, spec.K, 1, shift, None, None, True, bits_out=bits),
        "dgrad   direct": lambda: ops.conv_gemm(dz, pk_t, tab_t, dx, (S, S), 1, C, spec.Kt, 1, None, None, mask, False),
        "wgrad   direct": lambda: ops.conv_wgrad(spec, dz, x, [w], scale=scale, dot=dot, table=tab_w, sum_dz=sums, outs=[dw]),
    }
    if not args.direct_only:
        u_f, u_t = ops.winograd_filter(spec, w, False, scale), ops.winograd_filter(spec, w, True, scale)
        for v, sched in scheds:
            sfx = "" if len(scheds) == 1 else " (--gemm-schedule {})".format(v)
            legs["forward winograd" + sfx] = lambda sched=sched: ops.winograd_conv(x, u_f, out, d, shift, True, bits_out=bits, gemm_schedule=sched)
            legs["dgrad   winograd" + sfx] = lambda sched=sched: ops.winograd_conv(dz, u_t, dx, d, mask_bits=mask, gemm_schedule=sched)
        if hasattr(L.load(), "dasac_winograd4_output") and L.load().dasac_conv_mpad(C) % 128 == 0:       # absent from an older build
            u4_f, u4_t = ops.winograd4_filter(spec, w, False, scale), ops.winograd4_filter(spec, w, True, scale)
            legs["forward winograd F(4x4)"] = lambda: ops.winograd4_conv(x, u4_f, out, d, shift, True, bits_out=bits)
            legs["forward winograd F(4x4), no bits (no-grad pass)"] = lambda: ops.winograd4_conv(x, u4_f, out, d, shift, True)
            legs["dgrad   winograd F(4x4)"] = lambda: ops.winograd4_conv(dz, u4_t, dx, d, mask_bits=mask)
            legs["filter transform F(4x4) (per weight update, forward + dgrad)"] = lambda: (
                ops.winograd4_filter(spec, w, False, scale, out=u4_f), ops.winograd4_filter(spec, w, True, scale, out=u4_t))
        if hasattr(L.load(), "dasac_conv_wgrad_batched"):      # absent from an older build named by DASAC_LIB
            legs["wgrad   winograd"] = lambda: ops.winograd_wgrad(spec, dz, x, w, scale=scale, dot=dot, sum_dz=sums, out=dw)
        if hasattr(L.load(), "dasac_winograd4_wgrad_finish"):
            legs["wgrad   winograd F(4x4)"] = lambda: ops.winograd4_wgrad(spec, dz, x, w, scale=scale, dot=dot, sum_dz=sums, out=dw)
            T4 = L.load().dasac_winograd4_tiles(N, S, S, d)
            print("F(4x4) weight gradient: {} tiles, {} pixel splits of the 36 point contractions".format(
                T4, L.load().dasac_conv_wgrad_batched_splits(36, C, C, T4)))
        legs["filter transform (per weight update, forward + dgrad)"] = lambda: (ops.winograd_filter(spec, w, False, scale, out=u_f),
                                                                                 ops.winograd_filter(spec, w, True, scale, out=u_t))
    print("library: {}   shape: {} x {} -> {} x {} x {}, dilation {}   {} iterations per repetition".format(
        L.LIB_PATH, N, C, C, S, S, d, args.iters))
    for fn in legs.values():        # every leg once through, untimed: clocks and caches settled before the first repetition counts
        timed(fn, args.iters)
    for name, fn in legs.items():
        ms = [timed(fn, args.iters) for _ in range(args.reps)]
        print("{:<58s} ms per conv: {}   spread {:.4f}".format(name, "  ".join("{:.4f}".format(v) for v in ms), max(ms) - min(ms)))
    if not args.direct_only:
        for name in [n for n in legs if "winograd" in n]:
            legs[name]()
            torch.cuda.synchronize()
            profs = []
            for _ in range(args.reps):
                ops.PROFILE.start()
                for _ in range(args.iters):
                    legs[name]()
                profs.append(ops.PROFILE.stop())
            print(name + ", per-kernel split (event pair per launch), median of {} repetitions:".format(args.reps))
            for k, v in sorted(profs[0].items()):
                ms = sorted(p[k]["seconds"] / args.iters * 1e3 for p in profs)
                sec = ms[len(ms) // 2] * 1e-3 * args.iters
                print("    {:<28s} {:2d} launches  {:.4f} ms per conv   spread {:.4f}   {:.1f} TFLOP/s  {:.2f} TB/s algorithmic".format(
                    k, v["launches"] // args.iters, ms[len(ms) // 2], ms[-1] - ms[0], v["flops"] / max(sec, 1e-12) / 1e12,
                    v["bytes"] / max(sec, 1e-12) / 1e12))


if __name__ == "__main__":
    main()
