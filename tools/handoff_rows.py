"""One timing figure per hand-off instantiation of conv_gemm: the 7 stream-K and the 7 tail kernels (FAST fp32 plain / recording
the ReLU bits / masking with them / tile statistics, FAST split-bf16, generic fp32 and split-bf16), each on 8 x 256 x 97 x 97, 3x3
dilation 2 over 256 (FAST) or 136 (generic) input channels, stream-K forced, the tail by the library's own choice.
Usage (GPU box): [DASAC_LIB=other/libdasac_hip.so] python tools/handoff_rows.py  ->  "row <name> <us>": median of 15 launches, CUDA
events.  For A/B comparisons of two builds of the library (fresh processes, alternated): profiles/conv_plan.md section 3.
(tools/one_conv.py runs four fixed shapes on the library's own schedule: it cannot force stream-K and reaches neither the split-bf16,
the generic nor the statistics instantiations.)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "da-sac_amd"))
import torch
from dasac_hip import ops, lib as L
lib = L.load()
B, H, W, cout = 8, 97, 97, 256
torch.manual_seed(0)


def row(name, cin, prec, variant, schedule):
    ops.set_precision(prec)
    spec = ops.ConvSpec(cin, cout, [(3, 3, 2, 2)], 1)
    x = torch.randn(B, cin, H, W, device="cuda")
    w = [torch.randn(cout, cin, 3, 3, device="cuda") * 0.05]
    order = ops.gemm_order(spec, False)
    tab, pk = ops.conv_table(spec, H, W, False, x.device, order), ops.conv_pack(spec, w, False, order=order)
    y = torch.empty(B, cout, H, W, device="cuda")
    kw = {}
    if variant == "bits_out":
        kw = dict(relu=True, bits_out=ops.ReluBits(B, cout, H, W, x.device))
    elif variant == "mask_bits":
        m = ops.ReluBits(B, cout, H, W, x.device)
        m.words.random_(-2 ** 31, 2 ** 31 - 1)
        kw = dict(mask=m)
    elif variant == "stats":
        kw = dict(stats=ops.tile_stats_buffer(B, cout, H, W, x.device))
    if schedule is None:
        assert lib.dasac_conv_gemm_tail_split(B, H, W, cout, spec.K) > 0, name
    run = lambda: ops.conv_gemm(x, pk, tab, y, (H, W), 1, cout, spec.K, 1, None, None, schedule=schedule, **kw)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    ts = []
    for _ in range(15):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); run(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    print("row {} {:.1f}".format(name, ts[len(ts) // 2]), flush=True)


for sk, schedule in (("streamk", 2), ("tail", None)):
    for variant in ("plain", "bits_out", "mask_bits", "stats"):
        row("{}/fast/fp32/{}".format(sk, variant), 256, "fp32", variant, schedule)
    row(sk + "/fast/x3/plain", 256, "bf16x3", "plain", schedule)
    row(sk + "/generic/fp32/plain", 136, "fp32", "plain", schedule)
    row(sk + "/generic/x3/plain", 136, "bf16x3", "plain", schedule)
