"""Which of ATen's foreach kernels contract a*b + c into one fma?  dasac_adam_step and dasac_sgd_nesterov_step reproduce
torch.optim.Adam / SGD(nesterov=True) bit for bit only if they round where those kernels round.  Every foreach op of the two
update rules runs on 2^20 random elements and is compared with each candidate form, computed in fp64 and rounded to fp32 (the
product of two fp32 numbers is exact in fp64); printed: the number of elements that differ per candidate.
Usage (GPU box): python tools/aten_contraction_probe.py.  Result on torch 2.10 / ROCm 7: profiles/fused_optim.md."""
import torch

assert torch.cuda.is_available(), "aten_contraction_probe.py looks at the device kernels"
torch.manual_seed(0)
n = 1 << 20
dev = "cuda"
a, b, c = (torch.randn(n, device=dev) for _ in range(3))
f32 = lambda t: t.to(torch.float32)
d = lambda t: t.to(torch.float64)
S = lambda v: float(torch.tensor(v, dtype=torch.float32))     # scalar rounded to fp32, as a python double

def report(name, got, hyps):
    print(name, {k: int((got != v).sum()) for k, v in hyps.items()}, "of", n, flush=True)

wd = 5e-4
got = torch._foreach_add([a], [b], alpha=wd)[0]
report("foreach_add alpha", got, {"two roundings": a + f32(d(b) * S(wd)), "fma": f32(d(a) + d(b) * S(wd))})
x = a.clone(); torch._foreach_add_([x], [b], alpha=-2.5e-4)
report("foreach_add_ alpha=-lr", x, {"two roundings": a + f32(d(b) * S(-2.5e-4)), "fma": f32(d(a) + d(b) * S(-2.5e-4))})
for w in (1 - 0.9, 1 - 0.5, 1 - 0.3):
    x = a.clone(); torch._foreach_lerp_([x], [b], w)
    diff = b - a
    wf = S(w)
    if abs(wf) < 0.5:
        hy = {"two roundings": a + f32(d(diff) * wf), "fma": f32(d(a) + d(diff) * wf)}
    else:
        om = float(torch.tensor(1.0, dtype=torch.float32) - torch.tensor(w, dtype=torch.float32))      # Lerp.h: opmath_t(1) - weight
        hy = {"two roundings": b - f32(d(diff) * om), "fma": f32(d(b) - d(diff) * om)}
    report("foreach_lerp_ w=%g" % w, x, hy)
x = a.abs().clone(); torch._foreach_mul_([x], 0.999)
report("foreach_mul_ beta2", x, {"fp32 product": f32(d(a.abs()) * S(0.999))})
v = a.abs()
x = v.clone(); torch._foreach_addcmul_([x], [b], [b], 1 - 0.999)
bb = b * b
w2 = S(1 - 0.999)
report("foreach_addcmul_", x, {"a + s*(b*b) three roundings": v + f32(d(bb) * w2), "fma(s, b*b, a)": f32(d(v) + d(bb) * w2),
                               "(s*b)*b then add": v + f32(d(f32(d(b) * w2)) * d(b)), "fma(s*b, b, a)": f32(d(v) + d(f32(d(b) * w2)) * d(b))})
x = torch._foreach_sqrt([v])[0]
report("foreach_sqrt", x, {"correctly rounded": f32(d(v).sqrt())})
bc = (1 - 0.999 ** 3) ** 0.5
y = x.clone(); torch._foreach_div_([y], [bc])
report("foreach_div_ scalarlist", y, {"true division": f32(d(x) / S(bc)), "times fp32 reciprocal": f32(d(x) * float(1.0 / torch.tensor(bc, dtype=torch.float32))),
                                      "times double reciprocal rounded": f32(d(x) * S(1.0 / bc))})
z = y.clone(); torch._foreach_add_([z], 1e-8)
report("foreach_add_ eps", z, {"fp32 sum": f32(d(y) + S(1e-8))})
step = -(2.5e-4 / (1 - 0.5 ** 3))
p = a.clone(); torch._foreach_addcdiv_([p], [b], [z], [step])
q = f32(d(b) / d(z))
report("foreach_addcdiv_ scalarlist", p, {"a + s*(b/c) three roundings": a + f32(d(q) * S(step)), "fma(s, b/c, a)": f32(d(a) + d(q) * S(step))})
# SGD nesterov pieces
x = a.clone(); torch._foreach_mul_([x], 0.9); torch._foreach_add_([x], [b])
report("buf*momentum + d", x, {"two kernels, two roundings": f32(d(a) * S(0.9)) + b})
x = b.clone(); torch._foreach_add_([x], [a], alpha=0.9)
report("foreach_add_ alpha=momentum", x, {"two roundings": b + f32(d(a) * S(0.9)), "fma": f32(d(b) + d(a) * S(0.9))})
