"""The frozen-BN helpers of batchnorm.hip -- bn_fold, bn_fold_multi, bn_param_grads, channel_sums -- against float64 on the CPU,
from the formulas of include/dasac_hip.h.  Bounds are per element and relative to the terms each value is made of (as in
test_gpu_bn_kernels.py), never to the tensor's max, and come from first-order rounding analysis: one u = 2^-24 per correctly
rounded fp32 operation, then doubled.  They assume -ffp-contract=off and correctly rounded divide and sqrt.

bn_fold        invstd = 1/sqrt(var + eps): add (enters at half weight), sqrt, divide = 2.5u -> 5u relative;
               scale = gamma*invstd: + one multiply = 3.5u -> 7u*|scale|;
               shift = beta - (mean - b)*scale: subtract u, scale 3.5u, multiply u = 5.5u of |mean-b|*|scale|, and the final
               subtraction u*(|beta| + |mean-b|*|scale|) -> 13u*|mean-b|*|scale| + 2u*|beta|.
               C in {1, 37, 255, 256, 257, 2048} x conv_bias given / NULL x invstd wanted / NULL x eps in {1e-5, 1e-3}; var mixes
               0, 1e-12, O(1) and 1e6; gamma has negative values and exact 0; mean sits within 1e-6 relative of conv_bias in every
               third channel; outputs are C + 8 floats pre-filled with NaN (the 8 behind stay NaN, the C in front are written).
bn_fold_multi  one table (ops.build_refresh_tables) of jobs with C = 1, 255, 256, 257, 600, conv_bias alternating, two eps, the
               outputs fenced slices of one buffer: torch.equal to ops.bn_fold of the same inputs, fences intact.
bn_param_grads C in {1, 63, 64, 65, 300} x dot_rows in {1, 4, 33} x scale given / NULL x conv_bias given / NULL x each output
               alone and all three: dbeta equals sum_dz and dbias the CPU fp32 product scale*sum_dz bit for bit; dgamma within
               2u*(dot_rows + 3)*|invstd|*(sum_r |dot_r| + |b - mean|*|sum_dz|); outputs not requested stay untouched; dgamma
               without `dot` is DASAC_EINVAL.
channel_sums   N in {1, 3} x C in {1, 5} x HW in {1, 255, 256, 257, 1000, 65*65}, data with mean 100 / std 1 and a zero-mean
               set: |err| <= 2u*ceil(HW/256)*sum|x| of the channel (a thread's recursive fp32 partial plus the final rounding,
               doubled); `out=` returns the given buffer; HW >= 2^31 and null pointers are refused on the host.

Worst measured got/bound on the MI355X (the tests print every figure before asserting): bn_fold invstd 0.37, scale 0.37,
shift 0.49; bn_param_grads dgamma 0.24; channel_sums 0.43 (at HW = 1, where only the final rounding is left; 0.02 at HW = 65*65).
The fp64_yardstick ratio of channel_sums against ATen's fp32 sum is at most 0.09 (printed, not asserted)."""
import numpy as np
import pytest
import torch

import fp64_yardstick as Y

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EINVAL = -1
FENCE = 8


def _lib():
    from dasac_hip import lib as L
    return L, L.load()


def _nanbuf(n):
    return torch.full((n + FENCE,), float("nan"), dtype=torch.float32, device="cuda")


def _fenced(buf, n, what):
    """host copy of the n written floats of a NaN-prefilled buffer of n + FENCE; the fence must still be NaN"""
    h = buf.cpu()
    assert torch.isnan(h[n:]).all(), (what, "wrote behind the output")
    assert not torch.isnan(h[:n]).any(), (what, "left an element unwritten")
    return h[:n]


def _ratio(got, ref, bound):
    return float(((got.double() - ref).abs() / (bound + 1e-300)).max())


# ---- bn_fold -------------------------------------------------------------------------------------------------------------
def _fold_inputs(C, seed):
    g = torch.Generator().manual_seed(seed)
    gamma = torch.randn(C, generator=g)
    gamma[::5] = 0.0
    gamma[1::7] = -gamma[1::7].abs() - 0.1
    beta = torch.randn(C, generator=g)
    bias = torch.randn(C, generator=g) * 3
    mean = torch.randn(C, generator=g) * 3
    mean[::3] = bias[::3] * (1 + 1e-6 * torch.randn(C, generator=g)[::3])        # cancellation in mean - b
    var = torch.rand(C, generator=g) + 0.25
    var[::4] = 0.0
    var[1::4] = 1e-12
    var[2::8] = 1e6
    return gamma, beta, mean, var, bias


def _fold_ref(gamma, beta, mean, var, bias, eps):
    eps32 = float(np.float32(eps))                                                # the ABI takes eps as a float
    inv = 1.0 / torch.sqrt(var.double() + eps32)
    scale = gamma.double() * inv
    mb = mean.double() - (bias.double() if bias is not None else 0.0)
    shift = beta.double() - mb * scale
    return inv, scale, shift, mb


@pytest.mark.parametrize("C", [1, 37, 255, 256, 257, 2048])
def test_bn_fold_fp64(C):
    L, lib = _lib()
    gamma, beta, mean, var, bias = _fold_inputs(C, 100 + C)
    dev = [t.cuda() for t in (gamma, beta, mean, var, bias)]
    worst = {"invstd": 0.0, "scale": 0.0, "shift": 0.0}
    for eps in (1e-5, 1e-3):
        for with_bias in (True, False):
            for want_invstd in (True, False):
                what = (C, eps, with_bias, want_invstd)
                scale, shift, invstd = _nanbuf(C), _nanbuf(C), _nanbuf(C)
                code = lib.dasac_bn_fold(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
                                         dev[4].data_ptr() if with_bias else None, eps, C, scale.data_ptr(), shift.data_ptr(),
                                         invstd.data_ptr() if want_invstd else None, L.stream_ptr())
                torch.cuda.synchronize()
                assert code == 0, what
                inv_r, scale_r, shift_r, mb = _fold_ref(gamma, beta, mean, var, bias if with_bias else None, eps)
                r = {"scale": _ratio(_fenced(scale, C, what), scale_r, 7 * U * scale_r.abs()),
                     "shift": _ratio(_fenced(shift, C, what), shift_r, 13 * U * mb.abs() * scale_r.abs() + 2 * U * beta.double().abs())}
                if want_invstd:
                    r["invstd"] = _ratio(_fenced(invstd, C, what), inv_r, 5 * U * inv_r)
                else:
                    assert torch.isnan(invstd.cpu()).all(), (what, "invstd = NULL was written")
                for k, v in r.items():
                    worst[k] = max(worst[k], v)
                    assert v <= 1.0, (what, k, v)
                # gamma == 0 gives scale == 0 exactly and shift == beta exactly
                z = gamma == 0
                assert (scale.cpu()[:C][z] == 0).all() and torch.equal(shift.cpu()[:C][z], beta[z])
    print("bn_fold C={}: worst got/bound invstd {:.3g} scale {:.3g} shift {:.3g}".format(C, worst["invstd"], worst["scale"], worst["shift"]))


def test_bn_fold_ops_wrapper_equals_the_abi_call():
    from dasac_hip import ops
    L, lib = _lib()
    C = 257
    gamma, beta, mean, var, bias = (t.cuda() for t in _fold_inputs(C, 7))
    for cb in (bias, None):
        for want in (True, False):
            s, h, i = ops.bn_fold(gamma, beta, mean, var, 1e-5, conv_bias=cb, want_invstd=want)
            bs, bh, bi = _nanbuf(C), _nanbuf(C), _nanbuf(C)
            assert lib.dasac_bn_fold(gamma.data_ptr(), beta.data_ptr(), mean.data_ptr(), var.data_ptr(), L.ptr(cb) or None, 1e-5, C,
                                     bs.data_ptr(), bh.data_ptr(), bi.data_ptr(), L.stream_ptr()) == 0
            assert torch.equal(s, bs[:C]) and torch.equal(h, bh[:C])
            assert (i is None) == (not want) and (i is None or torch.equal(i, bi[:C]))


def test_bn_fold_refuses_null_and_empty():
    L, lib = _lib()
    t = torch.ones(4, device="cuda")
    p = t.data_ptr()
    args = lambda **kw: [kw.get("gamma", p), kw.get("beta", p), kw.get("mean", p), kw.get("var", p), None, 1e-5, kw.get("C", 4),
                         kw.get("scale", p), kw.get("shift", p), None, L.stream_ptr()]
    for bad in ({"gamma": None}, {"beta": None}, {"mean": None}, {"var": None}, {"scale": None}, {"shift": None}, {"C": 0}, {"C": -1}):
        assert lib.dasac_bn_fold(*args(**bad)) == EINVAL, bad


# ---- bn_fold_multi ---------------------------------------------------------------------------------------------------------
def test_bn_fold_multi_equals_bn_fold_job_by_job():
    from dasac_hip import ops
    Cs = [1, 255, 256, 257, 600]
    gap = 3                                                    # odd: the slices start on every 4-byte phase
    total = sum(3 * (C + gap) for C in Cs) + gap
    out = torch.full((total,), float("nan"), dtype=torch.float32, device="cuda")
    written = torch.zeros(total, dtype=torch.bool)
    jobs, ins, at = [], [], gap
    for j, C in enumerate(Cs):
        gamma, beta, mean, var, bias = (t.cuda() for t in _fold_inputs(C, 300 + j))
        cb = bias if j % 2 == 0 else None
        eps = 1e-5 if j % 3 else 1e-3
        outs = []
        for _ in range(3):
            outs.append(out[at:at + C])
            written[at:at + C] = True
            at += C + gap
        jobs.append((gamma, beta, mean, var, cb, tuple(outs), eps, C))
        ins.append((gamma, beta, mean, var, cb, eps))
    assert len({eps for *_, eps in ins}) == 2
    tables = ops.build_refresh_tables(jobs, [], out.device)
    assert tables["n_fold_chunks"] == sum((C + 255) // 256 for C in Cs)
    ops.refresh_network(tables)
    torch.cuda.synchronize()
    for (gamma, beta, mean, var, cb, eps), job in zip(ins, jobs):
        s, h, i = ops.bn_fold(gamma, beta, mean, var, eps, conv_bias=cb, want_invstd=True)
        assert torch.equal(job[5][0], s) and torch.equal(job[5][1], h) and torch.equal(job[5][2], i), (job[7], cb is not None, eps)
        assert not torch.isnan(s).any()
    host = out.cpu()
    assert torch.isnan(host[~written]).all(), "bn_fold_multi wrote between the jobs' outputs"
    assert not torch.isnan(host[written]).any()


# ---- bn_param_grads --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 63, 64, 65, 300])
def test_bn_param_grads_fp64(C):
    L, lib = _lib()
    g = torch.Generator().manual_seed(500 + C)
    worst = 0.0
    for rows in (1, 4, 33):
        dot = torch.randn(rows, C, generator=g) * 2 + 0.5
        sum_dz = torch.randn(C, generator=g)
        bias = torch.randn(C, generator=g)
        mean = torch.randn(C, generator=g)
        mean[::2] = bias[::2] + 1e-3 * torch.randn(C, generator=g)[::2]
        invstd = torch.rand(C, generator=g) * 3 + 0.1
        scale = torch.randn(C, generator=g)
        d = {k: v.cuda() for k, v in dict(dot=dot, sum_dz=sum_dz, bias=bias, mean=mean, invstd=invstd, scale=scale).items()}
        for with_scale in (True, False):
            for with_bias in (True, False):
                b64 = bias.double() if with_bias else torch.zeros(C, dtype=torch.float64)
                dg_ref = invstd.double() * (dot.double().sum(0) + (b64 - mean.double()) * sum_dz.double())
                dg_bound = 2 * U * (rows + 3) * invstd.double() * (dot.double().abs().sum(0) + (b64 - mean.double()).abs() * sum_dz.double().abs())
                dbias_ref = scale * sum_dz if with_scale else sum_dz          # CPU fp32: one rounding
                for req in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
                    what = (C, rows, with_scale, with_bias, req)
                    bufs = [_nanbuf(C) for _ in range(3)]
                    code = lib.dasac_bn_param_grads(d["dot"].data_ptr(), rows, d["sum_dz"].data_ptr(), d["mean"].data_ptr(),
                                                    d["invstd"].data_ptr(), d["scale"].data_ptr() if with_scale else None,
                                                    d["bias"].data_ptr() if with_bias else None, C,
                                                    *[b.data_ptr() if r else None for b, r in zip(bufs, req)], L.stream_ptr())
                    torch.cuda.synchronize()
                    assert code == 0, what
                    for b, r in zip(bufs, req):
                        if not r:
                            assert torch.isnan(b.cpu()).all(), (what, "an output that was not requested was written")
                    if req[0]:
                        ratio = _ratio(_fenced(bufs[0], C, what), dg_ref, dg_bound)
                        worst = max(worst, ratio)
                        assert ratio <= 1.0, (what, "dgamma", ratio)
                    if req[1]:
                        assert torch.equal(_fenced(bufs[1], C, what), sum_dz), (what, "dbeta")
                    if req[2]:
                        assert torch.equal(_fenced(bufs[2], C, what), dbias_ref), (what, "dbias")
    print("bn_param_grads C={}: worst dgamma got/bound {:.3g}".format(C, worst))


def test_bn_param_grads_beta_and_bias_need_no_dot_and_gamma_without_dot_is_refused():
    from dasac_hip import ops
    L, lib = _lib()
    C = 65
    g = torch.Generator().manual_seed(9)
    sum_dz, scale, mean, invstd = (torch.randn(C, generator=g).cuda() for _ in range(4))
    _, db, dcb = ops.bn_param_grads(None, sum_dz, None, None, scale, None, want_gamma=False, want_beta=True, want_bias=True)
    assert torch.equal(db, sum_dz) and torch.equal(dcb.cpu(), scale.cpu() * sum_dz.cpu())
    out = _nanbuf(C)
    p = sum_dz.data_ptr()
    for dot, rows, m, i in ((None, 1, mean.data_ptr(), invstd.data_ptr()), (p, 0, mean.data_ptr(), invstd.data_ptr()),
                            (p, 1, None, invstd.data_ptr()), (p, 1, mean.data_ptr(), None)):
        assert lib.dasac_bn_param_grads(dot, rows, p, m, i, None, None, C, out.data_ptr(), None, None, L.stream_ptr()) == EINVAL
    assert lib.dasac_bn_param_grads(p, 1, None, mean.data_ptr(), invstd.data_ptr(), None, None, C, out.data_ptr(), None, None, L.stream_ptr()) == EINVAL
    assert lib.dasac_bn_param_grads(p, 1, p, mean.data_ptr(), invstd.data_ptr(), None, None, 0, out.data_ptr(), None, None, L.stream_ptr()) == EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(out.cpu()).all()


# ---- channel_sums ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", [1, 255, 256, 257, 1000, 65 * 65])
def test_channel_sums_fp64(HW):
    from dasac_hip import ops
    worst = 0.0
    for N in (1, 3):
        for C in (1, 5):
            for kind in ("offset", "zero-mean"):
                g = torch.Generator().manual_seed(HW * 31 + N * 7 + C)
                x = torch.randn(N, C, HW, generator=g) + (100.0 if kind == "offset" else 0.0)
                ref = x.double().sum((0, 2))
                bound = 2 * U * ((HW + 255) // 256) * x.double().abs().sum((0, 2))
                buf = _nanbuf(C)
                got = ops.channel_sums(x.cuda(), out=buf[:C])
                assert got.data_ptr() == buf.data_ptr()
                alloc = ops.channel_sums(x.cuda())
                host = _fenced(buf, C, (N, C, HW, kind))
                assert torch.equal(alloc.cpu(), host)
                ratio = _ratio(host, ref, bound)
                worst = max(worst, ratio)
                print("channel_sums N={} C={} HW={} {}: got/bound {:.3g}, yardstick vs ATen fp32 sum {:.3g}".format(
                    N, C, HW, kind, ratio, Y._ratio(host, ref, x.sum((0, 2)))))
                assert ratio <= 1.0, (N, C, HW, kind, ratio)
    print("channel_sums HW={}: worst got/bound {:.3g}".format(HW, worst))


def test_channel_sums_refuses_on_the_host():
    L, lib = _lib()
    x = torch.ones(2 * 3 * 4, device="cuda")
    out = _nanbuf(3)
    for args in ((None, 2, 3, 4, out.data_ptr()), (x.data_ptr(), 2, 3, 4, None), (x.data_ptr(), 2, 3, 1 << 31, out.data_ptr()),
                 (x.data_ptr(), 2, 3, (1 << 31) + 5, out.data_ptr()), (x.data_ptr(), 2, 3, 0, out.data_ptr()),
                 (x.data_ptr(), 0, 3, 4, out.data_ptr()), (x.data_ptr(), 2, 0, 4, out.data_ptr())):
        assert lib.dasac_channel_sums(*args, L.stream_ptr()) == EINVAL, args
    torch.cuda.synchronize()
    assert torch.isnan(out.cpu()).all()
