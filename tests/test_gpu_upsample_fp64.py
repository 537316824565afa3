"""The bilinear half of the head, csrc/upsample.hip -- upsample_softmax<19 | generic, SOFTMAX, NARROW>, q32_to_double, upsample_bwd_x / _y --
against plain float64 ATen on the CPU, through dasac_hip.ops only.

Reference: F.interpolate(x.double(), size, mode="bilinear", align_corners=True), torch.softmax(.., 1) of it times ~ignore, and
autograd through the interpolate for the backward.  Yardstick: the same ATen code in float32 on the CPU.  up, probs (masked) and
the low-resolution gradient follow tests/fp64_yardstick.py: err(HIP vs fp64) <= 2 * err(ATen-fp32 vs fp64) + 1e-6.  No pixel is left
out of any comparison.

Which case reaches which instantiation is asserted, not assumed: `_narrow` restates the launcher's shared-tap predicate in numpy
float32 (dasac_upsample_softmax: col(d) = min(int(sw * d), w - 1), narrow iff col(min(ox + 3, W - 1)) - col(ox) <= 1 for every
quad start ox), `_grid` its grid, and every case names the path it must take:
  <19, *, NARROW>       C = 19, predicate true: factor 8 (W % 4 == 1), a non-integer factor (W % 4 == 2), extent-1 inputs and
                        outputs (scale 0), the 1030 x 1030 second pass
  <19, *, false>        C = 19, predicate false: factor 7/4 (9x6 -> 21x12), factor 1, shrinking both ways
  <kMaxC, *, false>     every other C <= 32: C = 1, 2, 21, 32 with the shared-tap branch taken by every quad at run time
                        (W % 4 == 3), C = 2 with quads on the per-pixel branch, column indices up to 2048, both second passes
Every case runs the logits-only launch (SOFTMAX = false), up + probs + sums, and probs + sums without up (SOFTMAX = true).

Exact conditions next to the toleranced ones: up is the same bits from the logits-only and the softmax kernels; want_up=False
changes no bit of probs or sums; probs is 0.0 wherever ignore is set; sums (of the UNMASKED softmax) is the same bits with and
without an ignore mask and between two runs; image b of a batch is the same bits as the one-image call; at factor 1, and on the
8-grid of an exact factor 8, up is the input bit for bit (weights 1 and 0); C = 33 is refused.

Class sums are held to the kernel's own (verified) probs, summed in float64, with a bound read off the code: a thread adds
n_t = 4 * ipt non-negative fp32 terms serially (ipt items of 4 pixels), a wave adds 6 shuffle levels -- (n_t + 6) roundings of at
most 2^-24 relative to a partial sum that never exceeds the total; a wave partial is rounded once to Q32 (2^-33 absolute), the
integer adds and the final conversion are exact:
    |sums[c] - S64[c]| <= (n_t + 6) * 2^-24 * S64[c] + n_waves * 2^-33,   n_waves = 4 * grid * B.

Measured on the MI355X, worst err_hip / (2 * err_aten + 1e-6) per group (every test prints its own; no case needed more than the
factor 2):
  up             0.25 at logit scales 3 and 50 (small shapes), 0.13 with 1e4 added; second pass 0.27 / 0.47 / 0.44 (generic
                 softmax / 19-class narrow / logits-only C = 1)
  probs          0.34 at scale 3, 0.59 at scale 50 ((2, 19, 9, 6, 21, 12)); second pass 0.34 / 0.49; 0.74 with 1e4 added to
                 every class -- the largest: the interpolation rounds at the spacing of fp32 near 1e4 (1e-3) and the softmax sees
                 those roundings at full size; the fp32 restatement of the tap arithmetic (oracle/head_ref.py) gives the same
                 0.74 on the CPU, so it belongs to the order of the tap arithmetic, not to the kernel's code
  upsample_bwd   0.19 ((1, 19, 13, 9, 6, 5), shrinking), with and without gscale; second pass 0.08 / 0.09
  class sums     at most 0.24 of the bound on the small shapes (one item per thread: the bound is ten roundings), 0.0018 of
                 it on the second pass (two items per thread, 4096 waves)
A ratio of 0.5 is an error equal to float32 ATen's.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fp64_yardstick import _ratio, _report

pytestmark = pytest.mark.gpu
GSCALE = 0.37
K_NUM_CU = 256       # common.hpp kNumCu
K_HB = 256           # head_common.hpp kHB: threads per block of the head's streaming kernels


# ---- the launcher, restated ----------------------------------------------------------------------------------------------------
def _ac_scale(n_in, n_out):
    """bilinear.hpp ac_scale, in float32"""
    return np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0.0)


def _narrow(w, W):
    """dasac_upsample_softmax's `narrow` loop (upsample.hip, "tap_ac's column arithmetic, on the host"): one fp32 multiply per column"""
    sw = _ac_scale(w, W)

    def col(d):
        return min(int(sw * np.float32(d)), w - 1)
    return all(col(min(ox + 3, W - 1)) - col(ox) <= 1 for ox in range(0, W, 4))


def _grid(B, H, W, softmax):
    """(grid.x, items per thread, waves that add a class-sum partial) of dasac_upsample_softmax (upsample.hip: `items`, `total` =
    stream_grid(B * items, kHB, softmax ? kNumCu * 4 : kNumCu * 16) and `grid`); stream_grid is common.hpp's: ceil(work / block)
    clamped to [1, max_blocks]."""
    items = H * ((W + 3) // 4)
    cap = K_NUM_CU * 4 if softmax else K_NUM_CU * 16
    total = max(1, min((B * items + K_HB - 1) // K_HB, cap))
    grid = max(1, min((items + K_HB - 1) // K_HB, (total + B - 1) // B))
    ipt = (items + grid * K_HB - 1) // (grid * K_HB)
    return grid, ipt, 4 * grid * B


def _default_cap():
    """stream_grid's default max_blocks (common.hpp): (kNumCu - reserved_cus()) * 16"""
    from dasac_hip import lib as L
    return (K_NUM_CU - L.load().dasac_reserved_cus()) * 16


# ---- cases: (B, C, h, w, H, W), kernel ("19" | "generic"), the launcher's predicate -----------------------------------------------
CASES = [
    ((2, 19, 5, 7, 33, 49), "19", True),        # <19,*,NARROW>, factor 8, W % 4 == 1
    ((1, 19, 3, 4, 9, 10), "19", True),         # <19,*,NARROW>, non-integer factor, W % 4 == 2
    ((2, 19, 9, 6, 21, 12), "19", False),       # <19,*,false>: some quad spans three low-res columns
    ((1, 19, 7, 7, 7, 7), "19", False),         # <19,*,false>, factor 1
    ((1, 19, 13, 9, 6, 5), "19", False),        # <19,*,false>, shrinking both ways, a one-pixel tail quad
    ((1, 19, 1, 1, 5, 7), "19", True),          # extent-1 input: both scales 0
    ((2, 19, 4, 5, 1, 1), "19", True),          # extent-1 output: both scales 0
    ((1, 19, 5, 1, 33, 9), "19", True),         # extent-1 width
    ((2, 1, 5, 7, 19, 27), "generic", True),    # generic kernel, every quad on the shared-tap branch, W % 4 == 3; C = 1
    ((2, 2, 5, 7, 19, 27), "generic", True),
    ((2, 21, 5, 7, 19, 27), "generic", True),
    ((2, 32, 5, 7, 19, 27), "generic", True),   # C = kMaxC
    ((1, 2, 9, 6, 21, 12), "generic", False),   # generic kernel, quads on the per-pixel tap branch
    ((1, 3, 1, 257, 1, 2049), "generic", True), # large column indices
]
SECOND_PASS = [
    ((1, 2, 9, 9, 1030, 1030), "generic", True, True),        # generic softmax kernels: 265740 items > 1024 blocks x 256
    ((1, 19, 129, 129, 1030, 1030), "19", True, True),        # <19,true,NARROW>, the same grid
    ((1, 1, 33, 33, 2052, 2052), "generic", True, False),     # <kMaxC,false,false>, C = 1: 1052676 items > 4096 blocks x 256
]
BWD_SECOND_PASS = (1, 2, 131074, 2, 262147, 3)    # planes * H * w = 1048588 > 4096 x 256; both scales are exactly 1/2


def _id(shape):
    return "x".join(map(str, shape))


def test_every_case_takes_the_path_its_comment_names():
    for shape, kernel, narrow in CASES + [c[:3] for c in SECOND_PASS]:
        B, C, h, w, H, W = shape
        assert ("19" if C == 19 else "generic") == kernel and C <= 32, shape
        assert _narrow(w, W) == narrow, shape
    reached = {(k, n) for _, k, n in CASES}
    assert reached == {("19", True), ("19", False), ("generic", True), ("generic", False)}
    assert {s[5] % 4 for s, _, _ in CASES} == {0, 1, 2, 3}
    assert (CASES[0][0][5] % 4, CASES[1][0][5] % 4, CASES[8][0][5] % 4) == (1, 2, 3)
    assert CASES[4][0][5] % 4 == 1 and CASES[4][0][5] > 4                    # a full quad and a one-pixel tail


# ---- forward -------------------------------------------------------------------------------------------------------------------
def _reference(x, size, ign, dtype):
    up = F.interpolate(x.to(dtype), size, mode="bilinear", align_corners=True)
    return up, torch.softmax(up, 1) * (~ign)[:, None]


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check_forward(what, shape, x, seed):
    from dasac_hip import ops
    B, C, h, w, H, W = shape
    ign = torch.rand(B, H, W, generator=torch.Generator().manual_seed(seed)) < 0.2
    # the logits sit between NaNs: a tap read past the last plane poisons the output even where its weight is 0 (the clamped
    # columns k1 / k2 of the shared-tap path, i1 on the last row and column)
    fence = torch.full((x.numel() + 64,), float("nan")).cuda()
    fence[32:32 + x.numel()] = x.flatten().cuda()
    xd, ignd = fence[32:32 + x.numel()].view(x.shape), ign.cuda()
    up0, none_p, none_s = ops.upsample_softmax(xd, (H, W))                                              # SOFTMAX = false
    assert none_p is None and none_s is None
    up1, probs1, sums1 = ops.upsample_softmax(xd, (H, W), ignd, want_probs=True, want_sums=True)
    none_u, probs2, sums2 = ops.upsample_softmax(xd, (H, W), ignd, want_up=False, want_probs=True, want_sums=True)
    _, probs3, sums3 = ops.upsample_softmax(xd, (H, W), None, want_up=False, want_probs=True, want_sums=True)
    assert none_u is None and up0.shape == (B, C, H, W) and sums1.shape == (C,) and sums1.dtype == torch.float64
    assert _bits_equal(up0, up1)                                          # the logits-only kernel and the softmax kernel
    assert _bits_equal(probs1, probs2) and torch.equal(sums1, sums2)      # up == NULL changes nothing; a second run: the same sums
    assert torch.equal(sums1, sums3)                                      # the sums are of the unmasked softmax
    assert float((probs1 * ignd[:, None]).abs().max()) == 0.0             # exactly 0 (no NaN either) where ignored
    keep = (~ignd)[:, None].expand_as(probs1)
    assert _bits_equal(probs1[keep], probs3[keep])                        # the mask only zeroes
    if B > 1:
        for b in range(B):
            ub, pb, _ = ops.upsample_softmax(xd[b:b + 1], (H, W), ignd[b:b + 1], want_probs=True, want_sums=True)
            assert _bits_equal(ub[0], up1[b]) and _bits_equal(pb[0], probs1[b]), b
    if (h, w) == (H, W):
        assert _bits_equal(up0, xd)                                       # factor 1: weights exactly 1 and 0

    u64, p64 = _reference(x, (H, W), ign, torch.float64)
    u32, p32 = _reference(x, (H, W), ign, torch.float32)
    ratios = {"up": _ratio(up1, u64, u32), "probs": _ratio(probs1, p64, p32)}

    # class sums against the kernel's own probs (held to the reference just above, unmasked ones bit-equal where not ignored)
    grid, ipt, n_waves = _grid(B, H, W, True)
    S64 = probs3.double().sum((0, 2, 3)).cpu()
    bound = (4 * ipt + 6) * 2.0 ** -24 * S64 + n_waves * 2.0 ** -33
    share = float(((sums3.cpu() - S64).abs() / bound).max())
    print("{} {}: class sums use {:.3g} of their bound (grid {}, {} items per thread)".format(what, shape, share, grid, ipt))
    assert share <= 1.0, (what, shape, share)
    _report(what, shape, ratios)


def _logits(shape, scale, seed):
    B, C, h, w, _, _ = shape
    return torch.randn(B, C, h, w, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("scale", [3.0, 50.0], ids=["s3", "s50"])
@pytest.mark.parametrize("case", CASES, ids=[_id(c[0]) for c in CASES])
def test_upsample_softmax_against_fp64(case, scale):
    """logits of scale 3, and of scale 50: a saturating softmax"""
    shape = case[0]
    _check_forward("upsample_softmax s{:g}".format(scale), shape, _logits(shape, scale, sum(shape)), sum(shape) + 1)


def test_upsample_softmax_subtracts_the_maximum():
    """1e4 added to every class: exp() of the raw values overflows; the spacing of fp32 at 1e4 (1e-3) is in the yardstick too"""
    shape = CASES[0][0]
    _check_forward("upsample_softmax +1e4", shape, _logits(shape, 3.0, 7) + 1e4, 8)


@pytest.mark.parametrize("case", SECOND_PASS, ids=[_id(c[0]) for c in SECOND_PASS])
def test_upsample_softmax_second_pass_of_the_capped_grid(case):
    """The smallest shapes at which some thread takes a second item: the softmax kernels' cap is kNumCu * 4 blocks over the
    whole batch, the logits-only kernels' kNumCu * 16."""
    shape, _, _, softmax = case
    B, _, _, _, H, W = shape
    grid, ipt, _ = _grid(B, H, W, softmax)
    items = H * ((W + 3) // 4)
    assert ipt >= 2 and items > grid * K_HB and grid * B == (K_NUM_CU * 4 if softmax else K_NUM_CU * 16)
    assert _grid(B, H, W, True)[1] >= 2                      # every shape loops in the softmax launches of _check_forward
    _check_forward("upsample_softmax grid-stride", shape, _logits(shape, 3.0, sum(shape)), sum(shape) + 1)


@pytest.mark.parametrize("C", [19, 3])
def test_upsample_at_an_exact_integer_factor_returns_the_input_on_its_grid(C):
    """13 x 9 -> 97 x 65: both scales are exactly 1/8, every eighth output sits on a source pixel with weights 1 and 0"""
    from dasac_hip import ops
    x = torch.randn(2, C, 13, 9, generator=torch.Generator().manual_seed(C)) * 3
    assert _ac_scale(13, 97) == 0.125 and _ac_scale(9, 65) == 0.125 and _narrow(9, 65)
    up0, _, _ = ops.upsample_softmax(x.cuda(), (97, 65))
    up1, _, _ = ops.upsample_softmax(x.cuda(), (97, 65), want_probs=True)
    assert _bits_equal(up0[..., ::8, ::8].contiguous(), x.cuda()) and _bits_equal(up1[..., ::8, ::8].contiguous(), x.cuda())


def test_more_than_32_classes_are_refused():
    from dasac_hip import ops
    from dasac_hip.lib import DasacError
    x = torch.randn(1, 33, 2, 2).cuda()
    for kw in ({}, {"want_probs": True, "want_sums": True}):
        with pytest.raises(DasacError, match="bad shape"):
            ops.upsample_softmax(x, (4, 4), **kw)


# ---- backward ------------------------------------------------------------------------------------------------------------------
def _bwd_reference(g, low_hw, dtype):
    """d sum(g * interpolate(x)) / dx: the transpose of the (linear) upsampling applied to g, in `dtype` on the CPU"""
    B, C, _, _ = g.shape
    x = torch.zeros(B, C, *low_hw, dtype=dtype, requires_grad=True)
    up = F.interpolate(x, g.shape[2:], mode="bilinear", align_corners=True)
    (d,) = torch.autograd.grad(up, x, g.to(dtype))
    return d


def _check_backward(what, shape):
    from dasac_hip import ops
    B, C, h, w, H, W = shape
    g = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(sum(shape) + 2))
    d64, d32 = _bwd_reference(g, (h, w), torch.float64), _bwd_reference(g, (h, w), torch.float32)
    plain = ops.upsample_bwd(g.cuda(), (h, w))
    scaled = ops.upsample_bwd(g.cuda(), (h, w), torch.tensor([GSCALE]).cuda())
    assert plain.shape == (B, C, h, w)
    _report(what, shape, {"gscale None": _ratio(plain, d64, d32), "gscale 0.37": _ratio(scaled, GSCALE * d64, GSCALE * d32)})


@pytest.mark.parametrize("case", CASES, ids=[_id(c[0]) for c in CASES])
def test_upsample_bwd_against_fp64_autograd(case):
    _check_backward("upsample_bwd", case[0])


def test_upsample_bwd_second_pass_of_the_capped_grid():
    """planes * H * w exceeds stream_grid's default cap times 256: upsample_bwd_x takes a second item (w = 2 keeps it small)"""
    B, C, h, w, H, W = BWD_SECOND_PASS
    assert B * C * H * w > _default_cap() * K_HB
    _check_backward("upsample_bwd grid-stride", BWD_SECOND_PASS)


def test_upsample_bwd_refuses_a_workspace_one_byte_short():
    from dasac_hip import lib as L
    lib = L.load()
    planes, h, w, H, W = 6, 5, 7, 33, 49
    need = lib.dasac_upsample_bwd_workspace(planes, H, w)
    assert need == planes * H * w * 4
    g = torch.randn(planes, H, W).cuda()
    out = torch.full((planes, h, w), 7.0).cuda()
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert lib.dasac_upsample_bwd(g.data_ptr(), planes, h, w, H, W, 0, out.data_ptr(), ws.data_ptr(), need - 1, L.stream_ptr()) != 0
    assert b"workspace" in lib.dasac_last_error()
    assert bool((out == 7.0).all())                                        # nothing was launched
    assert lib.dasac_upsample_bwd(g.data_ptr(), planes, h, w, H, W, 0, out.data_ptr(), ws.data_ptr(), need, L.stream_ptr()) == 0
    assert not bool((out == 7.0).any())
