"""The SAC head's loss and view-fusion kernels (csrc/cross_entropy.hip: ce_loss, ce_bwd_rows / ce_bwd_rows_wave + conf_pixel_sums;
csrc/warp.hip: warp_affine, warp_pool / warp_pool_avg, warp_back) against plain float64 ATen on the CPU, through dasac_hip.ops only.

Reference: F.cross_entropy / autograd (through F.interpolate(bilinear, align_corners=True) for the low-resolution gradient),
F.affine_grid + F.grid_sample(bilinear, zeros, align_corners=False), and the two poolings of sac.py:218-269 written out below,
all in float64.  Yardstick: the same ATen code in float32 on the CPU.  For every compared tensor, with conftest's rel_err,
    err(HIP vs fp64) <= 2 * err(ATen-fp32 vs fp64) + 1e-6
(the factor of test_resnet101_gradients_fp64_arbitration; 1e-6 is about 8 fp32 ulp of the tensor's max and covers the cases where
ATen lands exactly).  per_class gets 2^-29 absolute on top: its Q28 accumulation rounds each pixel's term by at most 2^-29 and the
sum is divided by B*HW.  Exact conditions sit next to the toleranced ones: dlogits is 0 at every ignored pixel, the mask is 0.0 or
1.0 and equals the reference's, pixels that sample nothing are exactly 0, want_aligned=False changes no bit of pooled / mask.

Discontinuities (the mask thresholds Z > tol and per-view sum < 0.1, the arg-min over view entropies) cannot be held to fp32
arithmetic at the threshold.  Pixels are left out of the pooled / mask comparison by the float64 reference alone: |Z - tol| < 1e-4
(both poolings); in min-entropy pooling also a view's probability sum within 1e-4 of 0.1, or the two lowest view entropies closer
than 1e-4 * max(1, |entropy|) (1e-4 is about 10x the fp32 error of a 32-term entropy; a pixel whose views are ALL empty is kept:
the first view wins on both sides).  The view-sum and entropy rules are not applied to avg pooling, which has no discontinuity
there.  The excluded share is asserted to be <= 0.5 % of a case's pixels.

Measured on the MI355X, worst err_hip / (2 * err_aten + 1e-6) per group (every test prints its own; no case needed more than
the factor 2):
  ce_loss               loss 0.076, dlogits 0.13, per_class 0.074 (small shapes: the 1e-6 floor is most of the bound);
                        second pass of the capped grid (2097159 pixels): loss 0.004, dlogits 0.16, per_class 0.031
  low-resolution grad   0.39 (the 19-class up-factors ~1 and 2), at most 0.16 on every other case
  warp_affine           0.50 random affines, 0.44 mirrored ones; wholly outside: exactly 0
  warp_pool avg         aligned 0.56, pooled 0.66
  warp_pool min-entropy aligned 0.56, pooled 0.59
  warp_back             0.47 (second pass of the capped grid)
A ratio of 0.5 is an error equal to float32 ATen's.  Excluded share per pooling case: 0 for every small shape in both modes but
(4, 2, 2, 31, 64) min-entropy 3.8e-4; (32, 1, 19, 182, 182) avg 1.4e-5; (32, 2, 3, 182, 182) min-entropy 1.5e-4.
"""
import pytest
import torch
import torch.nn.functional as F

from fp64_yardstick import _ratio, _report

pytestmark = pytest.mark.gpu
GSCALE = 0.37
EPS = 1e-5           # sac.py:189 entropy epsilon
MARGIN = 1e-4        # half-width of the excluded band around a discontinuity
MAX_EXCLUDED = 5e-3


# ---- cross entropy ---------------------------------------------------------------------------------------------------------
def _ce_reference(x, y, cw, conf, dtype, size=None):
    """(loss, GSCALE * d loss / d x, per_class) of the CE on x (or on x upsampled to `size`), in `dtype` on the CPU.
    mode 0 (conf None): mean over ALL pixels of CE(weight, ignore 255); mode 1: sac.py:148's [B,B,H,W] broadcast
    (conf[:,0].sum(0) * ce.sum(0)).sum() / (B*B*H*W).  per_class as sac.py:138-145: ce scattered by label (ignored pixels into
    class 0 with ce = 0), mean over pixels, mean over images."""
    x = x.detach().to(dtype).requires_grad_(True)
    up = x if size is None else F.interpolate(x, size, mode="bilinear", align_corners=True)
    ce = F.cross_entropy(up, y, weight=cw.to(dtype), ignore_index=255, reduction="none")
    B, H, W = ce.shape
    if conf is None:
        loss = ce.mean()
    else:
        loss = (conf[:, 0].to(dtype).sum(0) * ce.sum(0)).sum() / (B * B * H * W)
    (g,) = torch.autograd.grad(loss, x)
    with torch.no_grad():
        idx = y.clone()
        idx[y == 255] = 0
        pc = torch.zeros_like(up).scatter_(1, idx[:, None], ce[:, None]).flatten(2).mean(-1).mean(0)
    return loss.detach().view(1), g * GSCALE, pc


def _ce_inputs(B, C, H, W, mode, scale, seed):
    """logits of the given scale; ~30 % labels 255, the last image fully ignored (B > 1), the last class absent (C > 2: with two
    classes it would leave only the zero-weight one), class weights in (0.1, 1.1) with class 1's exactly 0; confidences for mode 1"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g) * scale
    y = torch.randint(0, C - 1 if C > 2 else C, (B, H, W), generator=g)
    y[torch.rand(B, H, W, generator=g) < 0.3] = 255
    if B > 1:
        y[-1] = 255
    y[0, 0, 0] = 0                                       # at least one pixel that carries loss, whatever the draw
    cw = torch.rand(C, generator=g) + 0.1
    cw[1] = 0.0
    conf = torch.rand(B, 1, H, W, generator=g) if mode else None
    return x, y, cw, conf


def _ce_on_gpu(x, y, cw, conf):
    from dasac_hip import ops
    gs = torch.tensor([GSCALE]).cuda()
    return ops.ce_loss(x.cuda(), y.cuda(), cw.cuda(), None if conf is None else conf.cuda(), want_grad=True, want_per_class=True, gscale=gs)


def _ce_check(what, case, x, y, cw, conf):
    B, _, H, W = x.shape
    loss, dl, pc = _ce_on_gpu(x, y, cw, conf)
    l64, g64, p64 = _ce_reference(x, y, cw, conf, torch.float64)
    l32, g32, p32 = _ce_reference(x, y, cw, conf, torch.float32)
    dl = dl.cpu()
    assert float((dl * (y == 255)[:, None]).abs().max()) == 0.0          # ignored pixels: exactly no gradient
    _report(what, case, {"loss": _ratio(loss, l64, l32), "dlogits": _ratio(dl, g64, g32),
                         "per_class": _ratio(pc, p64, p32, extra_abs=2.0 ** -29)})


# (B, C, H, W), logit scale; each runs in mode 0 (plain mean) and mode 1 (confidence-weighted B x B broadcast)
CE_CASES = [
    ((2, 19, 4, 5), 3.0),      # ce_loss<19>, HW % 4 == 0: dwordx4 loads and stores only
    ((2, 19, 3, 7), 3.0),      # ce_loss<19>, HW % 4 == 1: scalar tail of one pixel
    ((2, 19, 3, 6), 3.0),      # ce_loss<19>, HW % 4 == 2
    ((3, 19, 5, 3), 3.0),      # ce_loss<19>, HW % 4 == 3; B = 3: the cross-image product of mode 1
    ((2, 19, 1, 1), 3.0),      # ce_loss<19>, HW = 1 < one quad: the tail is all there is
    ((2, 19, 1, 3), 3.0),      # ce_loss<19>, HW = 3
    ((3, 2, 5, 7), 3.0),       # ce_loss<kMaxC> (runtime class count), C = 2
    ((3, 7, 5, 7), 3.0),       # ce_loss<kMaxC>, C = 7
    ((3, 32, 5, 7), 3.0),      # ce_loss<kMaxC>, C = kMaxC
    ((2, 7, 1, 2), 3.0),       # ce_loss<kMaxC>, HW = 2: tail only
    ((1, 19, 3, 7), 3.0),      # B = 1: mode 1's B x B broadcast degenerates to conf * ce
    ((2, 19, 3, 7), 40.0),     # logits of scale 40: the softmax must subtract the maximum
]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("case", CE_CASES, ids=["{}_s{:g}".format("x".join(map(str, s)), sc) for s, sc in CE_CASES])
def test_ce_loss_against_fp64(case, mode):
    (B, C, H, W), scale = case
    x, y, cw, conf = _ce_inputs(B, C, H, W, mode, scale, seed=B + C + H + W + mode)
    _ce_check("ce_loss", (case, mode), x, y, cw, conf)


@pytest.mark.parametrize("mode", [0, 1])
def test_ce_loss_second_pass_of_the_capped_grid(mode):
    """One full pass of the capped grid (ce_blocks: kNumCu * 8 blocks of 256 threads with 4 pixels each) plus 7 pixels: the
    second trip of the grid-stride loop, ending in a ragged quad (ce_loss<kMaxC>, C = 2, 17 MB of logits).  The cap is read from
    the workspace size, which is ce_blocks doubles (rounded up to 256 bytes) + 256 bytes of per-class slots.  |ce| stays far below
    the documented Q28 clamp of 4096."""
    from dasac_hip import lib as L
    lib = L.load()
    cap = (lib.dasac_ce_loss_workspace(1, 2, 1 << 30) - 256) // 8
    assert cap == (lib.dasac_ce_loss_workspace(1, 2, 1 << 29) - 256) // 8 and cap % 32 == 0      # saturated: the cap itself
    HW = cap * 256 * 4 + 7
    assert (lib.dasac_ce_loss_workspace(1, 2, HW) - 256) // 8 == cap
    x, y, cw, conf = _ce_inputs(1, 2, 1, HW, mode, 3.0, seed=mode)
    _ce_check("ce_loss grid-stride", (HW, mode), x, y, cw, conf)


def test_ce_loss_labels_outside_the_class_range_carry_nothing():
    """A label of 200 at C = 19 is treated like 255: no loss, no gradient, no per-class term (include/dasac_hip.h)."""
    x, y, cw, conf = _ce_inputs(2, 19, 3, 7, 1, 3.0, seed=5)
    y200 = y.clone()
    y200[0, 1, 2], y200[0, 2, 5], y[0, 1, 2], y[0, 2, 5] = 200, 200, 255, 255
    for c in (None, conf):
        la, da, pa = _ce_on_gpu(x, y, cw, c)
        lb, db, pb = _ce_on_gpu(x, y200, cw, c)
        assert float(la) != 0.0 and torch.equal(la, lb) and torch.equal(da, db) and torch.equal(pa, pb)
        assert float(db[0, :, 1, 2].abs().max()) == 0.0 and float(db[0, :, 2, 5].abs().max()) == 0.0


# ---- the low-resolution gradient ---------------------------------------------------------------------------------------------
# (B, C, h, w, H, W), mode: the shapes of test_ce_backward_straight_into_the_low_resolution_gradient without its two workload
# sizes (that test holds the kernels to the two-kernel path bit for bit; this one holds them to autograd of the composite)
LOW_CASES = [
    ((2, 19, 9, 13, 65, 97), 1),     # conf_pixel_sums + ce_bwd_rows_wave<19,16>: up-factor 8, 15 taps, 17 row chunks, W % 4 = 1
    ((3, 19, 5, 7, 33, 49), 0),      # ce_bwd_rows_wave<19,16>, mode 0
    ((1, 7, 4, 6, 8, 12), 1),        # ce_bwd_rows<kMaxC>: C = 7, B = 1 (each block adds the confidences itself)
    ((2, 19, 5, 6, 38, 46), 1),      # conf_pixel_sums + ce_bwd_rows_wave<19,24>: up-factor 9, 17 taps
    ((2, 19, 7, 9, 50, 71), 0),      # ce_bwd_rows_wave<19,24>: 18 taps, W % 4 = 3 (rotated last quad)
    ((1, 19, 33, 33, 33, 35), 0),    # ce_bwd_rows_wave<19,16>: up-factor ~1, 3 taps
    ((2, 19, 3, 4, 10, 3), 1),       # conf_pixel_sums + ce_bwd_rows<19>: W < 4 (no full quad), shrinking in x
    ((2, 19, 20, 30, 40, 60), 1),    # conf_pixel_sums + ce_bwd_rows_wave<19,16>: up-factor 2
    ((1, 19, 5, 5, 65, 65), 0),      # ce_bwd_rows<19>: up-factor 16, 35 positions per column (> 24: the loop form of phase 2)
    ((1, 19, 9, 9, 65, 65), 1),      # ce_bwd_rows<19>: B = 1 with confidences
    ((1, 19, 5, 6, 38, 46), 1),      # ce_bwd_rows<19>: B = 1 with confidences at a wave<24> geometry -- no conf_pixel_sums
    ((2, 19, 3, 2, 20, 49), 1),      # ce_bwd_rows<19>: up-factor 48 > 16, the workspace has no room for the confidence sums --
                                     # every block adds the B confidences itself; 49 positions per column
    ((2, 32, 3, 5, 17, 33), 1),      # conf_pixel_sums + ce_bwd_rows<kMaxC>: C = 32
]


@pytest.mark.parametrize("shape,mode", LOW_CASES, ids=["{}_m{}".format("x".join(map(str, s)), m) for s, m in LOW_CASES])
def test_ce_loss_bwd_low_against_fp64_autograd_of_the_composite(shape, mode):
    from dasac_hip import ops
    B, C, h, w, H, W = shape
    _, y, cw, conf = _ce_inputs(B, C, H, W, mode, 3.0, seed=sum(shape))
    low = torch.randn(B, C, h, w, generator=torch.Generator().manual_seed(sum(shape) + 1)) * 3
    up, _, _ = ops.upsample_softmax(low.cuda(), (H, W))
    got = ops.ce_loss_bwd_low(up, y.cuda(), (h, w), cw.cuda(), None if conf is None else conf.cuda(),
                              gscale=torch.tensor([GSCALE]).cuda())
    _, g64, _ = _ce_reference(low, y, cw, conf, torch.float64, size=(H, W))
    _, g32, _ = _ce_reference(low, y, cw, conf, torch.float32, size=(H, W))
    _report("ce_loss_bwd_low", (shape, mode), {"dlow": _ratio(got, g64, g32)})


# ---- affine warps ------------------------------------------------------------------------------------------------------------
def _warp(x, theta):
    """sac.py:289-290: affine_grid + grid_sample(bilinear, zeros, align_corners=False), in x's dtype"""
    grid = F.affine_grid(theta.to(x.dtype), list(x.shape), align_corners=False)
    return F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)


def _eye(n):
    return torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]).repeat(n, 1, 1)


def _random_thetas(n, g):
    return _eye(n) + 0.25 * torch.randn(n, 2, 3, generator=g)


def _inverse(theta):
    """float64 matrix inverse of the affines, rounded to fp32"""
    m = torch.zeros(theta.shape[0], 3, 3, dtype=torch.float64)
    m[:, :2] = theta.double()
    m[:, 2, 2] = 1.0
    return torch.linalg.inv(m)[:, :2].float().contiguous()


def _mirrored_thetas(B, H, W):
    """the workload's view affines with the guided h-flip on (theta[0,0] < 0): the plain mirror puts every tap on an integer
    source coordinate.  One-row / one-column maps have no half extent to normalise a shift by: the plain mirror only."""
    from oracle import head_ref
    if H < 2 or W < 2:
        return torch.tensor([[-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]).repeat(B, 1, 1)
    params = [(0, 0, 0.0, 1.0, -1), (3, -5, 0.0, 1.0, -1), (2, 4, 10.0, 1.2, -1), (-4, 1, -7.0, 0.8, -1)]
    theta, _ = head_ref.view_affines([params[i % 4] for i in range(B)], H, W)
    assert bool((theta[:, 0, 0] < 0).all())
    return theta


# (B, C, H, W)
WARP_CASES = [
    (4, 3, 33, 49),          # several blocks per image, odd sizes
    (2, 1, 1, 7),            # a single row: every vertical neighbour is outside
    (2, 2, 9, 1),            # a single column
    (2, 19, 1, 1),           # a single pixel
    (64, 1, 129, 129),       # grid cap (4096 + B - 1) / B = 64 blocks = 16384 pixels < 16641: the loop's second pass
]


@pytest.mark.parametrize("kind", ["random", "mirrored"])
@pytest.mark.parametrize("shape", WARP_CASES, ids=["x".join(map(str, s)) for s in WARP_CASES])
def test_warp_affine_against_fp64(shape, kind):
    from dasac_hip import ops
    B, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, C, H, W, generator=g)
    theta = _random_thetas(B, g) if kind == "random" else _mirrored_thetas(B, H, W)
    got = ops.warp_affine(x.cuda(), theta.cuda())
    _report("warp_affine", (shape, kind), {"out": _ratio(got, _warp(x.double(), theta), _warp(x, theta))})


@pytest.mark.parametrize("shape", WARP_CASES, ids=["x".join(map(str, s)) for s in WARP_CASES])
def test_warp_affine_samples_wholly_outside_the_image_are_exactly_zero(shape):
    """50 * [I | (2, 2)] and a translation by 10: every sample lands far outside (the kernel's clamp of wild coordinates), and
    grid_sample's zero padding makes the output exactly 0."""
    from dasac_hip import ops
    B, C, H, W = shape
    x = torch.randn(B, C, H, W, generator=torch.Generator().manual_seed(1)) + 5.0
    theta = _eye(B)
    theta[0::2] = 50.0 * torch.tensor([[1.0, 0.0, 2.0], [0.0, 1.0, 2.0]])
    theta[1::2, :, 2] = 10.0
    assert float(_warp(x.double(), theta).abs().max()) == 0.0
    assert float(ops.warp_affine(x.cuda(), theta.cuda()).abs().max()) == 0.0


# ---- warp + pool -------------------------------------------------------------------------------------------------------------
def _pool_reference(probs, theta, theta_inv, T, mode, tol, dtype):
    """sac.py:289-305 followed by _avg_pool (sac.py:238-269) or _minentropy_pool (sac.py:218-236) for whole groups on one rank,
    in `dtype`.  Returns aligned [N*T,C,H,W], pooled [N,C,H,W], mask [N,1,H,W] (bool) and, for the exclusion rule, Z [N,1,H,W],
    the per-view sums [N,T,H,W] and the per-view entropies [N,T,H,W] (None for avg pooling)."""
    p = probs.to(dtype)
    NT, C, H, W = p.shape
    N = NT // T
    aligned = _warp(p, theta)
    cov = _warp(torch.ones(NT, 1, H, W, dtype=dtype), theta_inv)
    v = (aligned * cov).view(N, T, C, H, W)
    vs = v.sum(2)                                                   # [N,T,H,W]
    if mode == "avg_pool":
        S = v.sum(1)
        Z = S.sum(1, keepdim=True)
        return aligned, S / Z.clamp_min(1e-3), Z > tol, Z, vs, None
    ent = -(v * torch.log((v + EPS) / (1 + EPS))).sum(2)
    ent[vs < 0.1] = 1.0 / EPS
    first = ent.argmin(1, keepdim=True)                             # the first minimum
    pooled = v.gather(1, first[:, :, None].expand(N, 1, C, H, W))[:, 0]
    Z = vs.sum(1, keepdim=True)
    return aligned, pooled, Z > tol, Z, vs, ent


def _excluded(mode, tol, Z, vs, ent):
    """[N,1,H,W] bool, from the float64 reference alone (module docstring)"""
    ex = (Z - tol).abs() < MARGIN
    if mode == "minentropy_pool":
        ex |= ((vs - 0.1).abs() < MARGIN).any(1, keepdim=True)
        if ent.shape[1] > 1:
            two = ent.topk(2, dim=1, largest=False).values
            close = (two[:, 1] - two[:, 0]) < MARGIN * two[:, 0].abs().clamp_min(1.0)
            all_empty = (vs < 0.1).all(1)
            ex |= (close & ~all_empty)[:, None]
    return ex


def _pool_inputs(shape):
    N, Tn, C, H, W = shape
    g = torch.Generator().manual_seed(sum(shape))
    probs = torch.softmax(3 * torch.randn(N * Tn, C, H, W, generator=g), 1)
    probs = probs * (torch.rand(N * Tn, 1, H, W, generator=g) >= 0.15)
    theta = _random_thetas(N * Tn, g)
    return probs, theta, _inverse(theta)


# (N, T, C, H, W), modes
POOL_CASES = [
    ((2, 4, 19, 33, 49), ("avg_pool", "minentropy_pool")),    # avg: warp_pool_avg<19,4>; min-entropy: generic warp_pool
    ((3, 2, 19, 21, 30), ("avg_pool", "minentropy_pool")),    # avg: warp_pool_avg<19,2>
    ((2, 1, 19, 9, 13), ("avg_pool", "minentropy_pool")),     # avg: warp_pool_avg<19,1>; a single view is its own arg-min
    ((2, 3, 19, 17, 23), ("avg_pool", "minentropy_pool")),    # T = 3: generic warp_pool in both modes
    ((2, 4, 7, 22, 9), ("avg_pool", "minentropy_pool")),      # C = 7: generic warp_pool
    ((2, 2, 32, 1, 7), ("avg_pool", "minentropy_pool")),      # C = kMaxC, a single row
    ((2, 5, 19, 12, 1), ("avg_pool", "minentropy_pool")),     # T = 5 > 4: generic warp_pool at C = 19; a single column
    ((4, 2, 2, 31, 64), ("avg_pool", "minentropy_pool")),     # C = 2, several blocks per group
    ((32, 1, 19, 182, 182), ("avg_pool",)),        # warp_pool_avg<19,1>, cap (4096 + N - 1) / N = 128 blocks = 32768 items < 33124
    ((32, 2, 3, 182, 182), ("minentropy_pool",)),  # generic warp_pool, the same cap: second pass of its loop
]
POOL_PARAMS = [(s, m) for s, ms in POOL_CASES for m in ms]


@pytest.mark.parametrize("shape,mode", POOL_PARAMS, ids=["{}_{}".format("x".join(map(str, s)), m[:3]) for s, m in POOL_PARAMS])
def test_warp_pool_against_fp64(shape, mode):
    from dasac_hip import ops
    N, Tn, C, H, W = shape
    tol = 0.1
    probs, theta, theta_inv = _pool_inputs(shape)
    pooled, mask, aligned = ops.warp_pool(probs.cuda(), theta.cuda(), theta_inv.cuda(), Tn, mode, tol)
    pooled2, mask2, none = ops.warp_pool(probs.cuda(), theta.cuda(), theta_inv.cuda(), Tn, mode, tol, want_aligned=False)
    assert none is None and torch.equal(pooled2, pooled) and torch.equal(mask2, mask)    # aligned == NULL: the same bits
    a64, p64, m64, Z, vs, ent = _pool_reference(probs, theta, theta_inv, Tn, mode, tol, torch.float64)
    a32, p32, _, _, _, _ = _pool_reference(probs, theta, theta_inv, Tn, mode, tol, torch.float32)
    ex = _excluded(mode, tol, Z, vs, ent)
    share = float(ex.float().mean())
    assert share <= MAX_EXCLUDED, (shape, mode, share)
    mask = mask.cpu()
    assert mask.shape == (N, 1, H, W) and bool(((mask == 0) | (mask == 1)).all())
    assert torch.equal(mask.bool() & ~ex, m64 & ~ex)
    keep = (~ex).expand_as(p64)
    print("warp_pool {} {}: excluded share {:.3g}".format(shape, mode, share))
    _report("warp_pool", (shape, mode), {"aligned": _ratio(aligned, a64, a32),
                                         "pooled": _ratio(pooled.cpu() * keep, p64 * keep, p32 * keep)})


# ---- warp back ---------------------------------------------------------------------------------------------------------------
def test_warp_back_second_pass_of_the_capped_grid():
    """(B, C, H, W) = (64, 2, 257, 257), two views per group: items = ceil(257 / 4) * 257 = 16705 columns of four rows against a
    cap of (4096 + B - 1) / B = 64 blocks = 16384 -- the second trip of warp_back's loop; the last row group has one row
    (warp_back_rows<1>).  Small shapes: test_gpu_head.py::test_warp_back_against_the_oracle."""
    from dasac_hip import ops
    B, C, H, W, Tn = 64, 2, 257, 257, 2
    g = torch.Generator().manual_seed(B + C + H + W)
    pooled = torch.rand(B // Tn, C, H, W, generator=g)
    mask = (torch.rand(B // Tn, 1, H, W, generator=g) > 0.3).float()
    theta = _random_thetas(B, g)
    got = ops.warp_back(pooled.cuda(), mask.cuda(), theta.cuda(), Tn)

    def ref(dtype):
        return _warp(pooled.to(dtype).repeat_interleave(Tn, 0), theta) * _warp(mask.to(dtype).repeat_interleave(Tn, 0), theta)
    _report("warp_back", (B, C, H, W), {"refined": _ratio(got, ref(torch.float64), ref(torch.float32))})
