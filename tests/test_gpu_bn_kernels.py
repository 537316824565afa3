"""Train-mode BatchNorm kernels (batchnorm.hip: bn_stats, bn_sums_finish, bn_tile_stats_reduce, bn_train_finalize, bn_apply,
bn_apply_tiles, bn_bwd_reduce, bn_bwd_apply, bn_bwd_apply_partials, bn_bwd_params) on their own, against float64 ATen
`F.batch_norm(training=True)` + autograd on the CPU.

Shapes sit where the kernels change behaviour: planes of fewer than 4 elements and planes that are not 16-byte aligned (the
vector loads have a scalar tail), one element past a reduction chunk (kBnChunk = 4096) and past an apply chunk (kBnBig = 16384),
several chunks per plane with a ragged last one, and N*C >= 65536 planes, where ops.py falls back from the one-rank fused kernels
to bn_stats / bn_bwd_reduce, whose grids also carry the plane index in gridDim.y.  Inputs have a mean of 10 standard deviations
(mean^2 / var = 100), so a statistics pass that lost precision would show.

Per-element bounds are relative to the magnitude of the terms each output is made of (not to the tensor's max).  Worst measured
ratio got/bound on the MI355X: y 0.05 and dz 0.34 (bound 4e-6 of the terms), d gamma / d beta 0.06 (bound 1e-6); var of the
stand-alone statistics pass 2.3e-7 relative (bound 1e-6 on invstd).  The fallback launches with gridDim.y = N*C = 65536 and
81920 run and stay within these bounds: the 65536-plane refusal of the fused one-rank kernels is a choice, not a HIP limit."""
import pytest
import torch
import torch.nn as nn

from conftest import rel_err

pytestmark = pytest.mark.gpu
EPS = 1e-5
TAU = 4e-6          # y, dz: |got - ref| <= TAU * (sum of the magnitudes of the terms)
TAU_P = 1e-6        # d gamma, d beta: relative to the channel's sums of the magnitudes of their terms


def _inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    N, C = shape[0], shape[1]
    sigma = torch.rand(C, generator=g) * 2 + 0.5
    z = torch.randn(shape, generator=g) * sigma.view(1, C, 1, 1) + 10 * sigma.view(1, C, 1, 1)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g)
    res = torch.randn(shape, generator=g)
    g_out = torch.randn(shape, generator=g)
    rm = torch.randn(C, generator=g)
    rv = torch.rand(C, generator=g) + 0.5
    return z, gamma, beta, res, g_out, rm, rv


def _bn(C, gamma, beta, rm, rv, momentum, track, nbt, device, dtype=torch.float32):
    bn = nn.BatchNorm2d(C, eps=EPS, momentum=momentum, track_running_stats=track).to(device=device, dtype=dtype)
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
        if track:
            bn.running_mean.copy_(rm)
            bn.running_var.copy_(rv)
            bn.num_batches_tracked.fill_(nbt)
    return bn


def _reference(z, res, relu, g_out, bn_ref):
    """float64 ATen: y = relu?(bn_ref(z) (+res)) with the module in train mode (batch statistics; running statistics and
    num_batches_tracked move as nn.BatchNorm2d moves them, momentum None = cumulative average); dz, dgamma, dbeta for the
    BN-output gradient dy = g_out * relu mask (what the engine hands bn_train_backward).  The mask is the reference's, so the
    kernel and the reference see the same dy."""
    zd = z.double().requires_grad_(True)
    bn_ref.train()
    out = bn_ref(zd)
    y = out.detach() + (res.double() if res is not None else 0)
    mask = (y > 0) if relu else torch.ones_like(y, dtype=torch.bool)
    if relu:
        y = y.clamp_min(0)
    dy = g_out.double() * mask
    out.backward(dy)
    mean = zd.detach().mean((0, 2, 3))
    var = zd.detach().var((0, 2, 3), unbiased=False)
    return y, dy.float(), zd.grad, bn_ref.weight.grad, bn_ref.bias.grad, mean, var


def _check_y(y, y_ref, z, gamma, beta, res, inv_ref, what):
    C = z.shape[1]
    term = (z.double().abs() * (gamma.double() * inv_ref).abs().view(1, C, 1, 1) + beta.double().abs().view(1, C, 1, 1)
            + (res.double().abs() if res is not None else 0))
    ratio = float(((y.double().cpu() - y_ref).abs() / (TAU * term + 1e-30)).max())
    assert ratio <= 1.0, (what, "y", ratio)
    return ratio


def _check_dz(dz, dz_ref, dy, z, gamma, mean_ref, inv_ref, what):
    C = z.shape[1]
    dyd = dy.double()
    n = z.numel() // C
    xh = (z.double() - mean_ref.view(1, C, 1, 1)) * inv_ref.view(1, C, 1, 1)
    a = dyd.sum((0, 2, 3)).abs() / n
    b = (dyd * xh).sum((0, 2, 3)).abs() / n
    # xhat is formed in fp32 from z and mean, each ~10 std: its rounding error scales with (|z| + |mean|) * invstd, not |xhat|
    xh_terms = (z.double().abs() + mean_ref.abs().view(1, C, 1, 1)) * inv_ref.view(1, C, 1, 1)
    term = (gamma.double() * inv_ref).abs().view(1, C, 1, 1) * (dyd.abs() + a.view(1, C, 1, 1) + xh_terms * b.view(1, C, 1, 1))
    ratio = float(((dz.double().cpu() - dz_ref).abs() / (TAU * term + 1e-30)).max())
    assert ratio <= 1.0, (what, "dz", ratio)
    return ratio


def _check_params(dg, db, dg_ref, db_ref, dy, z, mean_ref, inv_ref, what):
    C = z.shape[1]
    dyd = dy.double()
    xh_terms = (z.double().abs() + mean_ref.abs().view(1, C, 1, 1)) * inv_ref.view(1, C, 1, 1)     # as in _check_dz
    sg, sb = (dyd.abs() * xh_terms).sum((0, 2, 3)), dyd.abs().sum((0, 2, 3))
    # (a channel the ReLU closed entirely has dy = 0: both gradients must then be exactly 0)
    rg = float(((dg.double().cpu() - dg_ref).abs() / (TAU_P * sg + 1e-30)).max())
    rb = float(((db.double().cpu() - db_ref).abs() / (TAU_P * sb + 1e-30)).max())
    assert rg <= 1.0 and rb <= 1.0, (what, "dgamma / dbeta", rg, rb)
    return max(rg, rb)


# (N, C, H, W): plane sizes at the load / chunk edges; N*C = 65536 and beyond take the multi-launch fallback of ops.py
SHAPES = [
    (2, 64, 1, 1),          # HW = 1
    (1, 3, 1, 3),           # HW = 3 < one 16-byte load
    (3, 5, 7, 9),           # HW = 63: every plane but the first starts off 16-byte alignment
    (2, 16, 64, 65),        # HW = 4160: 64 elements past one reduction chunk
    (1, 8, 129, 129),       # HW = 16641: past an apply chunk, planes misaligned
    (2, 4, 193, 193),       # HW = 37249: 10 reduction chunks, 3 apply chunks, ragged last ones
    (32, 2048, 2, 2),       # N*C = 65536 planes: the fallback (gridDim.y = 65536)
    (40, 2048, 1, 3),       # N*C = 81920 planes, HW = 3
]
# variants: (res, relu, momentum, update_running, track_running_stats) -- every value appears on several shapes
VARIANTS = [
    (False, False, 0.1, True, True),
    (True, True, None, True, True),
    (True, False, 0.1, False, True),
    (False, True, None, False, True),
    (False, False, None, True, False),
    (True, True, 0.1, True, True),
    (False, True, None, True, True),
    (True, False, 0.1, True, True),
]
CASES = [(s, v) for s, v in zip(SHAPES, VARIANTS)] + [((3, 5, 7, 9), v) for v in VARIANTS[1:5]]


def _case_id(c):
    (shape, (res, relu, mom, upd, track)) = c
    return "{}{}{}_m{}{}{}".format("x".join(map(str, shape)), "_res" if res else "", "_relu" if relu else "", mom,
                                   "" if upd else "_noupd", "" if track else "_notrack")


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_bn_train_forward_backward_against_fp64(case):
    from dasac_hip import ops
    shape, (with_res, relu, momentum, upd, track) = case
    N, C, H, W = shape
    z, gamma, beta, res, g_out, rm, rv = _inputs(shape, seed=sum(shape))
    res = res if with_res else None
    nbt0 = 3
    bn = _bn(C, gamma, beta, rm, rv, momentum, track, nbt0, "cuda")
    bn_ref = _bn(C, gamma.double(), beta.double(), rm.double(), rv.double(), momentum, track, nbt0, "cpu", torch.float64)
    y_ref, dy, dz_ref, dg_ref, db_ref, mean_ref, var_ref = _reference(z, res, relu, g_out, bn_ref)
    inv_ref = (var_ref + EPS).rsqrt()

    zc = z.cuda()
    y, stats = ops.bn_train_forward(zc, bn, None if res is None else res.cuda(), relu, update_running=upd)
    mean, invstd, count, count_dev = stats
    assert count == N * H * W and count_dev is None
    assert float(((mean.double().cpu() - mean_ref).abs() / mean_ref.abs()).max()) < 1e-6
    assert float(((invstd.double().cpu() - inv_ref).abs() / inv_ref).max()) < 1e-6        # double accumulation: var to ~1e-7
    r_y = _check_y(y, y_ref, z, gamma, beta, res, inv_ref, shape)

    if track and upd:                                    # ATen's float64 bookkeeping of the same step
        assert rel_err(bn.running_mean, bn_ref.running_mean) < 1e-6 and rel_err(bn.running_var, bn_ref.running_var) < 1e-6
        assert int(bn.num_batches_tracked) == int(bn_ref.num_batches_tracked) == nbt0 + 1
    elif track:                                          # update_running=False: nothing moves
        assert torch.equal(bn.running_mean.cpu(), rm) and torch.equal(bn.running_var.cpu(), rv)
        assert int(bn.num_batches_tracked) == nbt0
    else:
        assert bn.running_mean is None and bn.num_batches_tracked is None

    dz, dg, db = ops.bn_train_backward(dy.cuda(), zc, stats, bn.weight.detach())
    r_dz = _check_dz(dz, dz_ref, dy, z, gamma, mean_ref, inv_ref, shape)
    r_p = _check_params(dg, db, dg_ref, db_ref, dy, z, mean_ref, inv_ref, shape)
    var_err = float((((invstd.double().cpu() ** -2 - EPS) - var_ref).abs() / var_ref).max())
    print("{}: y {:.3g}, dz {:.3g}, dgamma/dbeta {:.3g} of the bound; var {:.3g}".format(shape, r_y, r_dz, r_p, var_err))


def _conv_with_tile_stats(shape, cx, seed):
    """z = 1x1 conv + per-channel bias (mean ~10 std) through conv_gemm(stats=...): z and the per-tile statistics it left."""
    from dasac_hip import ops
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    spec = ops.ConvSpec(cx, C, [(1, 1, 1, 0)], 1)
    assert ops.stats_ok(C, cx)
    x = torch.randn(N, cx, H, W, generator=g).cuda()
    w = (torch.randn(C, cx, 1, 1, generator=g) / cx ** 0.5).cuda()
    bias = (10 + torch.rand(C, generator=g)).cuda()
    order = ops.gemm_order(spec, False)
    table, packed = ops.conv_table(spec, H, W, False, x.device, order), ops.conv_pack(spec, [w], False, None, order=order)
    z = torch.empty(shape, device="cuda")
    ts = ops.tile_stats_buffer(N, C, H, W, x.device)
    ops.conv_gemm(x, packed, table, z, (H, W), 1, C, spec.K, 1, bias, stats=ts)
    return z, ts


@pytest.mark.parametrize("shape", [
    (2, 128, 33, 41),       # one rank, N*C < 65536: bn_apply_tiles (one launch per layer), HW = 1353 (misaligned planes)
    (1, 128, 129, 129),     # bn_apply_tiles over two apply chunks (16641 elements)
    (32, 2048, 2, 2),       # N*C = 65536: bn_tile_stats_reduce + bn_train_finalize + bn_apply
])
def test_bn_train_forward_from_tile_statistics(shape):
    """The statistics a conv's epilogue left per tile: fp32 per-tile sums, so var keeps the bound test_gpu_bn_train.py documents
    (2e-3 on var / 1e-3 on invstd at mean^2/var = 1e4; here mean^2/var is ~100); y, running stats and the backward follow."""
    from dasac_hip import ops
    N, C, H, W = shape
    z, ts = _conv_with_tile_stats(shape, 64, seed=C + H)
    g = torch.Generator().manual_seed(7)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    res, g_out = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    bn = _bn(C, gamma, beta, torch.zeros(C), torch.ones(C), 0.1, True, 0, "cuda")
    bn_ref = _bn(C, gamma.double(), beta.double(), torch.zeros(C).double(), torch.ones(C).double(), 0.1, True, 0, "cpu", torch.float64)
    zh = z.cpu()
    y_ref, dy, dz_ref, dg_ref, db_ref, mean_ref, var_ref = _reference(zh, res, True, g_out, bn_ref)
    inv_ref = (var_ref + EPS).rsqrt()
    y, stats = ops.bn_train_forward(z, bn, res.cuda(), True, tile_stats=ts)
    mean, invstd = stats[0], stats[1]
    assert float(((mean.double().cpu() - mean_ref).abs() / mean_ref.abs()).max()) < 1e-6
    assert float(((invstd.double().cpu() - inv_ref).abs() / inv_ref).max()) < 1e-3
    assert rel_err(y, y_ref) < 1e-3
    assert rel_err(bn.running_mean, bn_ref.running_mean) < 1e-6 and rel_err(bn.running_var, bn_ref.running_var) < 2e-3
    assert int(bn.num_batches_tracked) == 1
    dz, dg, db = ops.bn_train_backward(dy.cuda(), z, stats, bn.weight.detach())
    assert rel_err(dz, dz_ref) < 1e-3 and rel_err(dg, dg_ref) < 1e-3 and rel_err(db, db_ref) < 1e-5


@pytest.mark.parametrize("source", ["stats", "tiles"])
@pytest.mark.parametrize("relu", [False, True])
def test_syncbn_kernel_sequence_on_two_halves_equals_bn_over_the_whole_batch(source, relu):
    """The SyncBN sequence ops.py runs with several ranks, on one process: each "rank" (half of the batch) reduces its own sums
    (dasac_bn_stats, or dasac_bn_tile_stats_reduce of its conv's tile statistics), the halves' sums are added in a device tensor
    (what the all-reduce does), dasac_bn_train_finalize runs with count = 0 and the all-reduced DEVICE count, dasac_bn_apply
    normalises the half; backward: dasac_bn_bwd_reduce (writing this half's own d gamma / d beta), the sums added,
    dasac_bn_bwd_apply with the device count.  Every half must equal float64 BN over the whole batch."""
    from dasac_hip import lib as L
    from dasac_hip import ops
    lib = L.load()
    shape = (4, 128, 17, 23)                       # HW = 391: planes misaligned for the 16-byte loads
    N, C, H, W = shape
    half = N // 2
    if source == "tiles":
        parts = [_conv_with_tile_stats((half, C, H, W), 64, seed=11 + r) for r in range(2)]
        zs, tss = [p[0] for p in parts], [p[1] for p in parts]
    else:
        z_all = _inputs(shape, seed=5)[0]
        zs, tss = [z_all[:half].cuda().contiguous(), z_all[half:].cuda().contiguous()], [None, None]
    g = torch.Generator().manual_seed(3)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    rm, rv = torch.randn(C, generator=g), torch.rand(C, generator=g) + 0.5
    res, g_out = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    z = torch.cat([t.cpu() for t in zs])
    bn_ref = _bn(C, gamma.double(), beta.double(), rm.double(), rv.double(), 0.1, True, 0, "cpu", torch.float64)
    y_ref, dy, dz_ref, dg_ref, db_ref, mean_ref, var_ref = _reference(z, res, relu, g_out, bn_ref)
    inv_ref = (var_ref + EPS).rsqrt()
    HW = H * W
    s = L.stream_ptr()
    ws_bytes = lib.dasac_bn_stats_workspace(half, C, HW)

    sums = []
    for r in range(2):
        t = torch.empty(2 * C, dtype=torch.float64, device="cuda")
        if source == "tiles":
            L.check(lib.dasac_bn_tile_stats_reduce(tss[r].data_ptr(), tss[r].shape[0], C, tss[r].shape[2], t.data_ptr(), s),
                    "dasac_bn_tile_stats_reduce")
        else:
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
            L.check(lib.dasac_bn_stats(zs[r].data_ptr(), half, C, HW, t.data_ptr(), ws.data_ptr(), ws_bytes, s), "dasac_bn_stats")
        sums.append(t)
    total = sums[0] + sums[1]                                     # the all-reduce of the raw sums ...
    count_dev = torch.tensor([float(N * HW)], dtype=torch.float64, device="cuda")   # ... and of the element count
    grad_sums, own = [], []
    for r in range(2):
        sl = slice(r * half, (r + 1) * half)
        gc, bc = gamma.cuda(), beta.cuda()
        rmc, rvc = rm.cuda(), rv.cuda()
        nbt = torch.zeros((), dtype=torch.int64, device="cuda")
        scale, shift, mean, invstd = (torch.empty(C, device="cuda") for _ in range(4))
        L.check(lib.dasac_bn_train_finalize(total.data_ptr(), 0.0, count_dev.data_ptr(), gc.data_ptr(), bc.data_ptr(), rmc.data_ptr(),
                                            rvc.data_ptr(), nbt.data_ptr(), 0.1, EPS, C, scale.data_ptr(), shift.data_ptr(),
                                            mean.data_ptr(), invstd.data_ptr(), s), "dasac_bn_train_finalize")
        rres = res[sl].cuda().contiguous()
        y = torch.empty_like(zs[r])
        L.check(lib.dasac_bn_apply(zs[r].data_ptr(), scale.data_ptr(), shift.data_ptr(), rres.data_ptr(), int(relu), half, C, HW,
                                   y.data_ptr(), s), "dasac_bn_apply")
        tol = 1e-3 if source == "tiles" else 1e-6
        assert float(((invstd.double().cpu() - inv_ref).abs() / inv_ref).max()) < tol, r
        assert float(((mean.double().cpu() - mean_ref).abs() / mean_ref.abs()).max()) < 1e-6, r
        if source == "stats":
            _check_y(y, y_ref[sl], z[sl], gamma, beta, res[sl], inv_ref, ("half", r))
        else:
            assert rel_err(y, y_ref[sl]) < 1e-3, r
        assert rel_err(rmc, bn_ref.running_mean) < 1e-6 and rel_err(rvc, bn_ref.running_var) < (2e-3 if source == "tiles" else 1e-6)
        assert int(nbt) == 1
        # backward, this half
        dyr = dy[sl].cuda().contiguous()
        gs = torch.empty(2 * C, dtype=torch.float64, device="cuda")
        dg, db = torch.full((C,), float("nan"), device="cuda"), torch.full((C,), float("nan"), device="cuda")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        L.check(lib.dasac_bn_bwd_reduce(dyr.data_ptr(), zs[r].data_ptr(), mean.data_ptr(), invstd.data_ptr(), half, C, HW, gs.data_ptr(),
                                        dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws_bytes, s), "dasac_bn_bwd_reduce")
        grad_sums.append(gs)
        own.append((dyr, mean, invstd, gc, dg, db))
    gtotal = grad_sums[0] + grad_sums[1]
    for r in range(2):
        sl = slice(r * half, (r + 1) * half)
        dyr, mean, invstd, gc, dg, db = own[r]
        dz = torch.empty_like(zs[r])
        L.check(lib.dasac_bn_bwd_apply(dyr.data_ptr(), zs[r].data_ptr(), mean.data_ptr(), invstd.data_ptr(), gc.data_ptr(),
                                       gtotal.data_ptr(), 0.0, count_dev.data_ptr(), half, C, HW, dz.data_ptr(), None, None, s),
                "dasac_bn_bwd_apply")
        if source == "stats":
            _check_dz(dz, dz_ref[sl], dy[sl], z[sl], gamma, mean_ref, inv_ref, ("half", r))
        else:
            assert rel_err(dz, dz_ref[sl]) < 1e-3, r
        # d gamma / d beta of a rank are its LOCAL sums (DDP averages them afterwards): sum over this half of dy*xhat, dy
        xh = (z[sl].double() - mean_ref.view(1, C, 1, 1)) * inv_ref.view(1, C, 1, 1)
        dg_half, db_half = (dy[sl].double() * xh).sum((0, 2, 3)), dy[sl].double().sum((0, 2, 3))
        if source == "stats":
            _check_params(dg, db, dg_half, db_half, dy[sl], z[sl], mean_ref, inv_ref, ("half", r))
        else:
            assert rel_err(dg, dg_half) < 1e-3 and rel_err(db, db_half) < 1e-5, r
    # and together they are the whole batch's
    assert rel_err(own[0][4] + own[1][4], dg_ref) < (1e-3 if source == "tiles" else 1e-5)
    assert rel_err(own[0][5] + own[1][5], db_ref) < 1e-5
