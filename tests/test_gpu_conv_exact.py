"""Every conv GEMM path, bit for bit, on operands whose products and partial sums are all exactly representable in fp32
(conv_lattice.py): one block per tile, stream-K, the split-K tail, pixel ranges, the batched launch, the epilogues and their
statistics, the pixel-split weight gradient with its dot rows and dasac_bn_param_grads, Winograd F(2x2,3x3), the split-bf16
kernels and the tap-expanded ASPP convolution.  Every summation order must give the integer reference's bits, so every
comparison is torch.equal: a dropped, duplicated or misaddressed product fails however small it is.  Each test asserts the
exactness precondition (computed from the reference operands alone) before it looks at a kernel's output;
test_conv_exact_cpu.py checks the same claims for the same cases without a GPU."""
import pytest
import torch

import conv_lattice as cl
from conv_lattice import BATCHED, PIX_CASES, SCHEDULE_CASE, TAIL_CASE, X3_BATCH, expanded_operands, x3_exact_ok

pytestmark = pytest.mark.gpu
NAN = float("nan")

_LISTS = cl.case_lists()
CONV_CASES, DOT_CASES, STATS, WINO_SHAPES, X3_CASES, EXPANDED = (_LISTS[k] for k in ("conv", "dot", "stats", "winograd", "x3", "expanded"))


def _dev(t):
    return None if t is None else t.cuda()


def _eq(got, want64):
    """Bit-for-bit (as values: -0 == +0) equality with the float64 reference, which must itself be an fp32 lattice point."""
    want = cl.f32(want64)
    got = got.cpu()
    return got.shape == want.shape and torch.equal(got, want)


def _bc(v):
    return v.double().view(1, -1, 1, 1)


def _flags_clean(ops):
    lib = ops.L.load()
    ws = ops.L.workspace(lib.dasac_conv_gemm_workspace(), torch.device("cuda", torch.cuda.current_device()), owner="conv_gemm")
    torch.cuda.synchronize()
    flags = ws[ws.numel() - 4 * 2049:].view(torch.int32)
    return int(flags.abs().sum()) == 0


# ----------------------------------------------------------------------------------------------
# forward, data gradient, weight gradient
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_forward_dgrad_wgrad_are_exact(case, scaled):
    from dasac_hip import ops
    name, cin, cout, br, stride, (N, H, W) = case
    spec = ops.ConvSpec(cin, cout, br, stride)
    o = cl.plain_operands(cin, cout, br, stride, (N, H, W))
    x, ws, dz, shift, res_out, res_in, mask_in = (o[k] for k in ("x", "ws", "dz", "shift", "res_out", "res_in", "mask_in"))
    scale = o["scale"] if scaled else None
    assert cl.exact_ok(x, ws, br, stride, dz, scale, shift, res_out, res_in)
    xd, wd, dzd, sd = x.cuda(), [w.cuda() for w in ws], dz.cuda(), _dev(scale)

    fwd = cl.conv_fwd(x, ws, br, stride, scale)
    assert _eq(ops.conv_forward(spec, xd, wd, scale=sd), fwd)
    want = torch.relu(fwd + _bc(shift) + res_out.double())
    assert 0.1 < float((want > 0).double().mean()) < 0.9
    assert _eq(ops.conv_forward(spec, xd, wd, sd, shift.cuda(), res_out.cuda(), relu=True), want)

    sums = torch.full((cout,), NAN, device="cuda")
    gw = ops.conv_wgrad(spec, dzd, xd, wd, scale=sd, sum_dz=sums, outs=[torch.full_like(w, NAN) for w in wd])   # every element is written
    for a, b in zip(gw, cl.conv_dw(dz, x, ws, br, stride, scale)):
        assert _eq(a, b)
    assert _eq(sums, dz.double().sum((0, 2, 3)))

    if stride == 1 or spec.taps == 1:
        dxr = cl.conv_dx(dz, ws, br, stride, (H, W), scale)
        assert _eq(ops.conv_dgrad(spec, dzd, wd, (H, W), scale=sd), dxr)
        masked = torch.where(mask_in > 0, dxr + res_in.double(), torch.zeros_like(dxr))
        assert 0.1 < float((masked != 0).double().mean()) < 0.9
        if stride == 1:
            assert _eq(ops.conv_dgrad(spec, dzd, wd, (H, W), scale=sd, res=res_in.cuda(), mask=mask_in.cuda()), masked)
        else:
            # strided 1x1: the GEMM scatters onto the stride lattice and accumulates IN PLACE; off-lattice positions keep `res`
            acc = res_in.cuda()
            dx = ops.conv_dgrad(spec, dzd, wd, (H, W), scale=sd, res=acc)
            assert dx.data_ptr() == acc.data_ptr() and _eq(dx, dxr + res_in.double())
            off = torch.ones(H, W, dtype=torch.bool)
            off[::stride, ::stride] = False
            assert torch.equal(dx.cpu()[:, :, off], res_in[:, :, off])
            assert _eq(ops.conv_dgrad(spec, dzd, wd, (H, W), scale=sd, res=res_in.cuda(), mask=mask_in.cuda()), masked)


@pytest.mark.parametrize("case", DOT_CASES, ids=[c[0] for c in DOT_CASES])
def test_wgrad_dot_rows_and_bn_param_grads_are_exact(case):
    """conv_wgrad(dot=...) leaves one partial row per block of 64 input channels: each row equals its own block's sum of W * G,
    and dasac_bn_param_grads on those rows and sum_dz (integer mean and bias, power-of-two invstd and scale) is exact."""
    from dasac_hip import ops
    name, cin, cout, br, stride, (N, H, W) = case
    spec = ops.ConvSpec(cin, cout, br, stride)
    o = cl.plain_operands(cin, cout, br, stride, (N, H, W))
    x, w, dz, scale = o["x"], o["ws"][0], o["dz"], o["scale"]
    g = cl.gen(cin + cout)
    mean, bias, invstd = cl.ints((cout,), 8, g), cl.ints((cout,), 8, g), cl.pow2(cout, g)
    assert cl.exact_ok(x, [w], br, stride, dz, scale, parts=("dw",)) and cl.dot_exact_ok(w, dz, x, br, stride)
    (ga,) = cl.conv_dw(dz.abs(), x.abs(), [w.abs()], br, stride)
    assert cl.bn_param_grads_exact_ok(cl.dot_rows_ref(w.abs(), ga), dz.abs().sum((0, 2, 3)), mean, bias)

    rows = ops.dot_rows(spec)
    assert rows == 4
    dot = torch.full((rows, cout), NAN, device="cuda")
    sums = torch.full((cout,), NAN, device="cuda")
    (gw,) = ops.conv_wgrad(spec, dz.cuda(), x.cuda(), [w.cuda()], scale=scale.cuda(), dot=dot, sum_dz=sums, outs=[torch.full_like(w.cuda(), NAN)])
    (gu,) = cl.conv_dw(dz, x, [w], br, stride)                                  # unscaled G
    assert _eq(gw, gu * scale.double().view(-1, 1, 1, 1))
    want_rows, want_sums = cl.dot_rows_ref(w, gu), dz.double().sum((0, 2, 3))
    assert _eq(dot, want_rows) and _eq(sums, want_sums)
    assert all(bool(want_rows[r].abs().sum() > 0) for r in range(rows))

    dg, db, dcb = ops.bn_param_grads(dot, sums, mean.cuda(), invstd.cuda(), scale.cuda(), bias.cuda(), True, True, True)
    rg, rb, rcb = cl.bn_param_grads_ref(want_rows, want_sums, mean, invstd, scale, bias)
    assert _eq(dg, rg) and _eq(db, rb) and _eq(dcb, rcb)
    assert bool((rg != 0).any()) and bool((rcb != 0).any())


# ----------------------------------------------------------------------------------------------
# schedules and epilogues
# ----------------------------------------------------------------------------------------------
def _gemm_case(case):
    """Operands on the device, the packed weights / table of the forward GEMM and the float64 convolution of one case."""
    from dasac_hip import ops
    name, cin, cout, br, stride, shape = case
    spec = ops.ConvSpec(cin, cout, br, stride)
    o = cl.plain_operands(cin, cout, br, stride, shape)
    order = ops.gemm_order(spec, False)
    dev = torch.device("cuda", 0)
    table = ops.conv_table(spec, shape[1], shape[2], False, dev, order)
    packed = ops.conv_pack(spec, [w.cuda() for w in o["ws"]], False, None, order=order)
    return spec, o, table, packed


def _epilogue(name, o, ref, shape, g):
    """One of the four epilogues the network uses: (shift, res, fp32 mask, relu, record bits, mask words, expected float64 output)."""
    shift, res, mask = o["shift"], o["res_out"], o["mask_out"]
    zero = torch.zeros_like(ref)
    if name == "none":
        return None, None, None, False, False, None, ref
    if name == "shift_res_relu_bits":
        return shift, res, None, True, True, None, torch.relu(ref + _bc(shift) + res.double())
    if name == "res_mask_bits":
        words = torch.randint(-2 ** 31, 2 ** 31 - 1, (shape[1] * ((shape[0] * shape[2] * shape[3] + 31) // 32),), generator=g,
                              dtype=torch.int64).to(torch.int32)
        return None, res, None, False, False, words, torch.where(cl.unpack_bits(words, shape), ref + res.double(), zero)
    assert name == "res_mask_fp32"
    return None, res, mask, False, False, None, torch.where(mask > 0, ref + res.double(), zero)


def _run_epilogue(ops, spec, o, table, packed, shape, epi, schedule):
    shift, res, mask, relu, want_bits, words, want = epi
    N, M, OH, OW = shape
    out = torch.full(shape, NAN, device="cuda")
    bits = None
    if want_bits:
        bits = ops.ReluBits(N, M, OH, OW, out.device)
        bits.words.fill_(0x55555555)
    if words is not None:
        mask = ops.ReluBits(N, M, OH, OW, out.device)
        mask.words.copy_(words)
    else:
        mask = _dev(mask)
    ops.conv_gemm(o["x"].cuda(), packed, table, out, (OH, OW), spec.stride, M, spec.K, 1, _dev(shift), _dev(res), mask, relu,
                  bits_out=bits, schedule=schedule)
    assert _eq(out, want), schedule
    if want_bits:
        assert torch.equal(cl.unpack_bits(bits.words, shape).cpu(), want > 0), schedule


@pytest.mark.parametrize("epi", ["none", "shift_res_relu_bits", "res_mask_bits", "res_mask_fp32"])
def test_tile_per_block_and_stream_k_equal_the_reference(epi):
    from dasac_hip import ops
    lib = ops.L.load()
    name, cin, cout, br, stride, (N, H, W) = SCHEDULE_CASE
    spec, o, table, packed = _gemm_case(SCHEDULE_CASE)
    assert cl.exact_ok(o["x"], o["ws"], br, stride, None, None, o["shift"], o["res_out"], parts=("fwd",))
    assert lib.dasac_conv_gemm_schedule(N, H, W, cout, spec.K) == 1 and ops.bits_ok(cout, cin)
    shape = (N, cout, H, W)
    ref = cl.conv_fwd(o["x"], o["ws"], br, stride)
    e = _epilogue(epi, o, ref, shape, cl.gen(11))
    ops.PROFILE.start()
    try:
        for schedule in (1, 2):
            _run_epilogue(ops, spec, o, table, packed, shape, e, schedule)
    finally:
        spans = ops.PROFILE.stop()
    assert {k: v["launches"] for k, v in spans.items()} == {"conv_gemm<tile-per-block>": 1, "conv_gemm<stream-K>": 1}
    assert _flags_clean(ops)


def test_split_k_tail_equals_the_reference():
    """The smallest shape whose launch is whole rounds one block per tile + a split-K tail: the library's choice (with the
    workspace), the plain one-block-per-tile launch and the reference are all equal, with and without an epilogue."""
    from dasac_hip import ops
    lib = ops.L.load()
    name, cin, cout, br, stride, (N, H, W) = TAIL_CASE
    spec, o, table, packed = _gemm_case(TAIL_CASE)
    split = lib.dasac_conv_gemm_tail_split(N, H, W, cout, spec.K)
    print("tail_split({}) = {}".format(TAIL_CASE[1:], split))
    assert split > 0                                      # (8 K-ranges of 9 steps per tail tile on an MI355X with no reserved CUs)
    # (fp32 on the CPU: exact on the lattice -- test_conv_exact_cpu.py holds it against float64 for this case -- and a sum of
    # non-negative terms that reached 2^24 cannot round back below it)
    assert cl.exact_ok(o["x"], o["ws"], br, stride, None, None, o["shift"], o["res_out"], dtype=torch.float32, parts=("fwd",))
    shape = (N, cout, H, W)
    ref = cl.conv_fwd(o["x"], o["ws"], br, stride, None, torch.float32).double()
    ops.PROFILE.start()
    try:
        for epi in ("none", "shift_res_relu_bits"):
            e = _epilogue(epi, o, ref, shape, cl.gen(12))
            for schedule in (None, 1):
                _run_epilogue(ops, spec, o, table, packed, shape, e, schedule)
    finally:
        spans = ops.PROFILE.stop()
    assert {k: v["launches"] for k, v in spans.items()} == {"conv_gemm<tile+tail>": 2, "conv_gemm<tile-per-block>": 2}
    assert _flags_clean(ops)


@pytest.mark.parametrize("case", STATS, ids=[c[0] for c in STATS])
def test_epilogue_statistics_are_the_integer_tile_sums(case):
    from dasac_hip import ops
    name, cin, cout, br, (N, H, W) = case[:5]
    spec = ops.ConvSpec(cin, cout, [br], 1)
    o = cl.stats_operands(cin, cout, br, (N, H, W))
    x, w, bias = o["x"], o["ws"][0], o["bias"]
    ref = cl.conv_fwd(x, [w], [br], 1) + _bc(bias)
    assert cl.exact_ok(x, [w], [br], 1, shift=bias, parts=("fwd",)) and cl.stats_exact_ok(ref)
    assert ops.stats_ok(cout, cin)
    s, q = cl.tile_sums(ref)
    assert bool((q > 0).all())
    order = ops.gemm_order(spec, False)
    xd = x.cuda()
    table, packed = ops.conv_table(spec, H, W, False, xd.device, order), ops.conv_pack(spec, [w.cuda()], False, None, order=order)
    # schedule 2 runs the persistent stream-K kernel only when the (tile, K-step) space gives each of its 768 workers a step; below
    # that the library runs one block per tile whatever is asked (tiles_1x1: 104 steps, ragged_m200: 432): streamk_3x3 (3168 steps)
    # is the case that checks the statistics slot of a tile cut among several workers
    steps = ((cout + 127) // 128) * ((N * H * W + 127) // 128) * (spec.K // 16)
    assert (steps >= 768) == (name == "streamk_3x3")
    for schedule in (1, 2):
        out = torch.full((N, cout, H, W), NAN, device="cuda")
        ts = ops.tile_stats_buffer(N, cout, H, W, xd.device).fill_(NAN)
        ops.conv_gemm(xd, packed, table, out, (H, W), 1, cout, spec.K, 1, bias.cuda(), stats=ts, schedule=schedule)
        assert _eq(out, ref), schedule
        assert ts.shape[0] == s.shape[0]
        assert _eq(ts[:, 0, :cout], s) and _eq(ts[:, 1, :cout], q), schedule
        assert not ts[:, :, cout:].cpu().ne(0).any(), schedule                  # (NaN != 0: the padded rows are written, as zeros)


# ----------------------------------------------------------------------------------------------
# pixel ranges (in the ABI; no caller in the repository passes a non-zero one)
# ----------------------------------------------------------------------------------------------
def _gemm_range(ops, spec, x, packed, table, out, shift, pix_begin, pix_count):
    lib = ops.L.load()
    ws = ops.L.workspace(lib.dasac_conv_gemm_workspace(), x.device, owner="conv_gemm")
    N, Cx, H, W = x.shape
    OH, OW = out.shape[2:]
    return lib.dasac_conv_gemm(x.data_ptr(), packed.data_ptr(), table.data_ptr(), out.data_ptr(), N, Cx, H, W, OH, OW, spec.stride,
                               spec.cout, spec.K, OH, OW, 1, shift.data_ptr(), 0, 0, 0, 0, 1, pix_begin, pix_count, 0,
                               ws.data_ptr(), ws.numel(), ops.L.stream_ptr())


@pytest.mark.parametrize("case", PIX_CASES, ids=[c[0] for c in PIX_CASES])
def test_pixel_ranges_write_exactly_their_tiles(case):
    from dasac_hip import ops
    name, cin, cout, br, stride, (N, H, W) = case
    spec, o, table, packed = _gemm_case(case)
    assert cl.exact_ok(o["x"], o["ws"], br, stride, None, None, o["shift"], parts=("fwd",))
    want = cl.f32(torch.relu(cl.conv_fwd(o["x"], o["ws"], br, stride) + _bc(o["shift"]))).permute(1, 0, 2, 3).reshape(cout, -1)
    npix = N * H * W
    tile = 256 if ops.L.load().dasac_conv_mpad(cout) == 32 else 128
    assert npix % tile != 0 and npix > 5 * tile
    xd, shift = o["x"].cuda(), o["shift"].cuda()
    for begin, count in ((tile, 2 * tile), (npix // tile * tile - tile, 0), (0, tile)):
        out = torch.full((N, cout, H, W), NAN, device="cuda")
        rc = _gemm_range(ops, spec, xd, packed, table, out, shift, begin, count)
        assert rc == 0, ops.L.load().dasac_last_error()
        end = begin + count if count else npix
        got = out.cpu().permute(1, 0, 2, 3).reshape(cout, -1)
        assert torch.equal(got[:, begin:end], want[:, begin:end]), (begin, count)
        assert bool(torch.isnan(got[:, :begin]).all()) and bool(torch.isnan(got[:, end:]).all()), (begin, count)
    # a range that does not start on a tile is refused on the host: nothing is launched, nothing written
    out = torch.full((N, cout, H, W), NAN, device="cuda")
    for begin, count in ((tile // 2, tile), (tile, tile // 2), (128 if tile == 256 else 64, 0)):
        assert _gemm_range(ops, spec, xd, packed, table, out, shift, begin, count) == -1      # DASAC_EINVAL
        assert b"whole" in ops.L.load().dasac_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())


def test_batched_launch_is_exact_and_stays_inside_its_entries():
    from dasac_hip import ops
    lib = ops.L.load()
    B, C, M, T = BATCHED
    spec = ops.ConvSpec(C, M, [(1, 1, 1, 0)], 1)
    kp, mp = lib.dasac_conv_kpad(C), lib.dasac_conv_mpad(M)
    gx, gw, go = 36, 8, 20                                    # gaps in elements (strides stay multiples of 4)
    nx, nw, no = C * T, kp * mp, M * T
    xb = torch.full((B, nx + gx), NAN, device="cuda")
    wb = torch.full((B, nw + gw), NAN, device="cuda")
    ob = torch.full((B, no + go), NAN, device="cuda")
    refs = []
    for b in range(B):
        o = cl.plain_operands(C, M, spec.branches, 1, (1, 1, T), seed=b)
        assert cl.exact_ok(o["x"], o["ws"], spec.branches, 1, parts=("fwd",))
        xb[b, :nx] = o["x"].reshape(-1).cuda()
        ops.conv_pack(spec, [o["ws"][0].cuda()], False, None, out=wb[b, :nw].view(kp, mp))
        refs.append(cl.conv_fwd(o["x"], o["ws"], spec.branches, 1))
    assert not torch.equal(refs[0], refs[1])
    xs, ws, os_ = xb[:, :nx].view(B, 1, C, 1, T), wb[:, :nw].view(B, kp, mp), ob[:, :no].view(B, 1, M, 1, T)
    assert xs.stride(0) > nx and ws.stride(0) > nw and os_.stride(0) > no
    ops.conv_gemm_batched(xs, ws, ops._winograd_table(C, T, xb.device), os_, (1, T), 1, M, C)
    for b in range(B):
        assert _eq(os_[b], refs[b]), b
    assert bool(torch.isnan(ob[:, no:]).all())


# ----------------------------------------------------------------------------------------------
# Winograd F(2x2,3x3)
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", WINO_SHAPES, ids=["{}x{}to{}_{}x{}_d{}".format(*s) for s in WINO_SHAPES])
def test_winograd_forward_and_data_gradient_are_exact(shape):
    """G holds +-1 and 0.5 only: with g = scale * w on a lattice, U = G g G^T lies on a quarter of g's spacing, V = B^T d B and the
    output transform on integers; so the three transforms and the sixteen point GEMMs reproduce the direct convolution's bits."""
    from dasac_hip import ops
    N, cin, cout, H, W, d = shape
    br = [(3, 3, d, d)]
    spec = ops.ConvSpec(cin, cout, br)
    o = cl.plain_operands(cin, cout, br, 1, (N, H, W))
    x, w, dz, scale, shift = o["x"], o["ws"][0], o["dz"], o["scale"], o["shift"]
    wt = w.flip(2, 3).transpose(0, 1).contiguous() * scale.view(1, -1, 1, 1)
    assert cl.exact_ok(x, [w], br, 1, dz, scale, shift, parts=("fwd", "dx"))
    assert cl.winograd_exact_ok(x, w, d, scale) and cl.winograd_exact_ok(dz, wt, d, None, cl.winograd_quantum(scale))
    assert ops.winograd_ok(spec, False) and ops.winograd_ok(spec, True)
    xd, wd, sd = x.cuda(), w.cuda(), scale.cuda()

    fwd = cl.conv_fwd(x, [w], br, 1, scale)
    u = ops.winograd_filter(spec, wd, False, sd)
    assert _eq(ops.winograd_conv(xd, u, torch.full((N, cout, H, W), NAN, device="cuda"), d), fwd)
    bits = ops.ReluBits(N, cout, H, W, xd.device)
    bits.words.fill_(-1)
    want = torch.relu(fwd + _bc(shift))
    assert 0.1 < float((want > 0).double().mean()) < 0.9
    assert _eq(ops.winograd_conv(xd, u, torch.full((N, cout, H, W), NAN, device="cuda"), d, shift.cuda(), True, bits_out=bits), want)
    assert torch.equal(cl.unpack_bits(bits.words, (N, cout, H, W)).cpu(), want > 0)

    ut = ops.winograd_filter(spec, wd, True, sd)
    dx = ops.winograd_conv(dz.cuda(), ut, torch.full((N, cin, H, W), NAN, device="cuda"), d)
    assert _eq(dx, cl.conv_dx(dz, [w], br, 1, (H, W), scale))


# ----------------------------------------------------------------------------------------------
# split-bf16
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["A", "B"])
@pytest.mark.parametrize("case", X3_CASES, ids=["{}to{}".format(c[0], c[1]) for c in X3_CASES])
def test_split_bf16_kernels_are_exact_on_both_operand_classes(case, cls):
    """Three bf16 MFMAs per product, head x head + head x tail + tail x head: class A puts the non-zero tails on the streamed
    operand, class B on the other one, so each cross term is needed for the exact result and tail x tail is exactly zero."""
    from dasac_hip import ops
    cin, cout, br, stride, H, W = case
    N = X3_BATCH
    spec = ops.ConvSpec(cin, cout, br, stride)
    o = cl.x3_operands(cls, cin, cout, br, stride, (N, H, W))
    (x, ws), (dz, wd), (gz, gx) = o["fwd"], o["dgrad"], o["wgrad"]
    shift, res, mask = o["shift"], o["res_out"], o["mask_in"]
    assert x3_exact_ok(o, br, stride)
    ops.set_precision("bf16x3")
    try:
        wsd = [w.cuda() for w in ws]
        assert ops.conv_pack(spec, wsd, False).dasac_x3
        y = ops.conv_forward(spec, x.cuda(), wsd, shift=shift.cuda(), res=res.cuda(), relu=True)
        assert _eq(y, torch.relu(cl.conv_fwd(x, ws, br, stride) + _bc(shift) + res.double()))
        if cin >= 64:
            dxr = cl.conv_dx(dz, wd, br, stride, (H, W))
            dx = ops.conv_dgrad(spec, dz.cuda(), [w.cuda() for w in wd], (H, W), mask=mask.cuda())
            assert _eq(dx, torch.where(mask > 0, dxr, torch.zeros_like(dxr)))
        sums = torch.full((cout,), NAN, device="cuda")
        gws = ops.conv_wgrad(spec, gz.cuda(), gx.cuda(), wsd, sum_dz=sums, outs=[torch.full_like(w, NAN) for w in wsd])
        for a, b in zip(gws, cl.conv_dw(gz, gx, ws, br, stride)):
            assert _eq(a, b)
        assert _eq(sums, gz.double().sum((0, 2, 3)))
    finally:
        ops.set_precision("fp32")


# ----------------------------------------------------------------------------------------------
# tap-expanded ASPP convolution
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", EXPANDED, ids=[c[0] for c in EXPANDED])
def test_expanded_conv_is_exact(case):
    from dasac_hip import ops
    name, cin, cout, br, (N, H, W), prec = case
    spec = ops.ConvSpec(cin, cout, br, 1)
    ex = ops.ExpandedConv(spec)
    o = expanded_operands(case)
    x, ws, dout, bias, res = o["x"], o["ws"], o["dz"], o["shift"], o["res_in"]
    assert cl.exact_ok(x, ws, br, 1, dout, None, bias, None, res)
    saved = ops.PRECISION
    ops.set_precision(prec)
    try:
        xd, wd, doutd = x.cuda(), [w.cuda() for w in ws], dout.cuda()
        packed_f, packed_t = ex.pack(wd, False), ex.pack(wd, True)
        table_f, table_t = ops.conv_table(ex.spec1, H, W, False, xd.device), ops.conv_table(ex.spec1, H, W, True, xd.device)
        assert _eq(ex.forward(xd, packed_f, table_f, bias.cuda()), cl.conv_fwd(x, ws, br, 1) + _bc(bias))
        d = ex.scatter(doutd)
        for a, b in zip(ex.wgrad(d, xd, wd, table_f, outs=[torch.full_like(w, NAN) for w in wd]), cl.conv_dw(dout, x, ws, br, 1)):
            assert _eq(a, b)
        dxr = cl.conv_dx(dout, ws, br, 1, (H, W))
        assert _eq(ex.dgrad(d, packed_t, table_t, (H, W)), dxr)
        want = torch.where(x > 0, dxr + res.double(), torch.zeros_like(dxr))
        assert _eq(ex.dgrad(d, packed_t, table_t, (H, W), res=res.cuda(), mask=xd), want)
    finally:
        ops.set_precision(saved)
