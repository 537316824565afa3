"""The conv GEMM's hand-off schedules and the weight gradient's pixel splits, bit for bit, at the points where their integer rules
branch (conv_lattice.py: STREAMK_CASES, TAIL_CASES, WGRAD_CASES; gemm_schedule_ref.py names what each plan reaches and
test_gemm_schedule_cpu.py checks that from the model): stream-K ranges that span tiles, ranges that are whole tiles, ranges
aligned to tiles, 143 contributors to one tile, ragged M and pixel tiles, three M tiles, every reserved-CU grid, a pixel range, the
split-bf16 kernel; split-K tails whose K-steps do not divide, whose pieces return early, whose leading rounds are not whole, two
leading rounds; weight gradients with empty trailing splits, 64 splits and the 768-split branch.

Every comparison is torch.equal against the integer reference on operands whose every partial sum fp32 holds exactly (the
precondition is asserted before any output is looked at), outputs start as NaN, and the hand-off flags are clean after every
launch that uses them.  The plan each case was written for is asserted from the library itself before the kernel runs."""
import pytest
import torch

import conv_lattice as cl
import gemm_schedule_ref as R
import test_gpu_conv_exact as E
from conv_lattice import STREAMK_CASES, STREAMK_RESERVED_CASES, STREAMK_X3_CASES, TAIL_CASES, WGRAD_CASES, WGRAD_X3_CASES

pytestmark = pytest.mark.gpu
NAN = float("nan")
F32 = torch.float32
_ids = lambda cases: [c[0] for c in cases]


@pytest.fixture(scope="module")
def refs():
    """Operands and references of the stream-K cases, shared by the tests of this module and dropped when it ends."""
    cache = {}
    yield cache
    cache.clear()


def _forward_case(case, cache=None):
    """(operands, fp32 reference as float64) of a case; kept in `cache` when one is given.  The reference is ATen's fp32 CPU
    convolution: exact on the lattice (test_conv_exact_cpu.py holds it against float64 for these cases), and the precondition in
    fp32 is as good as in float64 -- a sum of non-negative terms that reached 2^24 cannot round back below it."""
    if cache is not None and case[0] in cache:
        return cache[case[0]]
    name, cin, cout, br, stride, shape = case
    o = cl.plain_operands(cin, cout, br, stride, shape)
    assert cl.exact_ok(o["x"], o["ws"], br, stride, None, None, o["shift"], o["res_out"], dtype=F32, parts=("fwd",))
    got = (o, cl.conv_fwd(o["x"], o["ws"], br, stride, None, F32).double())
    if cache is not None:
        cache[case[0]] = got
    return got


def _packed(case, o):
    from dasac_hip import ops
    name, cin, cout, br, stride, shape = case
    spec = ops.ConvSpec(cin, cout, br, stride)
    order = ops.gemm_order(spec, False)
    table = ops.conv_table(spec, shape[1], shape[2], False, torch.device("cuda", 0), order)
    return spec, table, ops.conv_pack(spec, [w.cuda() for w in o["ws"]], False, None, order=order)


def _out_shape(case):
    name, cin, cout, br, stride, (N, H, W) = case
    return (N, cout) + cl.out_hw(br, stride, H, W)


def _streamk_runs(lib, case, npix=None):
    """The library runs one block per tile whatever is asked when the (tile, K-step) space has fewer steps than workers: the test
    states that inequality itself, next to the span name (which only repeats what was asked for).  npix: the pixels of a launch
    over a pixel range."""
    M, Npix, K = cl.gemm_shape(case)
    m_tiles, n_tiles, KT = R.gemm_tiles(1, 1, Npix if npix is None else npix, M, K)
    reserved = lib.dasac_reserved_cus()
    return (lib.dasac_conv_mpad(M) % 128 == 0 and m_tiles * n_tiles * KT >= R.sk_workers(reserved)
            and R.simulate_gemm(m_tiles, n_tiles, KT, reserved, 2, compact=True)["kind"] == "stream-K")


def _launches(spans):
    return {k: v["launches"] for k, v in spans.items()}


# ----------------------------------------------------------------------------------------------
# stream-K, forced
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STREAMK_CASES, ids=_ids(STREAMK_CASES))
def test_stream_k_equals_the_reference(case, refs):
    from dasac_hip import ops
    lib = ops.L.load()
    o, ref = _forward_case(case, refs)
    spec, table, packed = _packed(case, o)
    shape = _out_shape(case)
    assert lib.dasac_reserved_cus() == 0 and _streamk_runs(lib, case)
    # "spans" takes the four epilogues of the network, the others the plain store and the fused shift + residual + ReLU
    epis = ["none", "shift_res_relu_bits", "res_mask_bits", "res_mask_fp32"] if case[0] == "spans" else ["none", "shift_res_relu_bits"]
    assert ops.bits_ok(case[2], case[1])
    ops.PROFILE.start()
    try:
        for epi in epis:
            E._run_epilogue(ops, spec, o, table, packed, shape, E._epilogue(epi, o, ref, shape, cl.gen(21)), 2)
    finally:
        spans = ops.PROFILE.stop()
    assert _launches(spans) == {"conv_gemm<stream-K>": len(epis)}
    assert E._flags_clean(ops)


@pytest.mark.parametrize("reserved", cl.RESERVED)
@pytest.mark.parametrize("case", STREAMK_RESERVED_CASES, ids=_ids(STREAMK_RESERVED_CASES))
def test_stream_k_on_every_reserved_cu_grid(case, reserved, refs):
    """768, 744, 576 and 384 workers cut the same space into other ranges; each grid gives the reference's bits."""
    from dasac_hip import ops
    lib = ops.L.load()
    o, ref = _forward_case(case, refs)
    spec, table, packed = _packed(case, o)
    shape = _out_shape(case)
    prev = lib.dasac_set_reserved_cus(reserved)
    try:
        assert lib.dasac_reserved_cus() == reserved and _streamk_runs(lib, case)
        ops.PROFILE.start()
        try:
            E._run_epilogue(ops, spec, o, table, packed, shape, E._epilogue("none", o, ref, shape, None), 2)
        finally:
            spans = ops.PROFILE.stop()
        assert _launches(spans) == {"conv_gemm<stream-K>": 1}
        assert E._flags_clean(ops)
    finally:
        lib.dasac_set_reserved_cus(prev)


def test_stream_k_over_a_pixel_range_that_starts_past_tile_zero(refs):
    """Tiles 37 .. 185 (19072 steps: a range deposits, runs a whole tile and owns a cut one) and tiles 163 .. 199 (ranges inside a
    tile) of "spans": the range's pixels equal the reference, every other pixel keeps its NaN."""
    from dasac_hip import ops
    lib = ops.L.load()
    case = STREAMK_CASES[0]
    name, cin, cout, br, stride, (N, H, W) = case
    o, ref = _forward_case(case, refs)
    spec, table, packed = _packed(case, o)
    want = cl.f32(torch.relu(ref + E._bc(o["shift"]))).permute(1, 0, 2, 3).reshape(cout, -1)
    npix = N * H * W
    xd, shift = o["x"].cuda(), o["shift"].cuda()
    ws = ops.L.workspace(lib.dasac_conv_gemm_workspace(), xd.device, owner="conv_gemm")
    for begin, count in ((37 * 128, 149 * 128), (163 * 128, 0)):
        end = begin + count if count else npix
        assert _streamk_runs(lib, case, end - begin)
        out = torch.full((N, cout, H, W), NAN, device="cuda")
        # (the C entry point itself, as test_pixel_ranges_write_exactly_their_tiles calls it: the Python wrapper, which names the
        # spans, has no pixel range.  Schedule 2 is passed here in person, and the model says that the library honours it.)
        rc = lib.dasac_conv_gemm(xd.data_ptr(), packed.data_ptr(), table.data_ptr(), out.data_ptr(), N, cin, H, W, H, W, stride, cout,
                                 spec.K, H, W, 1, shift.data_ptr(), 0, 0, 0, 0, 1, begin, count, 2, ws.data_ptr(), ws.numel(),
                                 ops.L.stream_ptr())
        assert rc == 0, lib.dasac_last_error()
        got = out.cpu().permute(1, 0, 2, 3).reshape(cout, -1)
        assert torch.equal(got[:, begin:end], want[:, begin:end]), (begin, count)
        assert bool(torch.isnan(got[:, :begin]).all()) and bool(torch.isnan(got[:, end:]).all()), (begin, count)
        assert E._flags_clean(ops)


@pytest.mark.parametrize("cls", ["A", "B"])
@pytest.mark.parametrize("case", STREAMK_X3_CASES, ids=_ids(STREAMK_X3_CASES))
def test_stream_k_in_the_split_bf16_kernel(case, cls):
    from dasac_hip import ops
    lib = ops.L.load()
    name, cin, cout, br, stride, shape = case
    o = cl.x3_operands(cls, cin, cout, br, stride, shape)
    x, ws = o["fwd"]
    shift, res = o["shift"], o["res_out"]
    assert cl.exact_ok(x, ws, br, stride, None, None, shift, res, dtype=F32, parts=("fwd",))
    want = torch.relu(cl.conv_fwd(x, ws, br, stride, None, F32).double() + E._bc(shift) + res.double())
    spec = ops.ConvSpec(cin, cout, br, stride)
    order = ops.gemm_order(spec, False)
    oshape = _out_shape(case)
    assert _streamk_runs(lib, case)
    saved = ops.PRECISION
    ops.set_precision("bf16x3")
    try:
        packed = ops.conv_pack(spec, [w.cuda() for w in ws], False, None, order=order)
        assert packed.dasac_x3
        table = ops.conv_table(spec, shape[1], shape[2], False, torch.device("cuda", 0), order)
        out = torch.full(oshape, NAN, device="cuda")
        ops.PROFILE.start()
        try:
            ops.conv_gemm(x.cuda(), packed, table, out, oshape[2:], stride, cout, spec.K, 1, shift.cuda(), res.cuda(), None, True, schedule=2)
        finally:
            spans = ops.PROFILE.stop()
    finally:
        ops.set_precision(saved)
    assert _launches(spans) == {"conv_gemm<stream-K>": 1}
    assert E._eq(out, want)
    assert E._flags_clean(ops)


# ----------------------------------------------------------------------------------------------
# split-K tail, the library's own choice
# ----------------------------------------------------------------------------------------------
TAIL_PLANS = {"split5": (5, 128), "m3": (8, 341), "m5": (8, 204), "two_rounds": (8, 256), "reserved8": (8, 128)}     # split, lead_n


@pytest.mark.parametrize("case", TAIL_CASES, ids=_ids(TAIL_CASES))
def test_split_k_tail_plans_equal_the_reference(case):
    from dasac_hip import ops
    lib = ops.L.load()
    name, cin, cout, br, stride, (N, H, W) = case
    M, Npix, K = cl.gemm_shape(case)
    reserved = cl.TAIL_RESERVED.get(name, 0)
    o, ref = _forward_case(case)
    spec, table, packed = _packed(case, o)
    shape = _out_shape(case)
    prev = lib.dasac_set_reserved_cus(reserved)
    try:
        split = lib.dasac_conv_gemm_tail_split(N, H, W, cout, spec.K)
        plan = R.tail_plan(*R.gemm_tiles(1, 1, Npix, M, K), lib.dasac_reserved_cus())
        print("tail plan {}: split {}, lead_n {} (model: {})".format(name, split, plan[1], plan))
        assert lib.dasac_reserved_cus() == reserved and split == plan[0] and plan == TAIL_PLANS[name]
        ops.PROFILE.start()
        try:
            for epi in ("none", "shift_res_relu_bits"):
                e = E._epilogue(epi, o, ref, shape, cl.gen(22))
                for schedule in (None, 1):
                    E._run_epilogue(ops, spec, o, table, packed, shape, e, schedule)
        finally:
            spans = ops.PROFILE.stop()
        assert _launches(spans) == {"conv_gemm<tile+tail>": 2, "conv_gemm<tile-per-block>": 2}
        assert E._flags_clean(ops)
    finally:
        lib.dasac_set_reserved_cus(prev)


# ----------------------------------------------------------------------------------------------
# weight gradient
# ----------------------------------------------------------------------------------------------
def _poison_scratch(ops, nbytes):
    """0xFF over the stream's cached scratch buffer (all-ones words are NaN): a slab or a Psum row that a reduce kernel reads but no
    split wrote shows up in the result."""
    ws = ops.L.workspace(nbytes, torch.device("cuda", torch.cuda.current_device()))
    ws.fill_(0xFF)
    return ws


def _wgrad_plan(lib, case):
    name, cin, cout, br, stride, (N, H, W) = case
    M, Npix, K = cl.gemm_shape(case)
    plan = R.simulate_wgrad(M, K, cin, Npix)
    OH, OW = cl.out_hw(br, stride, H, W)
    nbytes = lib.dasac_conv_wgrad_workspace(N, OH, OW, M, K)
    assert nbytes == R.wgrad_workspace(N, OH, OW, M, K) >= plan["splits"] * plan["Mpad"] * (plan["Kpad"] + 1) * 4
    print("wgrad plan {}: {} splits of {} pixels, {} empty".format(name, plan["splits"], plan["per"], plan["empty"]))
    return plan, nbytes


@pytest.mark.parametrize("case", WGRAD_CASES, ids=_ids(WGRAD_CASES))
def test_weight_gradient_split_plans_are_exact(case):
    from dasac_hip import ops
    lib = ops.L.load()
    name, cin, cout, br, stride, shape = case
    spec = ops.ConvSpec(cin, cout, br, stride)
    o = cl.wgrad_operands(case)
    x, w, dz, scale = o["x"], o["ws"][0], o["dz"], o["scale"]
    assert cl.exact_ok(x, [w], br, stride, dz, scale, parts=("dw",)) and cl.dot_exact_ok(w, dz, x, br, stride)
    plan, nbytes = _wgrad_plan(lib, case)
    (gu,) = cl.conv_dw(dz, x, [w], br, stride)                                     # unscaled G
    want_rows, want_sums = cl.dot_rows_ref(w, gu, flat=cin < 32), dz.double().sum((0, 2, 3))
    rows = ops.dot_rows(spec)
    assert want_rows.shape == (rows, cout)
    dot = torch.full((rows, cout), NAN, device="cuda")
    sums = torch.full((cout,), NAN, device="cuda")
    wd = w.cuda()
    _poison_scratch(ops, nbytes)
    (gw,) = ops.conv_wgrad(spec, dz.cuda(), x.cuda(), [wd], scale=scale.cuda(), dot=dot, sum_dz=sums, outs=[torch.full_like(wd, NAN)])
    assert E._eq(gw, gu * scale.double().view(-1, 1, 1, 1))
    assert E._eq(sums, want_sums) and E._eq(dot, want_rows)
    assert bool((gu != 0).any()) and all(bool(want_rows[r].abs().sum() > 0) for r in range(rows))


@pytest.mark.parametrize("cls", ["A", "B"])
@pytest.mark.parametrize("case", WGRAD_X3_CASES, ids=_ids(WGRAD_X3_CASES))
def test_split_bf16_weight_gradient_split_plans_are_exact(case, cls):
    from dasac_hip import ops
    lib = ops.L.load()
    name, cin, cout, br, stride, shape = case
    spec = ops.ConvSpec(cin, cout, br, stride)
    o = cl.x3_operands(cls, cin, cout, br, stride, shape)
    gz, gx = o["wgrad"]
    ws = [torch.zeros(cout, cin, kh, kw) for kh, kw, _, _ in br]
    assert cl.exact_ok(gx, ws, br, stride, gz, parts=("dw",))
    plan, nbytes = _wgrad_plan(lib, case)
    want, want_sums = cl.conv_dw(gz, gx, ws, br, stride), gz.double().sum((0, 2, 3))
    sums = torch.full((cout,), NAN, device="cuda")
    wsd = [w.cuda() for w in ws]
    saved = ops.PRECISION
    ops.set_precision("bf16x3")
    try:
        _poison_scratch(ops, nbytes)
        gws = ops.conv_wgrad(spec, gz.cuda(), gx.cuda(), wsd, sum_dz=sums, outs=[torch.full_like(w, NAN) for w in wsd])
    finally:
        ops.set_precision(saved)
    for a, b in zip(gws, want):
        assert E._eq(a, b)
    assert E._eq(sums, want_sums)
