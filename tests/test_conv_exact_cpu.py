"""The lattice claims behind test_gpu_conv_exact.py, checked without a GPU: for every case that file runs, the exactness
precondition holds, ATen's fp32 CPU convolutions (one independent summation order) reproduce the float64 references bit for bit,
an fp32 numpy emulation of the F(2x2,3x3) transforms does too, and the split-bf16 operand classes leave one operand of every
product without a tail."""
import numpy as np
import pytest
import torch

import conv_lattice as cl
from conv_lattice import BATCHED, PIX_CASES, SCHEDULE_CASE, TAIL_CASE, X3_BATCH, expanded_operands, x3_exact_ok
from conv_lattice import STREAMK_CASES, STREAMK_X3_CASES, TAIL_CASES, WGRAD_CASES, WGRAD_X3_CASES

_LISTS = cl.case_lists()
CONV_CASES, DOT_CASES, STATS, WINO_SHAPES, X3_CASES, EXPANDED = (_LISTS[k] for k in ("conv", "dot", "stats", "winograd", "x3", "expanded"))

F32 = torch.float32


def _check_plain(cin, cout, branches, stride, shape, scaled, seed=0, dgrad=True):
    o = cl.plain_operands(cin, cout, branches, stride, shape, seed)
    scale = o["scale"] if scaled else None
    assert cl.exact_ok(o["x"], o["ws"], branches, stride, o["dz"] if dgrad else None, scale, o["shift"], o["res_out"], o["res_in"])
    ref = cl.conv_fwd(o["x"], o["ws"], branches, stride, scale)
    assert torch.equal(cl.conv_fwd(o["x"], o["ws"], branches, stride, scale, F32), cl.f32(ref))
    assert 0.1 < float((ref + o["shift"].view(1, -1, 1, 1) + o["res_out"] > 0).double().mean()) < 0.9      # a mixed ReLU pattern
    if dgrad:
        dx = cl.conv_dx(o["dz"], o["ws"], branches, stride, shape[1:], scale)
        assert torch.equal(cl.conv_dx(o["dz"], o["ws"], branches, stride, shape[1:], scale, F32), cl.f32(dx))
        for a, b in zip(cl.conv_dw(o["dz"], o["x"], o["ws"], branches, stride, scale, F32), cl.conv_dw(o["dz"], o["x"], o["ws"], branches, stride, scale)):
            assert torch.equal(a, cl.f32(b))
    return o


@pytest.mark.parametrize("scaled", [False, True], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_plain_lattice_is_exact_in_fp32(case, scaled):
    name, cin, cout, branches, stride, shape = case
    _check_plain(cin, cout, branches, stride, shape, scaled)


@pytest.mark.parametrize("case", DOT_CASES, ids=[c[0] for c in DOT_CASES])
def test_dot_rows_and_bn_param_grads_stay_exact(case):
    name, cin, cout, branches, stride, shape = case
    o = cl.plain_operands(cin, cout, branches, stride, shape)
    assert cl.dot_exact_ok(o["ws"][0], o["dz"], o["x"], branches, stride)
    (g,) = cl.conv_dw(o["dz"], o["x"], o["ws"], branches, stride)
    rows = cl.dot_rows_ref(o["ws"][0], g)
    assert rows.shape == ((cin + 63) // 64, cout) and torch.equal(cl.f32(rows).double(), rows)
    (ga,) = cl.conv_dw(o["dz"].abs(), o["x"].abs(), [o["ws"][0].abs()], branches, stride)
    mean, bias = cl.ints((cout,), 8, cl.gen(1)), cl.ints((cout,), 8, cl.gen(2))
    assert cl.bn_param_grads_exact_ok(cl.dot_rows_ref(o["ws"][0].abs(), ga), o["dz"].abs().sum((0, 2, 3)), mean, bias)


def test_schedule_tail_pixel_range_and_batched_cases():
    for name, cin, cout, branches, stride, shape in [SCHEDULE_CASE] + PIX_CASES:
        _check_plain(cin, cout, branches, stride, shape, False, dgrad=False)
    B, C, M, T = BATCHED
    for b in range(B):
        _check_plain(C, M, [(1, 1, 1, 0)], 1, (1, 1, T), False, seed=b, dgrad=False)


def test_split_k_tail_case():
    """The largest case: float64 once here; the GPU test may then lean on the fp32 CPU convolution, exact on the lattice."""
    name, cin, cout, branches, stride, shape = TAIL_CASE
    _check_plain(cin, cout, branches, stride, shape, False, dgrad=False)


@pytest.mark.parametrize("case", STATS, ids=[c[0] for c in STATS])
def test_statistics_lattice(case):
    name, cin, cout, br, shape = case[:5]
    o = cl.stats_operands(cin, cout, br, shape)
    assert all(set(t.unique().tolist()) <= {-1.0, 0.0, 1.0} for t in (o["x"], o["ws"][0]))
    assert cl.exact_ok(o["x"], o["ws"], [br], 1, shift=o["bias"])
    ref = cl.conv_fwd(o["x"], o["ws"], [br], 1) + o["bias"].view(1, -1, 1, 1)
    assert cl.stats_exact_ok(ref)
    assert torch.equal(cl.conv_fwd(o["x"], o["ws"], [br], 1, None, F32) + o["bias"].view(1, -1, 1, 1), cl.f32(ref))
    s, q = cl.tile_sums(ref)
    out32 = cl.f32(ref).permute(1, 0, 2, 3).reshape(cout, -1)
    for t in range(s.shape[0]):                      # fp32 sums of a tile in index order: the same integers
        seg = out32[:, 128 * t:128 * (t + 1)]
        assert torch.equal(seg.sum(1).double(), s[t]) and torch.equal((seg * seg).sum(1).double(), q[t])


@pytest.mark.parametrize("shape", WINO_SHAPES, ids=["{}x{}to{}_{}x{}_d{}".format(*s) for s in WINO_SHAPES])
def test_winograd_transforms_are_exact_on_the_lattice(shape):
    N, cin, cout, H, W, d = shape
    br = [(3, 3, d, d)]
    o = cl.plain_operands(cin, cout, br, 1, (N, H, W))
    w, scale = o["ws"][0], o["scale"]
    assert cl.exact_ok(o["x"], o["ws"], br, 1, o["dz"], scale, o["shift"])
    wt = w.flip(2, 3).transpose(0, 1).contiguous()                      # the data gradient's filter: rotated, channels swapped
    assert cl.winograd_exact_ok(o["x"], w, d, scale)
    assert cl.winograd_exact_ok(o["dz"], wt * scale.view(1, -1, 1, 1), d, None, cl.winograd_quantum(scale)) and cl.winograd_quantum(scale) >= 0.125
    # U on multiples of the quantum, V and the output on integers
    u = np.einsum("ai,mcij,bj->mcab", cl.WG, (w.double() * scale.double().view(-1, 1, 1, 1)).numpy(), cl.WG)
    assert np.array_equal(u / cl.winograd_quantum(scale), np.round(u / cl.winograd_quantum(scale)))
    fwd = cl.conv_fwd(o["x"], o["ws"], br, 1, scale)
    assert torch.equal(cl.winograd_emulate(o["x"], w, d, scale), cl.f32(fwd))
    dx = cl.conv_dx(o["dz"], o["ws"], br, 1, (H, W), scale)
    assert torch.equal(cl.winograd_emulate(o["dz"], wt * scale.view(1, -1, 1, 1), d), cl.f32(dx))


@pytest.mark.parametrize("cls", ["A", "B"])
@pytest.mark.parametrize("case", X3_CASES, ids=["{}to{}".format(c[0], c[1]) for c in X3_CASES])
def test_split_bf16_classes(case, cls):
    cin, cout, branches, stride, H, W = case
    shape = (X3_BATCH, H, W)
    o = cl.x3_operands(cls, cin, cout, branches, stride, shape)
    x, ws = o["fwd"]
    dz, wd = o["dgrad"]
    gz, gx = o["wgrad"]
    tails = 0
    for a, bs in ((x, ws), (dz, wd), (gz, [gx])):
        ha, ta = cl.bf16_split(a)
        assert np.array_equal(ha.astype(np.float64) + ta, a.numpy())                      # head + tail is the operand, exactly
        for b in bs:
            hb, tb = cl.bf16_split(b)
            assert np.array_equal(hb.astype(np.float64) + tb, b.numpy())
            assert not ta.any() or not tb.any()                                            # tail x tail is exactly zero
            assert ta.any() or tb.any()                                                    # and one cross term is live
            tails += int(ta.any()) - int(tb.any())
    assert tails == (3 if cls == "A" else -3)                                             # A: the streamed operand; B: the other one
    assert x3_exact_ok(o, branches, stride)
    ref = cl.conv_fwd(x, ws, branches, stride)
    assert torch.equal(cl.conv_fwd(x, ws, branches, stride, None, F32), cl.f32(ref))
    dxr = cl.conv_dx(dz, wd, branches, stride, (H, W))
    assert torch.equal(cl.conv_dx(dz, wd, branches, stride, (H, W), None, F32), cl.f32(dxr))
    for a, b in zip(cl.conv_dw(gz, gx, ws, branches, stride, None, F32), cl.conv_dw(gz, gx, ws, branches, stride)):
        assert torch.equal(a, cl.f32(b))


@pytest.mark.parametrize("case", EXPANDED, ids=[c[0] for c in EXPANDED])
def test_expanded_cases(case):
    name, cin, cout, branches, shape, prec = case
    o = expanded_operands(case)
    assert float(o["x"].min()) >= 0
    assert cl.exact_ok(o["x"], o["ws"], branches, 1, o["dz"], None, o["shift"], None, o["res_in"])
    ref = cl.conv_fwd(o["x"], o["ws"], branches, 1)
    assert torch.equal(cl.conv_fwd(o["x"], o["ws"], branches, 1, None, F32), cl.f32(ref))
    dxr = cl.conv_dx(o["dz"], o["ws"], branches, 1, shape[1:])
    assert torch.equal(cl.conv_dx(o["dz"], o["ws"], branches, 1, shape[1:], None, F32), cl.f32(dxr))
    for a, b in zip(cl.conv_dw(o["dz"], o["x"], o["ws"], branches, 1, None, F32), cl.conv_dw(o["dz"], o["x"], o["ws"], branches, 1)):
        assert torch.equal(a, cl.f32(b))


# ----------------------------------------------------------------------------------------------
# the cases of test_gpu_conv_schedules_exact.py
# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", STREAMK_CASES + TAIL_CASES, ids=[c[0] for c in STREAMK_CASES + TAIL_CASES])
def test_schedule_lattice_cases(case):
    """float64 once here: the GPU tests then lean on the fp32 CPU convolution, exact on the lattice."""
    name, cin, cout, branches, stride, shape = case
    _check_plain(cin, cout, branches, stride, shape, False, dgrad=False)


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_weight_gradient_split_cases(case):
    name, cin, cout, branches, stride, shape = case
    o = cl.wgrad_operands(case)
    x, w, dz, scale = o["x"], o["ws"][0], o["dz"], o["scale"]
    assert cl.exact_ok(x, [w], branches, stride, dz, scale, parts=("dw",)) and cl.dot_exact_ok(w, dz, x, branches, stride)
    (g,) = cl.conv_dw(dz, x, [w], branches, stride)
    (g32,) = cl.conv_dw(dz, x, [w], branches, stride, None, F32)
    assert torch.equal(g32, cl.f32(g)) and torch.equal(cl.f32(g * scale.double().view(-1, 1, 1, 1)).double(), g * scale.double().view(-1, 1, 1, 1))
    rows = cl.dot_rows_ref(w, g, flat=cin < 32)
    assert rows.shape == ((cin * (w.shape[2] * w.shape[3] if cin < 32 else 1) + 63) // 64, cout) and torch.equal(cl.f32(rows).double(), rows)
    assert bool((rows.abs().sum(1) > 0).all())


@pytest.mark.parametrize("cls", ["A", "B"])
@pytest.mark.parametrize("case", STREAMK_X3_CASES + WGRAD_X3_CASES, ids=[c[0] for c in STREAMK_X3_CASES + WGRAD_X3_CASES])
def test_split_bf16_schedule_and_split_cases(case, cls):
    name, cin, cout, branches, stride, shape = case
    o = cl.x3_operands(cls, cin, cout, branches, stride, shape)
    pairs = [(o["fwd"][0], o["fwd"][1])] if case in STREAMK_X3_CASES else [(o["wgrad"][0], [o["wgrad"][1]])]
    for a, bs in pairs:
        ha, ta = cl.bf16_split(a)
        assert np.array_equal(ha.astype(np.float64) + ta, a.numpy())
        for b in bs:
            hb, tb = cl.bf16_split(b)
            assert np.array_equal(hb.astype(np.float64) + tb, b.numpy())
            assert (not ta.any() or not tb.any()) and (ta.any() or tb.any())             # tail x tail is zero, one cross term is live
            assert bool(ta.any()) == (cls == "A")
    if case in STREAMK_X3_CASES:
        x, ws = o["fwd"]
        assert cl.exact_ok(x, ws, branches, stride, None, None, o["shift"], o["res_out"], parts=("fwd",))
        assert torch.equal(cl.conv_fwd(x, ws, branches, stride, None, F32), cl.f32(cl.conv_fwd(x, ws, branches, stride)))
    else:
        gz, gx = o["wgrad"]
        ws = [torch.zeros(cout, cin, kh, kw) for kh, kw, _, _ in branches]
        assert cl.exact_ok(gx, ws, branches, stride, gz, parts=("dw",))
        for a, b in zip(cl.conv_dw(gz, gx, ws, branches, stride, None, F32), cl.conv_dw(gz, gx, ws, branches, stride)):
            assert torch.equal(a, cl.f32(b))
