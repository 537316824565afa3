"""The batched tile-per-block launch of the conv GEMM (dasac_conv_gemm_batched: the 16 point GEMMs of a Winograd convolution as one
grid): bit-equal to one `conv_gemm(..., schedule=1)` call per entry, confined to its own entry when the per-batch strides leave gaps,
refused by the host checks without a launch, and what `ops.winograd_conv` issues by default."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# (batch, C, M, T): the GEMM of a 1x1 convolution over C planes of 1 x T pixels, as the Winograd path issues it
CASES = [
    (16, 32, 128, 130),     # two pixel tiles, the second with 2 live columns
    (3, 16, 136, 129),      # padded M = 256: ragged M, a ragged last row group
    (2, 48, 128, 1000),     # T no multiple of 128, three K-steps
    (1, 32, 128, 256),      # batch 1, exact tiles
    (16, 32, 128, 8),       # fewer pixels than one tile
]
IDS = ["b{}_c{}_m{}_t{}".format(*c) for c in CASES]
SENTINEL = -12345.0


def _dev():
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _case(case):
    """Operands of one case and the reference: one tile-per-block conv_gemm launch per entry.  Computed once, read-only."""
    from dasac_hip import ops
    from dasac_hip import lib as L
    B, C, M, T = case
    lib = L.load()
    g = torch.Generator(device="cpu").manual_seed(B * 1000003 + C * 1009 + M * 31 + T)
    x = torch.randn(B, 1, C, 1, T, generator=g).to(_dev())
    packed = torch.randn(B, lib.dasac_conv_kpad(C), lib.dasac_conv_mpad(M), generator=g).to(_dev())
    table = ops._winograd_table(C, T, _dev())
    ref = torch.full((B, 1, M, 1, T), SENTINEL, device=_dev())
    for b in range(B):
        ops.conv_gemm(x[b], packed[b], table, ref[b], (1, T), 1, M, C, schedule=1)
    torch.cuda.synchronize()
    return x, packed, table, ref


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_batched_launch_equals_one_tile_per_block_launch_per_entry_bit_for_bit(case):
    from dasac_hip import ops
    B, C, M, T = case
    x, packed, table, ref = _case(case)
    out = torch.full_like(ref, SENTINEL)
    ops.conv_gemm_batched(x, packed, table, out, (1, T), 1, M, C)
    assert not bool((ref == SENTINEL).any()), "the reference left an element unwritten"
    assert torch.equal(_bits(out), _bits(ref))


@pytest.mark.parametrize("case", CASES[:3], ids=IDS[:3])
def test_padded_strides_read_and_write_nothing_outside_an_entry(case):
    """Entries of x and packed lie apart with NaN between them, entries of out with a sentinel between them: the outputs equal the
    contiguous case bit for bit and every gap element of out still holds the sentinel."""
    from dasac_hip import ops
    B, C, M, T = case
    x, packed, table, ref = _case(case)
    gx, gw, go = 36, 8, 20                                    # gaps in elements (strides stay multiples of 4)
    nx, nw, no = C * T, packed[0].numel(), M * T
    xb = torch.full((B, nx + gx), float("nan"), device=_dev())
    wb = torch.full((B, nw + gw), float("nan"), device=_dev())
    ob = torch.full((B, no + go), SENTINEL, device=_dev())
    xb[:, :nx] = x.reshape(B, nx)
    wb[:, :nw] = packed.reshape(B, nw)
    xs, ws, os_ = xb[:, :nx].view(B, 1, C, 1, T), wb[:, :nw].view(packed.shape), ob[:, :no].view(B, 1, M, 1, T)
    assert xs.stride(0) == nx + gx and os_.stride(0) == no + go and ws.stride(0) == nw + gw
    ops.conv_gemm_batched(xs, ws, table, os_, (1, T), 1, M, C)
    assert torch.equal(_bits(ob[:, :no]), _bits(ref.reshape(B, no)))
    assert bool((ob[:, no:] == SENTINEL).all())


def test_batch_of_one_with_zero_strides_is_the_single_launch():
    from dasac_hip import ops
    case = CASES[3]
    B, C, M, T = case
    x, packed, table, ref = _case(case)
    out = torch.full_like(ref, SENTINEL)
    ops.conv_gemm_batched(x, packed, table, out, (1, T), 1, M, C, strides=(0, 0, 0))
    assert torch.equal(_bits(out), _bits(ref))


def test_host_checks_refuse_without_launching():
    from dasac_hip import ops, DasacError
    dev = _dev()
    T = 130

    def operands(B, C, M):
        from dasac_hip import lib as L
        lib = L.load()
        x = torch.ones(max(B, 1), 1, C, 1, T, device=dev)[:B]
        packed = torch.ones(max(B, 1), lib.dasac_conv_kpad(C), lib.dasac_conv_mpad(M), device=dev)[:B]
        out = torch.full((max(B, 1), 1, M, 1, T), SENTINEL, device=dev)
        return x, packed, ops._winograd_table(C if C % 16 == 0 else 16, T, dev), out

    def refused(match, B, C, M, exc=DasacError, **kw):
        x, packed, table, out = operands(B, C, M)
        with pytest.raises(exc, match=match):
            ops.conv_gemm_batched(x, packed, table, out[:B], (1, T), 1, M, C, **kw)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), "a refused call wrote to its output"

    refused("batch 0", 0, 32, 128)                                                        # a batch of 0
    refused("multiple of 16", 2, 24, 128)                                                 # C % 16 != 0
    refused("128-row tile", 2, 32, 40)                                                    # a padded M of 64
    refused("smaller than one entry", 2, 32, 128, strides=(32 * T - 4, 128 * 128, 128 * T))
    refused("smaller than one entry", 2, 32, 128, strides=(32 * T, 128 * 128, 128 * T - 4))
    refused("multiples of 4", 2, 32, 128, strides=(32 * T + 2, 128 * 128, 128 * T))
    # no epilogue operand exists in the batched form: the binding has no parameter to take one
    ones = torch.ones(128, device=dev)
    for kw in ({"shift": ones}, {"res": ones}, {"mask": ones}, {"relu": True}, {"bits_out": ones}, {"stats": ones}):
        refused("unexpected keyword", 2, 32, 128, exc=TypeError, **kw)


def test_winograd_conv_issues_one_batched_launch_and_equals_sixteen_launches():
    from dasac_hip import ops
    N, C, M, H, W, d = 2, 32, 128, 9, 7, 4
    dev = _dev()
    g = torch.Generator(device="cpu").manual_seed(7)
    x = torch.randn(N, C, H, W, generator=g).to(dev)
    w = (torch.randn(M, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5).to(dev)
    shift = torch.randn(M, generator=g).to(dev)
    u = ops.winograd_filter(ops.ConvSpec(C, M, [(3, 3, d, d)]), w, False)
    each = ops.winograd_conv(x, u, torch.empty(N, M, H, W, device=dev), d, shift, True, gemm_schedule=1).clone()
    torch.cuda.synchronize()
    ops.PROFILE.start()
    one = ops.winograd_conv(x, u, torch.empty(N, M, H, W, device=dev), d, shift, True, gemm_schedule="auto")
    prof = ops.PROFILE.stop()
    assert torch.equal(_bits(one), _bits(each))
    gemms = {k: v["launches"] for k, v in prof.items() if k.startswith("conv_gemm")}
    assert gemms == {"conv_gemm<batched>": 1}, gemms
