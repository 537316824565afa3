"""dasac_dropout_planes (pointwise.hip: philox4x32_10, dropout_planes) as a known-answer test: the keep mask of every plane is
PREDICTED from Philox4x32-10 of (seed, offset, plane), computed by tests/philox_ref.py from the published definition (itself
held to the Random123 vectors by test_philox_ref_cpu.py), under the contract of include/dasac_hip.h:
    counter = (plane, 0, offset low word, offset high word), key = (seed low word, seed high word),
    k = first output word >> 8,  kept iff k / 2^24 >= p,  kept value 1/(1-p) in fp32, dropped value +0.
k / 2^24 and p are both exact in double, so the predicted compare is the kernel's fp32 compare exactly.

Cases: three (seed, offset) pairs (zero; both high words set; all-ones seed) x p in {0, 2^-24, 0.1, 0.5, 0.9, 1 - 2^-24} over
4099 planes; for 16 planes with k spread over [0, 2^24) a launch at p = k/2^24 (kept) and at (k+1)/2^24 (dropped), which pins the
shift and the scale of the uniform and not only the generator; n in {1, 255, 256, 257} into NaN-fenced buffers; the host refuses
p = 1, p < 0 and n = 0; ops.dropout_planes equals the C ABI call with the generator's (seed, offset) and advances the offset by
4 * ceil(n / 4).  The second counter word (planes >= 2^32) is out of reach of a test and NOT covered.

Everything here is an equality: there is no tolerance and so no ratio to record.  On the MI355X all masks and values matched;
the kept fractions over the 4099 planes (printed by the test) lie within 0.012 of 1 - p for every (seed, offset)."""
import numpy as np
import pytest
import torch

import philox_ref as P

pytestmark = pytest.mark.gpu

N = 4099
PAIRS = [(0, 0), (0x9E3779B97F4A7C15, 0x100000004), (0xFFFFFFFFFFFFFFFF, 12)]
PS = [0.0, 2.0 ** -24, 0.1, 0.5, 0.9, 1.0 - 2.0 ** -24]
EINVAL = -1


def _launch(seed, offset, p, n, fence=8):
    """Raw C ABI call into a NaN-filled buffer of n + fence floats; returns (code, host fp32 array of n + fence)."""
    from dasac_hip import lib as L
    lib = L.load()
    buf = torch.full((max(n, 0) + fence,), float("nan"), dtype=torch.float32, device="cuda")
    code = lib.dasac_dropout_planes(seed, offset, float(p), n, buf.data_ptr(), L.stream_ptr())
    torch.cuda.synchronize()
    return code, buf.cpu().numpy()


def _predict(k, p):
    """(keep mask, expected fp32 values) for the 24-bit integers k at probability p (p is rounded to fp32 as the ABI takes it)."""
    p32 = np.float32(p)
    keep = k.astype(np.float64) / 2.0 ** 24 >= float(p32)
    scale = np.float32(1.0) / (np.float32(1.0) - p32)
    return keep, np.where(keep, scale, np.float32(0.0)).astype(np.float32)


def _assert_planes(got, k, p, what):
    n = k.shape[0]
    keep, want = _predict(k, p)
    assert np.isnan(got[n:]).all(), (what, "wrote behind the planes")
    assert not np.isnan(got[:n]).any(), (what, "left a plane unwritten")
    assert np.array_equal(got[:n] != 0, keep), (what, "keep mask", int(((got[:n] != 0) != keep).sum()))
    assert np.array_equal(got[:n].view(np.uint32), want.view(np.uint32)), (what, "values")      # bits: 1/(1-p), and +0 not -0
    return keep


@pytest.mark.parametrize("seed,offset", PAIRS)
def test_mask_is_philox4x32_10_of_seed_offset_plane(seed, offset):
    k = P.uniform24(N, seed, offset)
    assert k.min() >= 0 and k.max() < 1 << 24
    for p in PS:
        code, got = _launch(seed, offset, p, N)
        assert code == 0
        keep = _assert_planes(got, k, p, (hex(seed), hex(offset), p))
        print("dropout seed {:#x} offset {:#x} p {:.8g}: kept {:.4f} of {}".format(seed, offset, p, keep.mean(), N))
        if p == 0.0:
            assert keep.all() and (got[:N] == 1.0).all()
    # different (seed, offset) give different masks (the prediction is not degenerate)
    assert not np.array_equal(k, P.uniform24(N, seed ^ 1, offset)) and not np.array_equal(k, P.uniform24(N, seed, offset + 4))


@pytest.mark.parametrize("seed,offset", PAIRS[:2])
def test_threshold_sits_exactly_at_k_over_2_to_24(seed, offset):
    k = P.uniform24(N, seed, offset)
    order = np.argsort(k, kind="stable")
    order = order[k[order] < (1 << 24) - 1]                      # (k + 1) / 2^24 must stay below 1
    picks = order[np.linspace(0, order.shape[0] - 1, 16).astype(np.int64)]
    assert len(set(int(k[i]) >> 20 for i in picks)) >= 12        # spread over the range
    for i in picks:
        ki = int(k[i])
        for kk, kept in ((ki, True), (ki + 1, False)):
            p = kk / 2.0 ** 24                                    # exact in fp32
            assert float(np.float32(p)) == p
            code, got = _launch(seed, offset, p, N)
            assert code == 0
            _assert_planes(got, k, p, (hex(seed), int(i), kk))
            assert (got[i] != 0) == kept, (int(i), ki, kk)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_block_edges_into_fenced_buffers(n):
    seed, offset = PAIRS[1]
    k = P.uniform24(n, seed, offset)
    for p in (0.0, 0.5):
        code, got = _launch(seed, offset, p, n)
        assert code == 0 and got.shape[0] == n + 8
        _assert_planes(got, k, p, (n, p))


def test_host_refuses_bad_arguments_before_any_launch():
    from dasac_hip import lib as L
    for p, n in ((1.0, 16), (-0.25, 16), (float("nan"), 16), (0.5, 0), (0.5, -3)):
        code, got = _launch(1, 0, p, n, fence=16)
        assert code == EINVAL, (p, n, code)
        assert np.isnan(got).all()
    assert L.load().dasac_dropout_planes(1, 0, 0.5, 16, None, L.stream_ptr()) == EINVAL


def test_ops_wrapper_draws_from_the_generator_state_and_advances_it():
    from dasac_hip import ops
    dev = torch.device("cuda", torch.cuda.current_device())
    gen = torch.cuda.default_generators[dev.index]
    state = gen.get_state()
    try:
        gen.manual_seed(0x1234567887654321)
        gen.set_offset(40)
        B, Cn, p = 3, 7, 0.3                                      # n = 21: not a multiple of 4
        seed, offset = gen.initial_seed(), gen.get_offset()
        got = ops.dropout_planes(B, Cn, p, dev)
        assert gen.get_offset() == offset + 4 * ((B * Cn + 3) // 4) == offset + 24
        code, raw = _launch(seed & 0xFFFFFFFFFFFFFFFF, offset, p, B * Cn)
        assert code == 0 and got.shape == (B, Cn)
        assert np.array_equal(got.cpu().numpy().reshape(-1).view(np.uint32), raw[:B * Cn].view(np.uint32))
        _assert_planes(raw, P.uniform24(B * Cn, seed & 0xFFFFFFFFFFFFFFFF, offset), p, "ops")
        again = ops.dropout_planes(B, Cn, p, dev)                 # the next call draws at the advanced offset
        code, raw2 = _launch(seed & 0xFFFFFFFFFFFFFFFF, offset + 24, p, B * Cn)
        assert np.array_equal(again.cpu().numpy().reshape(-1).view(np.uint32), raw2[:B * Cn].view(np.uint32))
    finally:
        gen.set_state(state)
