"""The momentum-teacher update (optim.hip: ema_chunks, ema_tensor_sums, ema_finish; ops.EmaPlan) bit for bit.

Reference, on the CPU in plain torch: `slow.mul_(m).add_(fast * (1.0 - m))` in fp32 (oracle.head_ref.momentum_update's line:
three roundings, the factors fl32(m) and fl32(1 - m) with the difference taken in DOUBLE), and for the returned distance
d = slow - fast in fp32, sum_t sqrt(sum(d.double()**2)) in float64, rounded to fp32 once.

Asserted: every slow tensor equals the reference in every BIT (sign of zero included) for m in {0.99, 0.999, 0.5, 0.0, 1.0}; the
distance is within ONE fp32 ulp of the reference (derived: both sides add exact double products, so the order of summation moves
the double by at most n * 2^-53 relative, far below the fp32 rounding); update=False writes nothing, leaves `_version` alone and
returns the distance the following update=True call returns; update=True advances every `_version`; two runs from one state
give the same bits; a NaN / an Inf planted in one `fast` element reaches exactly that slow element and the distance, as in the
reference.  All slow tensors are slices of ONE device buffer, separated by an odd number of sentinel floats (tensors start on
every 4-byte phase); the sentinels, and the fast tensors laid out the same way, are unchanged after every call.

Shapes: 141 tensors (ema_finish walks more than 64) whose sizes cycle through 1, 5, 63, 64, 65, 255, 256, 257, chunk - 1, chunk,
chunk + 1, 2 * chunk with chunk = dasac_ema_chunk_elems(); one tensor of 70 * chunk + 3 elements in the middle (more than 64
chunks: the second stride of ema_tensor_sums); the first and the last tensor have one element.  A second plan has one tensor of
one element.  Inputs are zero (either sign) or normal with |x| >= 1e-30: denormal handling is NOT covered.

Finding of this module: dasac_ema_update took the momentum as a float and formed 1 - fl32(m) (0.0099999905 for m = 0.99) where
the reference multiplies by fl32(1 - m) (0.01); about a quarter of the elements differed in the last bit at m = 0.99 and 0.999.
The ABI now takes a double.  Measured on the MI355X: all tensors bit-equal; distance error 0 ulp for every m (bound 1 ulp);
the oracle's fp32 torch.norm sum lies 3 ulp below (printed by the test, not asserted)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MOMENTA = [0.99, 0.999, 0.5, 0.0, 1.0]
SENTINEL = np.float32(-7.25e8)
N_TENSORS = 141
BIG_AT = 70


def _chunk():
    from dasac_hip import lib as L
    return L.load().dasac_ema_chunk_elems()


def _layout(sizes):
    """(offsets, total, mask): tensor i occupies [offsets[i], offsets[i] + sizes[i]) of a flat buffer; 1, 3, 5 or 7 sentinel floats
    stand before each tensor and after the last."""
    offs, at = [], 0
    for i, n in enumerate(sizes):
        at += (1, 3, 5, 7)[i % 4]
        offs.append(at)
        at += n
    total = at + 3
    mask = np.zeros(total, bool)
    for o, n in zip(offs, sizes):
        mask[o:o + n] = True
    return offs, total, mask


def _sizes():
    c = _chunk()
    cyc = [1, 5, 63, 64, 65, 255, 256, 257, c - 1, c, c + 1, 2 * c]
    sizes = [cyc[i % len(cyc)] for i in range(N_TENSORS)]
    sizes[BIG_AT] = 70 * c + 3
    sizes[0] = sizes[-1] = 1
    return sizes


def _host(sizes, seed):
    """flat fp32 (slow, fast) with sentinels outside the tensors, signed zeros at a few places of every tensor"""
    offs, total, mask = _layout(sizes)
    rng = np.random.RandomState(seed)
    slow = (rng.standard_normal(total) * 0.5).astype(np.float32)
    fast = (slow + rng.standard_normal(total).astype(np.float32) * np.float32(0.05)).astype(np.float32)
    for buf in (slow, fast):
        tiny = np.abs(buf) < 1e-30
        buf[tiny] = np.float32(1e-3)
    zeros = [(0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (-0.0, 1.5), (2.5, -0.0), (0.0, -3.0), (-1.25, 0.0)]
    for t, (o, n) in enumerate(zip(offs, sizes)):
        for j in range(min(n, len(zeros))):
            s, f = zeros[(j + t) % len(zeros)]
            at = o + (j * 97) % n if n >= len(zeros) * 97 else o + j
            slow[at], fast[at] = np.float32(s), np.float32(f)
    slow[~mask] = SENTINEL
    fast[~mask] = SENTINEL
    return offs, mask, slow, fast


def _reference(slow, fast, offs, sizes, m):
    """(updated flat slow, distance rounded to fp32, the oracle's fp32 torch.norm sum); sentinels are left as they are"""
    ts, tf = torch.from_numpy(slow.copy()), torch.from_numpy(fast)
    total64, total32 = 0.0, torch.zeros(())
    for o, n in zip(offs, sizes):
        s, f = ts[o:o + n], tf[o:o + n]
        d = s - f
        total64 = total64 + float(torch.sqrt((d.double() ** 2).sum()))
        total32 = total32 + torch.norm(d)
        s.mul_(m).add_(f * (1.0 - m))
    return ts.numpy(), np.float32(total64), float(total32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class _Device:
    def __init__(self, sizes, offs, slow, fast):
        from dasac_hip import ops
        self.slow, self.fast = torch.from_numpy(slow).cuda(), torch.from_numpy(fast).cuda()
        self.slows = [self.slow[o:o + n] for o, n in zip(offs, sizes)]
        self.fasts = [self.fast[o:o + n] for o, n in zip(offs, sizes)]
        assert len({t.data_ptr() % 16 for t in self.slows}) == 4 or len(sizes) < 8      # every 4-byte phase
        self.plan = ops.EmaPlan(self.fasts, self.slows)

    def reset(self, slow, fast):
        self.slow.copy_(torch.from_numpy(slow))
        self.fast.copy_(torch.from_numpy(fast))

    def run(self, m, update):
        out = self.plan.run(m, update)
        torch.cuda.synchronize()
        return out.cpu().numpy()[0]


def _ulp_err(got, ref32):
    if np.isnan(ref32) or np.isinf(ref32):
        return 0.0 if (np.isnan(got) if np.isnan(ref32) else got == ref32) else float("inf")
    return abs(float(got) - float(ref32)) / float(np.spacing(np.abs(ref32)))


@pytest.fixture(scope="module")
def case():
    sizes = _sizes()
    offs, mask, slow, fast = _host(sizes, 11)
    dev = _Device(sizes, offs, slow, fast)
    assert dev.plan.n_tensors == N_TENSORS > 128 and max(sizes) > 64 * _chunk()
    return sizes, offs, mask, slow, fast, dev


@pytest.mark.parametrize("m", MOMENTA)
def test_update_is_bit_exact_and_touches_nothing_else(case, m):
    sizes, offs, mask, slow, fast, dev = case
    want, d_ref, d_norm32 = _reference(slow, fast, offs, sizes, m)
    assert np.array_equal(_bits(want[~mask]), _bits(slow[~mask]))
    dev.reset(slow, fast)
    versions = [t._version for t in dev.slows]
    # update=False: the distance only
    d0 = dev.run(m, False)
    assert np.array_equal(_bits(dev.slow.cpu().numpy()), _bits(slow)), "update=False wrote a slow tensor or a sentinel"
    assert [t._version for t in dev.slows] == versions
    # update=True
    d1 = dev.run(m, True)
    got = dev.slow.cpu().numpy()
    err = _ulp_err(d1, d_ref)
    print("ema m={}: distance {!r} ref {!r} ({:.2f} ulp, bound 1); oracle fp32 norm sum {!r} ({:+.2f} ulp from got)".format(
        m, float(d1), float(d_ref), err, d_norm32, (float(d1) - d_norm32) / float(np.spacing(d_ref))))
    assert _bits(np.float32(d0)) == _bits(np.float32(d1)), "update=False returned another distance"
    assert err <= 1.0, (m, float(d1), float(d_ref))
    assert np.array_equal(_bits(got[~mask]), _bits(slow[~mask])), "a sentinel between the slow tensors changed"
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (m, bad.size, bad[:4], got[bad[:4]], want[bad[:4]])
    assert np.array_equal(_bits(dev.fast.cpu().numpy()), _bits(fast)), "the fast buffer changed"
    assert all(t._version > v for t, v in zip(dev.slows, versions))
    for t, o, n in zip(dev.slows, offs, sizes):                    # per tensor, as the issue states it
        assert torch.equal(t.cpu(), torch.from_numpy(want[o:o + n]))
    # a second run from the same state: the same bits
    dev.reset(slow, fast)
    d2 = dev.run(m, True)
    assert _bits(np.float32(d2)) == _bits(np.float32(d1))
    assert np.array_equal(_bits(dev.slow.cpu().numpy()), _bits(got))


@pytest.mark.parametrize("what", ["nan", "inf"])
def test_non_finite_fast_element_reaches_its_element_and_the_distance(case, what):
    sizes, offs, mask, slow, fast, dev = case
    m = 0.99
    fast = fast.copy()
    at = offs[BIG_AT] + 65 * _chunk() + 1                        # inside the big tensor, in a chunk of the second stride
    fast[at] = np.float32(np.nan if what == "nan" else np.inf)
    want, d_ref, _ = _reference(slow, fast, offs, sizes, m)
    assert (np.isnan(want[at]) and np.isnan(d_ref)) if what == "nan" else (np.isposinf(want[at]) and np.isposinf(d_ref))
    dev.reset(slow, fast)
    d0 = dev.run(m, False)
    d1 = dev.run(m, True)
    got = dev.slow.cpu().numpy()
    for d in (d0, d1):
        assert np.isnan(d) if what == "nan" else d == d_ref
    assert np.isnan(got[at]) if what == "nan" else got[at] == want[at]
    others = np.ones(got.shape[0], bool)
    others[at] = False
    assert np.array_equal(_bits(got[others]), _bits(want[others]))
    assert not np.isnan(got[others]).any()


def test_single_element_plan():
    sizes = [1]
    for m in MOMENTA:
        offs, mask, slow, fast = _host(sizes, 5)
        slow[offs[0]], fast[offs[0]] = np.float32(0.3), np.float32(-1.7)
        dev = _Device(sizes, offs, slow, fast)
        want, d_ref, _ = _reference(slow, fast, offs, sizes, m)
        d0, d1 = dev.run(m, False), dev.run(m, True)
        assert _bits(np.float32(d0)) == _bits(np.float32(d1)) and _ulp_err(d1, d_ref) <= 1.0
        assert np.array_equal(_bits(dev.slow.cpu().numpy()), _bits(want))
        assert np.array_equal(_bits(dev.fast.cpu().numpy()), _bits(fast))


def test_reference_restatement_on_the_cpu():
    """The reference line equals round(round(sl * fl32(m)) + round(f * fl32(1 - m))) evaluated through float64 (each fp32 product
    of two fp32 numbers is exact in double, so rounding it to fp32 is one rounding), with 1 - m taken in double -- and differs
    from the same with 1 - fl32(m) for m = 0.99 and 0.999: the distinction the kernel test rests on."""
    rng = np.random.RandomState(3)
    s, f = rng.standard_normal(20000).astype(np.float32), rng.standard_normal(20000).astype(np.float32)
    for m in MOMENTA:
        ref = torch.from_numpy(s.copy()).mul_(m).add_(torch.from_numpy(f) * (1.0 - m)).numpy()
        a = (s.astype(np.float64) * float(np.float32(m))).astype(np.float32)
        b = (f.astype(np.float64) * float(np.float32(1.0 - m))).astype(np.float32)
        assert np.array_equal(_bits(ref), _bits((a.astype(np.float64) + b.astype(np.float64)).astype(np.float32)))
        b_wrong = (f.astype(np.float64) * float(np.float32(1.0 - float(np.float32(m))))).astype(np.float32)
        wrong = (a.astype(np.float64) + b_wrong.astype(np.float64)).astype(np.float32)
        assert np.array_equal(_bits(ref), _bits(wrong)) == (m in (0.5, 0.0, 1.0))
