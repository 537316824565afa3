"""tests/guarded_operands.py on CPU tensors: bodies land on the requested phases for every item size, a byte written just outside
a body is reported with its side and offset, a modified input is reported, the torch stand-in forwards everything it does not
allocate, and its allocating functions honour shape, dtype, device and fill in both calling styles."""
import pytest
import torch

from exact_workspace import BACK, FRONT, GUARD
from guarded_operands import ALIGN, FILL, PLAIN_FILL, Arena, bits_equal, body_ptr

CPU = torch.device("cpu")


@pytest.mark.parametrize("phase", range(4))
@pytest.mark.parametrize("dtype", [torch.float32, torch.int32, torch.int64, torch.float64, torch.uint8, torch.bool])
def test_bodies_land_on_the_requested_phases(phase, dtype):
    arena = Arena(phase)
    item = torch.empty(0, dtype=dtype).element_size()
    src = torch.arange(1, 38).to(dtype)
    for k in range(18):                       # more than the 16 phases of a byte tensor: the phases wrap
        t = arena.place(src) if k % 2 else arena.torch.empty(37, dtype=dtype)
        assert body_ptr(t) % 16 == ((phase + k) % (16 // item)) * item
        assert t.dtype == dtype and tuple(t.shape) == (37,) and t.is_contiguous()
        assert torch.equal(t, src) if k % 2 else bool((t.view(torch.uint8) == FILL).all())
        e = arena.entries[-1]
        assert e.off >= FRONT and e.whole.numel() - e.off - e.nbytes >= BACK and e.nbytes == 37 * item
        assert body_ptr(t) == body_ptr(e.whole) + e.off
        assert bool((e.whole[:e.off] == GUARD).all()) and bool((e.whole[e.off + e.nbytes:] == GUARD).all())
    assert arena.check() == 18


def test_fp32_phases_cover_all_four_and_uint8_all_sixteen_over_the_base_phases():
    seen = {torch.float32: set(), torch.uint8: set(), torch.int64: set()}
    for phase in range(16):
        arena = Arena(phase)
        for dtype in seen:
            seen[dtype].add(body_ptr(arena.torch.empty(3, dtype=dtype)) % 16)
    assert seen[torch.float32] == {0, 4, 8, 12} and seen[torch.int64] == {0, 8} and seen[torch.uint8] == set(range(16))


def test_descriptor_tables_stay_aligned_and_take_no_phase():
    arena = Arena(1)
    table = arena.torch.empty((128, 4), dtype=torch.int32)          # a conv gather table
    words = arena.torch.empty(40, dtype=torch.int32)                # ReLU bit words: an operand
    chunks = arena.torch.zeros(5, 2, dtype=torch.int32)
    after = arena.torch.empty(3, dtype=torch.float32)
    assert body_ptr(table) % ALIGN == 0 and body_ptr(chunks) % ALIGN == 0
    assert body_ptr(words) % 16 == 4 and body_ptr(after) % 16 == 8
    arena.entries[0].whole[arena.entries[0].off - 1] = 0            # descriptors are guarded like everything else
    with pytest.raises(AssertionError, match=r"front guard changed at body offset -1 "):
        arena.check()


def test_a_byte_written_just_before_a_body_is_reported():
    arena = Arena(2)
    arena.place(torch.zeros(5))
    arena.place(torch.zeros(3, 7), name="logits")
    e = arena.entries[1]
    e.whole[e.off - 1] = 0
    with pytest.raises(AssertionError, match=r"tensor logits \(84 bytes, phase 12\): front guard changed at body offset -1 \(1 bytes"):
        arena.check()


def test_a_byte_written_just_after_a_body_is_reported():
    arena = Arena(0)
    out = arena.torch.empty((3, 7), dtype=torch.float32)
    out.fill_(1.0)                                                   # the body is the caller's
    assert arena.check() == 1
    e = arena.entries[0]
    e.whole[e.off + e.nbytes] = 0
    e.whole[e.off + e.nbytes + 9] = 1
    with pytest.raises(AssertionError, match=r"float32\[3, 7\]#0 \(84 bytes, phase 0\): back guard changed at body offset 84 \(2 bytes"):
        arena.check()


def test_a_modified_input_is_reported_unless_declared_in_place():
    arena = Arena(3)
    x = arena.place(torch.arange(12, dtype=torch.int64), name="labels")
    y = arena.place(torch.arange(12, dtype=torch.int64), name="written", inplace=True)
    y[3] = -1
    assert arena.check() == 2
    x[5] = 255
    with pytest.raises(AssertionError, match=r"input labels \(96 bytes\) was modified: first at byte 40 \(1 bytes"):
        arena.check()
    plain = Arena(None)
    z = plain.place(torch.ones(4), name="plain input")
    z[1] = float("nan")
    with pytest.raises(AssertionError, match="input plain input"):
        plain.check()


def test_the_stand_in_forwards_everything_else_untouched():
    proxy = Arena(0).torch
    for name in ("float32", "int64", "uint8", "Tensor", "cat", "tensor", "from_numpy", "autograd", "cuda", "no_grad", "contiguous_format",
                 "is_tensor", "distributed"):
        assert getattr(proxy, name) is getattr(torch, name), name
    assert torch.equal(proxy.cat([proxy.tensor([1.0]), proxy.tensor([2.0])]), torch.tensor([1.0, 2.0]))
    with pytest.raises(AttributeError):
        proxy.no_such_attribute
    with pytest.raises(AttributeError):
        proxy.empty = None


@pytest.mark.parametrize("phase", [None, 1])
def test_allocators_honour_shape_dtype_device_and_fill_in_both_calling_styles(phase):
    arena = Arena(phase)
    t, fill = arena.torch, (PLAIN_FILL if phase is None else FILL)
    for made in (t.empty(2, 3), t.empty((2, 3)), t.empty(torch.Size((2, 3)), dtype=torch.float32, device=CPU), t.empty([2, 3], device="cpu")):
        assert tuple(made.shape) == (2, 3) and made.dtype == torch.float32 and made.device == CPU
        assert bool((made.view(torch.uint8) == fill).all())
    assert t.empty(5, dtype=torch.int64).dtype == torch.int64 and t.empty((), dtype=torch.int64).shape == ()
    assert t.empty(0, dtype=torch.float64).numel() == 0 and t.empty((2, 0, 3)).shape == (2, 0, 3)
    for made in (t.zeros(2, 3, dtype=torch.float64), t.zeros((2, 3), dtype=torch.float64)):
        assert tuple(made.shape) == (2, 3) and made.dtype == torch.float64 and bool((made == 0).all())
    assert t.zeros((), dtype=torch.int64).shape == () and int(t.zeros((), dtype=torch.int64)) == 0
    for made in (t.ones(4, dtype=torch.uint8), t.ones((4,), dtype=torch.uint8)):
        assert tuple(made.shape) == (4,) and made.dtype == torch.uint8 and bool((made == 1).all())
    f = t.full((2, 2), 255, dtype=torch.uint8)
    assert f.dtype == torch.uint8 and bool((f == 255).all())
    assert t.full((3,), 7).dtype == torch.int64 and t.full((3,), 0.5).dtype == torch.float32 and t.full((3,), True).dtype == torch.bool
    assert bool((t.full((3,), 0.5) == 0.5).all())
    like = torch.arange(6, dtype=torch.int64).view(2, 3)
    e = t.empty_like(like)
    assert e.shape == like.shape and e.dtype == torch.int64 and bool((e.view(torch.uint8) == fill).all())
    assert t.empty_like(like, dtype=torch.float32, memory_format=torch.contiguous_format).dtype == torch.float32
    assert t.empty_like(like.t(), memory_format=torch.contiguous_format).is_contiguous()
    z = t.zeros_like(like, memory_format=torch.contiguous_format)
    assert z.shape == like.shape and z.dtype == torch.int64 and bool((z == 0).all())
    with pytest.raises(AssertionError):
        t.empty(2, layout=torch.strided)                   # an unknown keyword is refused, not dropped
    assert arena.check() == len(arena.entries)


def test_the_plain_arena_allocates_plainly_and_fills_differently():
    plain = Arena(None)
    a = plain.torch.empty(7, dtype=torch.float32)
    b = plain.place(torch.arange(7.0))
    assert FILL != PLAIN_FILL != GUARD != FILL
    assert bool((a.view(torch.uint8) == PLAIN_FILL).all()) and torch.equal(b, torch.arange(7.0))
    assert a.untyped_storage().nbytes() == 28 and plain.entries[0].whole is None
    assert plain.check() == 2


def test_an_arena_knows_its_own_tensors():
    for arena in (Arena(2), Arena(None)):
        a, b = arena.place(torch.arange(6.0).view(2, 3)), arena.torch.zeros(4, dtype=torch.int64)
        assert arena.owns(a) and arena.owns(a[1]) and arena.owns(b[:2]) and arena.owns(a.detach())
        assert not arena.owns(torch.zeros(3)) and not arena.owns(a.clone())


def test_bits_equal_is_bitwise():
    nan = torch.tensor([float("nan"), 1.0])
    assert bits_equal(nan, nan.clone()) and not torch.equal(nan, nan.clone())
    assert not bits_equal(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert bits_equal(None, None) and not bits_equal(None, nan)
    assert not bits_equal(torch.zeros(2), torch.zeros(2, dtype=torch.float64)) and not bits_equal(torch.zeros(2), torch.zeros(1, 2))
    assert bits_equal(torch.arange(6).view(2, 3).t(), torch.arange(6).view(2, 3).t().contiguous())
