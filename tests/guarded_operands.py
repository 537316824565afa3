"""Operands between guard bands, at a chosen alignment phase (a helper, not a conftest; the sibling of exact_workspace.py, which
does the same for workspaces).

An `Arena(phase)` gives every tensor it places or allocates one fresh uint8 allocation
    [ front guard 4096 B | body | back guard >= 1 MiB ]
whose body starts at a byte address congruent to ((phase + k) % (16 // itemsize)) * itemsize modulo 16, k = the number of
phased tensors placed before it: the operands of one call sit at different phases, fp32 at 4 of them, int64 / fp64 at 2, uint8 and
bool at all 16.  Both guards hold 0xA5 and are those of exact_workspace.py, so a write that misses its tensor by less than 4 KiB
in front or 1 MiB behind lands inside a live allocation: an overrun is detected, never provoked.

Two ways in:
  * `arena.place(t)` copies a (host) tensor into such a body and keeps a copy of what it put there;
  * `arena.torch` stands in for the name `torch` inside a wrapper module (monkeypatch.setattr(ops, "torch", arena.torch)): its
    `empty`, `empty_like`, `zeros`, `zeros_like`, `full` and `ones` allocate bodies -- `empty*` pre-filled with the byte
    `arena.fill`, the others with what was asked for -- and every other attribute is torch's own.
int32 tensors of two dimensions are DESCRIPTOR tables (conv gather tables [Kpad, 4], chunk lists [n, 2]): include/dasac_hip.h asks
16 / 8 bytes for them, so they get guards but stay on a 256-byte boundary.  One-dimensional int32 tensors (ReLU bit words) are
operands and get phases.

`arena.check()` synchronises, then asserts that no guard byte changed and that every placed input still holds its copy (inputs
placed with inplace=True, which the header declares written, are exempt).

`Arena(None)` is the plain comparand: ordinary allocations at the allocator's own alignment, no guards, `empty*` pre-filled with a
DIFFERENT byte -- an element that no run writes differs between a plain and a guarded run."""
import torch

from exact_workspace import BACK, FRONT, GUARD

ALIGN = 256                 # descriptor tables and the plain arena's notion of "aligned"
FILL = 0x5C                 # guarded runs: fp32 2.48e17, int64 0x5C5C..., uint8 92
PLAIN_FILL = 0x3A           # the plain run: fp32 7.1e-4


def body_ptr(t):
    """Address of a tensor's first byte (data_ptr() is 0 for every empty tensor; this is where it lies)."""
    return t.untyped_storage().data_ptr() + t.storage_offset() * t.element_size()


def is_descriptor(shape, dtype):
    return dtype == torch.int32 and len(shape) == 2


def _shape(size):
    if len(size) == 1 and not isinstance(size[0], int):
        size = tuple(size[0])
    return tuple(int(v) for v in size)


class _Entry:
    __slots__ = ("name", "whole", "off", "nbytes", "body", "copy")

    def __init__(self, name, whole, off, nbytes, body, copy):
        self.name, self.whole, self.off, self.nbytes, self.body, self.copy = name, whole, off, nbytes, body, copy


class Arena:
    def __init__(self, phase, fill=None):
        self.phase = None if phase is None else int(phase)
        self.fill = int((PLAIN_FILL if phase is None else FILL) if fill is None else fill)
        self.entries = []
        self.placed = 0               # k: phased tensors so far
        self.torch = _TorchProxy(self)

    # ---- allocation ------------------------------------------------------------------------------------------------------------
    def _body(self, shape, dtype, device, name, descriptor=False):
        shape = tuple(int(v) for v in shape)
        item = torch.empty(0, dtype=dtype).element_size()
        numel = 1
        for v in shape:
            numel *= v
        nbytes = numel * item
        if self.phase is None:
            body = torch.empty(shape, dtype=dtype, device=device)
            self.entries.append(_Entry(name, None, 0, nbytes, body, None))
            return body
        if descriptor:
            unit, want = ALIGN, 0
        else:
            unit, want = 16, ((self.phase + self.placed) % (16 // item)) * item
            self.placed += 1
        whole = torch.empty(FRONT + nbytes + BACK + unit, dtype=torch.uint8, device=device)
        off = FRONT + (want - (body_ptr(whole) + FRONT)) % unit
        whole.fill_(GUARD)
        flat = whole[off:off + nbytes]
        body = (flat if dtype == torch.uint8 else flat.view(dtype)).view(shape)
        self.entries.append(_Entry(name, whole, off, nbytes, body, None))
        return body

    def alloc(self, shape, dtype=None, device=None, value=None, name=None):
        """A body of `shape`: filled with `value`, or with the byte `fill` when value is None."""
        dtype = torch.get_default_dtype() if dtype is None else dtype
        shape = tuple(shape)
        name = name or "{}{}#{}".format(str(dtype).replace("torch.", ""), list(shape), len(self.entries))
        body = self._body(shape, dtype, device, name, is_descriptor(shape, dtype))
        if value is None:
            if body.numel():
                body.view(-1).view(torch.uint8).fill_(self.fill)
        else:
            body.fill_(value)
        return body

    def place(self, t, name=None, inplace=False):
        """A device tensor equal to `t` (made contiguous) in a body of its own; the arena keeps a copy unless `inplace` says that
        the header declares the operand written."""
        device = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
        t = t.detach().contiguous()
        name = name or "placed {}{}#{}".format(str(t.dtype).replace("torch.", ""), list(t.shape), len(self.entries))
        body = self._body(t.shape, t.dtype, device, name)
        body.copy_(t)
        if not inplace:
            self.entries[-1].copy = t.to(device).clone()
        return body

    def owns(self, t):
        """True when `t` (or the tensor it is a view of) lies in an allocation of this arena."""
        base = t.untyped_storage().data_ptr()
        return any((e.body if e.whole is None else e.whole).untyped_storage().data_ptr() == base for e in self.entries)

    # ---- checks ----------------------------------------------------------------------------------------------------------------
    def check(self):
        """Asserts that no guard byte of any tensor changed and that every input still equals its copy; returns the number of
        tensors."""
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        for e in self.entries:
            if e.whole is not None:
                for side, lo, hi in (("front", 0, e.off), ("back", e.off + e.nbytes, e.whole.numel())):
                    bad = (e.whole[lo:hi] != GUARD).nonzero()
                    if bad.numel():
                        first = lo + int(bad[0]) - e.off          # relative to the body's first byte
                        raise AssertionError("tensor {} ({} bytes, phase {}): {} guard changed at body offset {} ({} bytes in all)".format(
                            e.name, e.nbytes, (body_ptr(e.whole) + e.off) % 16, side, first, bad.numel()))
            if e.copy is not None and e.nbytes:
                now, was = e.body.reshape(-1).view(torch.uint8), e.copy.reshape(-1).view(torch.uint8)
                bad = (now != was).nonzero()
                if bad.numel():
                    raise AssertionError("input {} ({} bytes) was modified: first at byte {} ({} bytes in all)".format(
                        e.name, e.nbytes, int(bad[0]), bad.numel()))
        return len(self.entries)


class _TorchProxy:
    """`torch` with the six allocating functions of the wrapper modules routed into an arena."""

    def __init__(self, arena):
        object.__setattr__(self, "_arena", arena)

    def __getattr__(self, name):
        return getattr(torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("the torch stand-in is read-only")

    @staticmethod
    def _opts(kw, like=None):
        dtype = kw.pop("dtype", None)
        device = kw.pop("device", None)
        fmt = kw.pop("memory_format", None)
        assert fmt in (None, torch.contiguous_format, torch.preserve_format), fmt
        assert not kw.pop("requires_grad", False) and not kw.pop("pin_memory", False)
        assert not kw, "the torch stand-in does not know the keywords {}".format(sorted(kw))
        if like is not None:
            dtype = like.dtype if dtype is None else dtype
            device = like.device if device is None else device
            assert fmt == torch.contiguous_format or like.is_contiguous(), "empty_like of a strided tensor keeps its strides"
        return dtype, (torch.device(device) if device is not None else torch.device("cpu"))

    def empty(self, *size, **kw):
        if kw.get("pin_memory"):                     # a host staging buffer, not an operand
            return torch.empty(*size, **kw)
        dtype, device = self._opts(kw)
        return self._arena.alloc(_shape(size), dtype, device)

    def zeros(self, *size, **kw):
        dtype, device = self._opts(kw)
        return self._arena.alloc(_shape(size), dtype, device, 0)

    def ones(self, *size, **kw):
        dtype, device = self._opts(kw)
        return self._arena.alloc(_shape(size), dtype, device, 1)

    def full(self, size, fill_value, **kw):
        dtype, device = self._opts(kw)
        if dtype is None:
            dtype = torch.bool if isinstance(fill_value, bool) else torch.int64 if isinstance(fill_value, int) else torch.get_default_dtype()
        return self._arena.alloc(_shape((size,)), dtype, device, fill_value)

    def empty_like(self, t, **kw):
        dtype, device = self._opts(kw, t)
        return self._arena.alloc(t.shape, dtype, device)

    def zeros_like(self, t, **kw):
        dtype, device = self._opts(kw, t)
        return self._arena.alloc(t.shape, dtype, device, 0)


def bits_equal(a, b):
    """Bit for bit (NaN equals NaN, -0.0 differs from 0.0): shapes, dtypes and the bytes."""
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.numel() == 0:
        return True
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))
