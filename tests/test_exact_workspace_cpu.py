"""tests/exact_workspace.py on CPU tensors: the guards report a write on either side of the body with its offset, the fills
are the stated ones, and a request for nothing works."""
import pytest
import torch

from exact_workspace import ALIGN, BACK, FRONT, GUARD, ExactWorkspace, body_ptr

CPU = torch.device("cpu")


def test_layout_and_fills():
    ws = ExactWorkspace(slack=0, poison=0xFF)
    a = ws(1000, CPU)
    b = ws(1000, CPU, owner="conv_gemm")
    assert a.dtype == torch.uint8 and a.numel() == 1000 and a.data_ptr() % ALIGN == 0 and b.data_ptr() % ALIGN == 0
    assert bool((a == 0xFF).all()) and bool((b == 0).all())                 # scratch: poison; an owner's buffer: zeros
    for (nbytes, owner, whole, off, body), view in zip(ws.requests, (a, b)):
        assert (nbytes, body) == (1000, 1000) and off >= FRONT and whole.numel() - off - body >= BACK
        assert view.data_ptr() == whole.data_ptr() + off
        assert bool((whole[:off] == GUARD).all()) and bool((whole[off + body:] == GUARD).all())
    assert [r[1] for r in ws.requests] == [None, "conv_gemm"]
    assert ws.check() == 2
    z = ExactWorkspace(slack=64, poison=0x00)(1000, CPU)
    assert z.numel() == 1064 and bool((z == 0).all())
    a.fill_(7)                                                                # the whole body is the caller's
    assert ws.check() == 2


def test_a_write_one_byte_before_the_body_is_reported_with_its_offset():
    ws = ExactWorkspace()
    ws(64, CPU)
    ws(1000, CPU, owner="x")
    _, _, whole, off, _ = ws.requests[1]
    whole[off - 1] = 0
    with pytest.raises(AssertionError, match=r"owner 'x', 1000 bytes asked for.*front guard changed at body offset -1 "):
        ws.check()


def test_a_write_one_byte_after_the_body_is_reported_with_its_offset():
    ws = ExactWorkspace(slack=24)
    ws(1000, CPU)
    _, _, whole, off, body = ws.requests[0]
    assert body == 1024
    whole[off + body] = 0
    whole[off + body + 5] = 1
    with pytest.raises(AssertionError, match=r"owner None, 1000 bytes asked for \(\+24 slack\): back guard changed at body offset 1024 \(2 "):
        ws.check()


def test_a_request_for_nothing_gives_an_empty_view_with_a_valid_pointer():
    ws = ExactWorkspace()
    v = ws(0, CPU)
    _, _, whole, off, body = ws.requests[0]
    assert v.numel() == 0 and body == 0 and body_ptr(v) == whole.data_ptr() + off and body_ptr(v) % ALIGN == 0
    assert ws.check() == 1
    whole[off] = 0                               # the first byte behind an empty body is guard
    with pytest.raises(AssertionError, match="back guard changed at body offset 0 "):
        ws.check()
