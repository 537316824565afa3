"""A stand-in for dasac_hip.lib.workspace that hands every caller EXACTLY the bytes it asked for, between two guards (a helper,
not a conftest).  Tests install it with monkeypatch.setattr(dasac_hip.lib, "workspace", ExactWorkspace(...)): every wrapper looks
`L.workspace` up at call time.

Each request gets one fresh uint8 tensor
    [ front guard 4096 B | body of nbytes + slack | back guard >= 1 MiB ]
whose body starts on a 256-byte boundary.  Both guards hold 0xA5; the body holds `poison` (owner None: scratch whose contents
the contract leaves undefined) or zeros (a named owner: include/dasac_hip.h promises those buffers zero-filled).  The back guard
is at least as large as the 1 MiB floor of the real cache, so a write that stayed inside the real buffer stays inside this
allocation: an overrun is detected, never provoked."""
import torch

GUARD = 0xA5
FRONT = 4096
BACK = 1 << 20
ALIGN = 256


def body_ptr(view):
    """Address of a returned view's first byte.  For a request of 0 bytes the view is empty, and torch reports data_ptr() == 0 for
    every empty tensor; the view still lies at the body's place in its allocation, which this returns."""
    return view.untyped_storage().data_ptr() + view.storage_offset()


class ExactWorkspace:
    def __init__(self, slack=0, poison=0xFF):
        self.slack, self.poison = int(slack), int(poison)
        self.requests = []            # (nbytes, owner, whole tensor, body offset, body bytes)

    def __call__(self, nbytes, device, owner=None):
        nbytes = int(nbytes)
        body = nbytes + self.slack
        whole = torch.empty(FRONT + body + BACK + ALIGN, dtype=torch.uint8, device=device)
        off = FRONT + (-(whole.data_ptr() + FRONT)) % ALIGN
        whole.fill_(GUARD)
        view = whole[off:off + body]
        view.fill_(0 if owner is not None else self.poison)
        self.requests.append((nbytes, owner, whole, off, body))
        return view

    def check(self):
        """Asserts that no guard byte of any request changed; returns the number of requests."""
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        for nbytes, owner, whole, off, body in self.requests:
            for name, lo, hi in (("front", 0, off), ("back", off + body, whole.numel())):
                bad = (whole[lo:hi] != GUARD).nonzero()
                if bad.numel():
                    first = lo + int(bad[0]) - off            # relative to the body's first byte
                    raise AssertionError("workspace of owner {!r}, {} bytes asked for (+{} slack): {} guard changed at body offset {} "
                                         "({} bytes in all)".format(owner, nbytes, self.slack, name, first, bad.numel()))
        return len(self.requests)
