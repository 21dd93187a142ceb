"""Where a pass writes, as a test input: guard bands around every `torch.empty`, the check of a red-zoned workspace
against the regions its pass carved, and the bit-for-bit snapshot of what a call may only read.
A plain module, imported by name: it registers no fixture and no plugin, and importing it needs no GPU."""
import contextlib

import torch

from tests import poison

# Every check runs once per fill: a stray byte equals at most one of the two, so no stray store escapes both.
FILLS = poison.FILLS[1:]
assert FILLS == (0xFF, 0x7B)


def _first_bad(t, fill):
    """The index of the first byte of the uint8 tensor `t` that is not `fill`, or None."""
    bad = (t != fill).nonzero()
    return int(bad[0]) if bad.numel() else None


class GuardedAllocs:
    """The allocations made inside guarded_allocs(): (byte buffer, bytes of the tensor, its shape, its dtype) each."""
    def __init__(self, fill, band):
        self.fill, self.band, self.allocs = int(fill), int(band), []

    def check(self):
        """Both bands of every allocation still hold the fill."""
        for raw, nbytes, shape, dtype in self.allocs:
            front, behind = _first_bad(raw[:self.band], self.fill), _first_bad(raw[self.band + nbytes:], self.fill)
            what = f"torch.empty({tuple(shape)}, {dtype}) of {nbytes} bytes, bands of {self.band} filled with {self.fill:#04x}"
            assert front is None, f"{what}: byte {self.band - front} in front of the tensor holds {int(raw[front]):#04x}"
            assert behind is None, f"{what}: byte {behind} behind the tensor's end holds {int(raw[self.band + nbytes + behind]):#04x}"


@contextlib.contextmanager
def guarded_allocs(fill, band=65536, device_type="cuda"):
    """Inside the body every `torch.empty` on a device of `device_type` -- native.py's outputs and any workspace it grows -- returns a
    view into a byte buffer of band + nbytes + band filled with `fill` (the tensor's own bytes too).  The band is a multiple of 512,
    so the view keeps a fresh allocation's alignment.  Yields the record of those allocations; its check() asserts that both bands
    of each still hold the fill.  `torch.empty` is the original again afterwards, also when the body raises."""
    assert band > 0 and band % 512 == 0
    real = torch.empty
    rec = GuardedAllocs(fill, band)

    def empty(*size, **kw):
        dev = kw.get("device")
        if dev is None or torch.device(dev).type != device_type or set(kw) - {"device", "dtype"}:
            return real(*size, **kw)
        dtype = kw.get("dtype") or torch.get_default_dtype()
        meta = real(*size, dtype=dtype, device="meta")
        nbytes = meta.numel() * meta.element_size()
        raw = torch.full((band + nbytes + band,), rec.fill, dtype=torch.uint8, device=dev)
        rec.allocs.append((raw, nbytes, meta.shape, dtype))
        return raw[band:band + nbytes].view(dtype).view(meta.shape)

    torch.empty = empty
    try:
        yield rec
    finally:
        torch.empty = real


def check_workspace(ws, regions, fill):
    """Every byte of the uint8 tensor `ws` outside the union of [offset, offset + bytes) of `regions` -- (name, offset, bytes) as
    NativeContext.ws_regions returns them -- still equals `fill`: the zones, the alignment slack behind a region's requested bytes,
    and the rest up to the end.  The message names the region in front of the first bad byte and how far behind it the byte lies."""
    fill = int(fill)
    gaps, end, prev = [], 0, None                               # (first byte, one past the last, the region in front)
    for name, off, n in sorted(regions, key=lambda r: (r[1], r[1] + r[2])):
        assert 0 <= off and off + n <= ws.numel(), f"region {name} = [{off}, {off + n}) leaves the workspace of {ws.numel()} bytes"
        if off > end:
            gaps.append((end, off, prev))
        if off + n >= end:
            end, prev = off + n, (name, off, n)
    if ws.numel() > end:
        gaps.append((end, ws.numel(), prev))
    if not gaps or not bool((torch.cat([ws[a:b] for a, b, _ in gaps]) != fill).any()):
        return
    for a, b, front in gaps:
        i = _first_bad(ws[a:b], fill)
        if i is not None:
            where = (f"{a + i - (front[1] + front[2])} bytes behind the requested {front[2]} bytes of region {front[0]!r} (at offset {front[1]})"
                     if front else "in front of the first region")
            raise AssertionError(f"workspace byte {a + i} holds {int(ws[a + i]):#04x}, not the fill {fill:#04x}: {where}")


class unchanged:
    """A snapshot of {name: tensor} (or a sequence of tensors; None entries are skipped) taken now; check() holds each tensor to the
    same bits.  For what a call may only read: its inputs and engine.weights_tensor()."""
    def __init__(self, tensors):
        items = tensors.items() if isinstance(tensors, dict) else enumerate(tensors)
        self.live = {k: t for k, t in items if t is not None}
        self.was = {k: t.detach().clone() for k, t in self.live.items()}

    def check(self):
        for k, t in self.live.items():
            same = t.shape == self.was[k].shape and torch.equal(poison.bits(t), poison.bits(self.was[k]))
            if not same:
                bad = (poison.bits(t) != poison.bits(self.was[k])).reshape(-1).nonzero().reshape(-1)
                raise AssertionError(f"input {k!r} of shape {tuple(t.shape)} was written: {bad.numel()} elements differ, the first at flat index {int(bad[0])}")
