"""Guard-banded buffers for the kernel tests (a plain helper module, imported like util.py).

`guarded(shape, dtype, fill)` returns a contiguous payload view into one flat buffer laid out as
head guard | payload | tail guard.  The guards hold 0xFF bytes -- NaN in fp32 / bf16 / fp16 and 255 in a uint8 mask, which
no class index reaches -- so a store past either end of the payload is caught by `check()`, and a load past either end that
feeds a result surfaces as NaN.  Each guard is at least 1 MiB and at least 256 payload rows (one 256-row tile written past
the end; a 1-D payload counts as rows of one element), rounded up to 4096 bytes so the payload keeps at least the alignment torch's allocator gives.

`snapshot(*inputs)` / `unchanged(snap)` check that a call left its inputs bitwise the same.
"""
import torch

GUARD_BYTE = 0xFF
_MIN_GUARD = 1 << 20
_ALIGN = 4096


class _Guard:
    __slots__ = ("buf", "head", "nbytes", "esize", "row", "name")

    def __init__(self, buf, head, nbytes, esize, row, name):
        self.buf, self.head, self.nbytes, self.esize, self.row, self.name = buf, head, nbytes, esize, row, name


def _guard_bytes(row_bytes):
    g = max(_MIN_GUARD, 256 * row_bytes)
    return (g + _ALIGN - 1) // _ALIGN * _ALIGN


def guarded(shape, dtype=torch.float32, fill="nan", device="cuda:0", name=None):
    """Payload tensor of `shape` / `dtype` between two 0xFF guards.  fill: "nan" (0xFF bytes), "zero", or a tensor whose
    values are copied in (its shape must match).  The returned view keeps the whole buffer alive."""
    if isinstance(shape, int):
        shape = (shape,)
    shape = tuple(int(d) for d in shape)
    esize = torch.empty((), dtype=dtype).element_size()
    numel = 1
    for d in shape:
        numel *= d
    nbytes = numel * esize
    row = shape[-1] if len(shape) >= 2 else 1   # a flat buffer (scratch, arena) has no rows: offsets are in elements
    g = _guard_bytes(max(row, 1) * esize)
    buf = torch.full((2 * g + nbytes,), GUARD_BYTE, dtype=torch.uint8, device=device)
    payload = buf[g:g + nbytes].view(dtype).view(shape)
    if isinstance(fill, torch.Tensor):
        assert tuple(fill.shape) == shape, (tuple(fill.shape), shape)
        payload.copy_(fill)
    elif fill == "zero":
        payload.zero_()
    else:
        assert fill == "nan", fill   # the payload already holds 0xFF bytes
    payload._guard = _Guard(buf, g, nbytes, esize, max(row, 1), name)
    return payload


def _describe(off, nbytes, esize, row, before):
    """offset of a corrupted byte: elements / rows before the start or past the end of the payload."""
    dist = (-off if before else off - nbytes)   # bytes; >= 1 before the start, >= 0 past the end
    el = (dist + esize - 1) // esize if before else dist // esize
    rows = (el + row - 1) // row if before else el // row
    return el, rows


def _unit(count, row):
    word = "row" if row > 1 else "element"
    return word if count == 1 else word + "s"


def check(*tensors):
    """Asserts that both guards of every guarded tensor are byte-identical to the 0xFF pattern."""
    for i, t in enumerate(tensors):
        if t is None:
            continue
        gd = getattr(t, "_guard", None)
        assert gd is not None, f"tensor {i} was not allocated by guarded()"
        name = gd.name or f"tensor {i}"
        head = gd.buf[:gd.head] != GUARD_BYTE
        tail = gd.buf[gd.head + gd.nbytes:] != GUARD_BYTE
        if not bool(head.any()) and not bool(tail.any()):
            continue
        bad_head = head.nonzero().flatten()
        bad_tail = tail.nonzero().flatten()
        msgs = []
        if bad_head.numel():
            first, last = int(bad_head[0]) - gd.head, int(bad_head[-1]) - gd.head   # negative byte offsets
            e0, r0 = _describe(first, gd.nbytes, gd.esize, gd.row, True)
            e1, r1 = _describe(last, gd.nbytes, gd.esize, gd.row, True)
            msgs.append(f"wrote {r0} {_unit(r0, gd.row)} before the start of {name} ({bad_head.numel()} bytes changed, from {e0} to {e1} "
                        f"elements / {r0} to {r1} rows before the start)")
        if bad_tail.numel():
            first, last = int(bad_tail[0]) + gd.nbytes, int(bad_tail[-1]) + gd.nbytes
            e0, r0 = _describe(first, gd.nbytes, gd.esize, gd.row, False)
            e1, r1 = _describe(last, gd.nbytes, gd.esize, gd.row, False)
            msgs.append(f"wrote {r1 + 1} {_unit(r1 + 1, gd.row)} past the end of {name} ({bad_tail.numel()} bytes changed, from element {e0} "
                        f"to {e1} past the end / rows {r0} to {r1} past the end)")
        assert not msgs, "; ".join(msgs)


def snapshot(*tensors):
    """Bitwise copies of the given tensors (None entries kept), for `unchanged`."""
    return [(t, None if t is None else t.detach().clone()) for t in tensors]


def unchanged(snap):
    """Asserts every tensor of a `snapshot` is bitwise what it was (NaN payloads included)."""
    for i, (t, c) in enumerate(snap):
        if t is None:
            continue
        a = t.detach().contiguous().view(-1).view(torch.uint8)
        b = c.contiguous().view(-1).view(torch.uint8)
        if not torch.equal(a, b):
            n = int((a != b).sum())
            name = getattr(getattr(t, "_guard", None), "name", None) or f"input {i}"
            raise AssertionError(f"{name} changed: {n} bytes differ")
