"""CPU checks of tests/guard.py: a write one element outside the payload is caught and reported at the right offset."""
import pytest
import torch

from guard import check, guarded, snapshot, unchanged


def _flat(t):
    return t._guard.buf


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16, torch.uint8, torch.int64])
def test_untouched_buffer_passes(dtype):
    t = guarded((5, 7), dtype, "zero", device="cpu", name="C")
    t.fill_(1)
    check(t)
    assert t.is_contiguous() and tuple(t.shape) == (5, 7) and t.dtype == dtype
    assert t.data_ptr() % 4096 == _flat(t).data_ptr() % 4096   # the guard is a multiple of 4096 bytes


def test_guard_sizes_and_fill():
    t = guarded((3, 4096), torch.float32, "nan", device="cpu")
    g = t._guard
    assert g.head % 4096 == 0 and g.head >= 1 << 20 and g.head >= 256 * 4096 * 4
    assert len(g.buf) - g.head - g.nbytes == g.head
    assert torch.isnan(t).all()
    src = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    assert torch.equal(guarded((3, 4), torch.float32, src, device="cpu"), src)
    m = guarded((2, 2), torch.uint8, "nan", device="cpu")
    assert (m == 255).all()
    flat = guarded(3 << 20, torch.float32, "zero", device="cpu")   # 1-D: rows of one element, so the guard stays 1 MiB
    assert flat._guard.head == 1 << 20


def test_write_one_element_past_the_end():
    t = guarded((4, 8), torch.float32, "zero", device="cpu", name="C")
    flat = _flat(t)
    g = t._guard
    flat[g.head + g.nbytes:g.head + g.nbytes + 4].view(torch.float32)[0] = 0.0   # element 0 past the end
    with pytest.raises(AssertionError, match=r"wrote 1 row past the end of C .*from element 0 to 0 past the end"):
        check(t)


def test_write_rows_past_the_end_counts_rows():
    t = guarded((4, 8), torch.float32, "zero", device="cpu", name="C")
    g = t._guard
    tail = g.buf[g.head + g.nbytes:].view(torch.float32)
    tail[2 * 8 + 5] = 1.0   # row 2 past the end, i.e. 3 rows written past the end
    with pytest.raises(AssertionError, match=r"wrote 3 rows past the end of C .*from element 21 to 21"):
        check(t)


def test_write_one_element_before_the_start():
    t = guarded((4, 8), torch.bfloat16, "zero", device="cpu", name="A")
    g = t._guard
    g.buf[g.head - 2:g.head].view(torch.bfloat16)[0] = 0.0   # the element just before the payload
    with pytest.raises(AssertionError, match=r"wrote 1 row before the start of A .*from 1 to 1 elements"):
        check(t)


def test_single_corrupted_byte_is_caught():
    t = guarded(16, torch.float32, "zero", device="cpu", name="v")
    g = t._guard
    g.buf[-1] = 0x7F   # the very last guard byte
    with pytest.raises(AssertionError, match="past the end of v"):
        check(t)


def test_snapshot_unchanged():
    x = guarded((3, 3), torch.float32, torch.arange(9.0).reshape(3, 3) + 1.0, device="cpu", name="x")
    y = torch.full((2,), float("nan"))
    snap = snapshot(x, None, y)
    unchanged(snap)   # NaN payloads compare bitwise
    x[1, 1] = -x[1, 1]   # one sign bit
    with pytest.raises(AssertionError, match="x changed: 1 bytes differ"):
        unchanged(snap)
