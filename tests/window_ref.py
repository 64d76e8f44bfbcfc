"""CPU restatement (torch fp32) of the sliding-window arithmetic of include/vitseg.h: the window grid
(vitseg_window_count / vitseg_window_origins), the tile gather (vitseg_window_gather) and the overlapping-tile blend
(vitseg_window_blend).  Test infrastructure, imported like util.py; built on the oracle's `upsample_bilinear`, `_fma`,
`sigmoid_aten` and `predict_mask`, which it imports and does not edit.

The blend, per pixel and class, over the covering tiles in increasing tile number (image-major, window row, window column):
    v  = upsample_bilinear(tile's low-res map)[ly, lx]           (the decoder tail's taps and fma placement)
    wt = w[ly] * w[lx]
    one covering tile:  result = v
    otherwise:          acc = fma(wt, v, acc);  ws = ws + wt   from acc = 0, ws = 0;   result = acc / ws
every operation a single correctly rounded fp32 one.
"""
import torch

from oracle import vitseg_oracle as O


def count(extent, S, stride):
    """1 + ceil((extent - S) / stride)"""
    return 1 + -((S - extent) // stride)


def origins(extent, S, stride):
    """origin_i = min(i * stride, extent - S): the last window is shifted back to end at the edge"""
    return [min(i * stride, extent - S) for i in range(count(extent, S, stride))]


def weights(kind, S):
    if kind == "uniform":
        return torch.ones(S, dtype=torch.float32)
    assert kind == "linear", kind
    i = torch.arange(S, dtype=torch.float32)
    return torch.minimum(i + 1, S - i)          # min(i + 1, S - i): an exact triangular window


def gather(x, S, oy, ox):
    """fp32 NCHW [n, 3, H, W] -> tiles [n * ny * nx, 3, S, S] in tile order (torch slicing)"""
    return torch.stack([x[b, :, y:y + S, xx:xx + S] for b in range(x.shape[0]) for y in oy for xx in ox])


def fma_rn(a, b, c):
    """round_fp32(a * b + c) with ONE rounding.  The oracle's `_fma` forms a * b + c in fp64 (the product is exact there, the
    sum is rounded to 53 bits) and rounds that to fp32: two roundings, which differ from one exactly when the fp64 sum lies on
    the midpoint of two fp32 values while the true sum does not.  Those cases are found (the low 29 bits of the fp64
    significand are 1 0...0) and decided by the sign of the fp64 sum's own rounding error (TwoSum, exact)."""
    r = O._fma(a, b, c)
    p, cd = a.double() * b.double(), c.double().expand_as(r)
    s = p + cd
    mid = (s.view(torch.int64) & 0x1FFFFFFF) == 0x10000000
    if bool(mid.any()):
        bb = s - p
        err = (p - (s - bb)) + (cd - bb)          # s + err = p + c exactly
        lo = torch.nextafter(r, torch.full_like(r, float("-inf")))
        hi = torch.nextafter(r, torch.full_like(r, float("inf")))
        # the fp32 neighbours of the midpoint s: r is one of them, the other lies across s
        other = torch.where(r.double() > s, lo, hi)
        up, down = torch.maximum(r, other), torch.minimum(r, other)
        fixed = torch.where(err > 0, up, torch.where(err < 0, down, r))
        r = torch.where(mid & torch.isfinite(s), fixed, r)
    return r


def blend(lowres, n, H, W, S, oy, ox, w):
    """lowres fp32 [n * ny * nx, C, g, g] -> blended logits fp32 [n, C, H, W]"""
    ny, nx = len(oy), len(ox)
    T, C = lowres.shape[0], lowres.shape[1]
    assert T == n * ny * nx and lowres.dtype == torch.float32
    wt = (w[:, None] * w[None, :]).expand(C, S, S)
    acc = torch.zeros((n, C, H, W), dtype=torch.float32)
    ws = torch.zeros((n, C, H, W), dtype=torch.float32)
    one = torch.zeros((n, C, H, W), dtype=torch.float32)
    cnt = torch.zeros((n, 1, H, W), dtype=torch.int32)
    t = 0
    for b in range(n):
        for y in oy:
            for x in ox:
                v = O.upsample_bilinear(lowres[t:t + 1], (S, S))[0]
                sl = (b, slice(None), slice(y, y + S), slice(x, x + S))
                acc[sl] = fma_rn(wt, v, acc[sl])
                ws[sl] = ws[sl] + wt
                one[sl] = v
                cnt[b, :, y:y + S, x:x + S] += 1
                t += 1
    assert int(cnt.min()) >= 1, "a pixel is covered by no window"
    return torch.where(cnt == 1, one, acc / ws)


def mask(logits):
    """argmax_c sigmoid_aten(logits), first maximal index (uint8)"""
    return O.predict_mask(logits).to(torch.uint8)


def ties(logits):
    """number of pixels where two classes share the maximal fp32 sigmoid"""
    s = O.sigmoid_aten(logits)
    return int(((s == s.max(dim=1, keepdim=True).values).sum(dim=1) > 1).sum())
