"""CPU restatement of vitseg_confidence (include/vitseg.h): the per-pixel score of a stated mask, its 16-bit form, the
per-region score rows and the calibration histogram.  Test infrastructure, imported like util.py; built on the oracle's
`upsample_bilinear` and `sigmoid_aten`, which it imports and does not edit (the oracle, not F.interpolate: below H + W > 128
ATen takes another kernel whose last bit differs, oracle/vitseg_oracle.py:195).

Per pixel, c = mask[pixel], v_k = upsample_bilinear(lowres)[k, pixel]:
    prob    p = sigmoid_aten(v_c)
    margin  p = min(max(sigmoid_aten(v_c) - sigmoid_aten(max_{k != c} v_k), 0), 1)
    c >= C  p = 0
    q = rint(p * float32(65535))      (fp32 product, ties to even)
every operation a single correctly rounded fp32 one.
"""
import numpy as np
import torch

from oracle import vitseg_oracle as O

KINDS = {"prob": 0, "margin": 1}


def values(lowres, S):
    """fp32 [n, C, g, g] -> the full-size logits fp32 [n, C, S, S] (the decoder tail's taps and fma placement)"""
    return O.upsample_bilinear(lowres, (S, S))


def score_logits(v, mask, kind):
    """(p fp32 [n, S, S], q int64 [n, S, S]) numpy arrays from full-size logits v [n, C, S, S] and mask uint8 [n, S, S]"""
    C = v.shape[1]
    m = mask.long()
    valid = m < C
    mc = m.clamp(max=C - 1)[:, None]
    vc = v.gather(1, mc)[:, 0]
    if kind == "prob":
        p = O.sigmoid_aten(vc)
    else:
        assert kind == "margin" and C >= 2, (kind, C)
        other = v.clone().scatter_(1, mc, float("-inf")).max(dim=1).values
        p = (O.sigmoid_aten(vc) - O.sigmoid_aten(other)).clamp(0.0, 1.0)
    p = torch.where(valid, p, torch.zeros_like(p)).numpy()
    assert p.dtype == np.float32
    q = np.rint(p * np.float32(65535)).astype(np.int64)
    return p, q


def confidence(lowres, mask, kind):
    """(p, q) of a low-res head output fp32 [n, C, g, g] and a mask uint8 [n, S, S]"""
    return score_logits(values(lowres, mask.shape[-1]), mask, kind)


def score_rows(q, labels, max_regions, low_q):
    """int64 [n, max_regions, 4]: per region (pixels, sum_q, max(65535 - q), pixels with q < low_q); labels int [n, S, S],
    negative = no region, an index >= max_regions is skipped"""
    q = np.asarray(q)
    lab = np.asarray(labels).astype(np.int64)
    n = q.shape[0]
    out = np.zeros((n, max_regions, 4), dtype=np.int64)
    for b in range(n):
        keep = (lab[b] >= 0) & (lab[b] < max_regions)
        l, v = lab[b][keep], q[b][keep]
        out[b, :, 0] = np.bincount(l, minlength=max_regions)
        # (float64 weights: a sum below 2^53 is exact)
        out[b, :, 1] = np.bincount(l, weights=v.astype(np.float64), minlength=max_regions).astype(np.int64)
        np.maximum.at(out[b, :, 2], l, 65535 - v)
        out[b, :, 3] = np.bincount(l, weights=(v < low_q).astype(np.float64), minlength=max_regions).astype(np.int64)
    return out


def hist(q, mask, gt, bins, ignore_label=-1):
    """int64 [n, bins, 3]: per image and bin = (q * bins) >> 16 the (pixels, pixels with mask == gt, sum_q) over the pixels
    with gt != ignore_label"""
    q = np.asarray(q)
    m, t = np.asarray(mask).astype(np.int64), np.asarray(gt).astype(np.int64)
    n = q.shape[0]
    out = np.zeros((n, bins, 3), dtype=np.int64)
    for b in range(n):
        keep = t[b] != ignore_label
        v = q[b][keep]
        k = (v * bins) >> 16
        out[b, :, 0] = np.bincount(k, minlength=bins)
        out[b, :, 1] = np.bincount(k, weights=(m[b][keep] == t[b][keep]).astype(np.float64), minlength=bins).astype(np.int64)
        out[b, :, 2] = np.bincount(k, weights=v.astype(np.float64), minlength=bins).astype(np.int64)
    return out
