"""CPU restatement (torch fp32) of the test-time-augmentation merge of include/vitseg.h (vitseg_tta_blend).  Test
infrastructure, imported like util.py; built on the oracle's `upsample_bilinear`, `sigmoid_aten` and `predict_mask` and on
window_ref's single-rounding `fma_rn`, which it imports and does not edit.

A view's op is 0..7: f = op >> 2 a horizontal flip applied first, r = op & 3 counter-clockwise quarter turns.  Per class
and pixel, over the views in order:
    u_k = unview(upsample_bilinear(lowres_k, (S, S)), op_k)
    t_k = u_k (mode 0)  |  sigmoid_aten(u_k) (mode 1)
    K == 1:    result = t_1
    otherwise: acc = fma(w_k, t_k, acc) from acc = 0;   result = acc / Wsum,  Wsum = the fp32 sum of the weights in view order
    mask = first maximal index of sigmoid_aten(result) (mode 0)  |  result (mode 1)
every operation a single correctly rounded fp32 one.
"""
import torch

from oracle import vitseg_oracle as O
from window_ref import fma_rn

LOGITS, PROBS = 0, 1


def view(X, op):
    f, r = op >> 2, op & 3
    return torch.rot90(torch.flip(X, [-1]) if f else X, r, dims=(-2, -1))


def unview(Y, op):
    f, r = op >> 2, op & 3
    Z = torch.rot90(Y, -r, dims=(-2, -1))
    return Z if not f else torch.flip(Z, [-1])


def weight_sum(weights):
    ws = torch.zeros((), dtype=torch.float32)
    for w in weights:
        ws = ws + torch.tensor(w, dtype=torch.float32)
    return ws


def blend(views, S, mode):
    """views: [(lowres fp32 [n, C, g, g], op, weight)] -> merged fp32 [n, C, S, S]"""
    ts = []
    for low, op, _ in views:
        assert low.dtype == torch.float32
        u = unview(O.upsample_bilinear(low, (S, S)), op).contiguous()
        ts.append(O.sigmoid_aten(u) if mode == PROBS else u)
    if len(views) == 1:
        return ts[0]
    acc = torch.zeros_like(ts[0])
    for t, (_, _, w) in zip(ts, views):
        acc = fma_rn(torch.full_like(t, w), t, acc)
    return acc / weight_sum([w for _, _, w in views])


def mask(merged, mode):
    """uint8 [n, S, S]: the first maximal index of sigmoid_aten(merged) (mode 0) or of merged (mode 1)"""
    if mode == PROBS:
        return merged.argmax(dim=1).to(torch.uint8)   # torch's argmax returns the first maximal index
    return O.predict_mask(merged).to(torch.uint8)
