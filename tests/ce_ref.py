"""The oracle of the cross-entropy options (a plain helper module, imported like util.py): torch's CPU `F.cross_entropy` in
fp64 on `F.interpolate(z.double(), mode="bilinear")`, and the closed-form loss / gradient the kernels implement, which
tests/test_ce_options_cpu.py holds against that oracle.

    keep = (y != ignore_index);  den = sum_keep w[y]
    loss = [ (1 - eps) sum_keep w[y] (lse - z_y) + (eps / C) sum_keep sum_c w[c] (lse - z_c) ] / den
    d loss / d z_c = keep [ (1 - eps) w[y] (p_c - 1[c = y]) + (eps / C) (p_c sum_k w[k] - w[c]) ] / den
"""
import torch
import torch.nn.functional as F

TORCH_IGNORE = -100   # F.cross_entropy's own default: "no ignore_index" for labels that never take this value


def upsample64(z, S):
    """fp64 [B, C, S, S]: the bilinear upsample of the low-res logits z [B, C, g, g] (align_corners=False)."""
    return F.interpolate(z.double(), (S, S), mode="bilinear", align_corners=False)


def ce_ref(z, target, S, ignore_index=None, class_weight=None, label_smoothing=0.0):
    """(loss, d loss / d up, lse, up), all fp64, from torch's CPU autograd.  target: [B, S, S] integer labels, each in
    [0, C) or equal to ignore_index (torch raises on any other)."""
    up = upsample64(z, S).requires_grad_(True)
    t = target.long()
    if ignore_index is None:
        assert not bool((t == TORCH_IGNORE).any())
    w = None if class_weight is None else torch.as_tensor(class_weight, dtype=torch.float32).double()
    loss = F.cross_entropy(up, t, weight=w, ignore_index=TORCH_IGNORE if ignore_index is None else int(ignore_index),
                           label_smoothing=float(label_smoothing), reduction="mean")
    loss.backward()
    return loss.detach(), up.grad, torch.logsumexp(up.detach(), dim=1), up.detach()


def ce_closed_form(up, target, ignore_index=None, class_weight=None, label_smoothing=0.0):
    """(loss, d loss / d up, den) from the formulas above in fp64, no autograd.  Labels outside [0, C) other than
    ignore_index are not handled here."""
    up = up.double()
    B, C = up.shape[0], up.shape[1]
    t = target.long()
    keep = torch.ones_like(t, dtype=torch.bool) if ignore_index is None else t != int(ignore_index)
    w = torch.ones(C, dtype=torch.float64) if class_weight is None else \
        torch.as_tensor(class_weight, dtype=torch.float32).double()
    eps = float(label_smoothing)
    tc = torch.where(keep, t, torch.zeros_like(t))
    lse = torch.logsumexp(up, dim=1)
    p = torch.exp(up - lse[:, None])
    wy = w[tc] * keep
    den = wy.sum()
    zy = up.gather(1, tc[:, None])[:, 0]
    wv = w.view(1, C, 1, 1)
    smooth = ((lse[:, None] - up) * wv).sum(1) * keep
    loss = ((1.0 - eps) * (wy * (lse - zy)).sum() + eps / C * smooth.sum()) / den
    onehot = F.one_hot(tc, C).permute(0, 3, 1, 2).double()
    grad = ((1.0 - eps) * wy[:, None] * (p - onehot) + eps / C * (p * w.sum() - wv)) * keep[:, None] / den
    return loss, grad, den
