"""The oracle of the hard-pixel losses (a plain helper module, imported like ce_ref.py): the focal / OHEM loss of
include/vitseg_hardloss.h in fp64 by torch's CPU autograd over a GIVEN hard set, the closed form the kernels implement, and
the exact integer / bit selection of the hard set from an fp32 plane of per-pixel CE values.

    ce_i = lse - up_y;  q_i = -expm1(-ce_i);  f_i = w[y] q_i^gamma ce_i;  m_i = q_i^gamma + gamma (1 - q_i) ce_i q_i^(gamma - 1)
    loss = sum_H f_i / sum_H w[y];  d loss / d up_c = [i in H] w[y] m_i (p_c - 1[c = y]) / sum_H w[y]
    k = min(n_valid, max(min_kept, ceil(n_valid keep_q16 / 65536)));  tau = min(loss_thresh, k-th largest ce);  H = {ce >= tau}
"""
import numpy as np
import torch
import torch.nn.functional as F

import ce_ref


def _setup(up, target, kept_mask, ignore_index, class_weight):
    C = up.shape[1]
    t = target.long()
    keep = torch.ones_like(t, dtype=torch.bool) if ignore_index is None else t != int(ignore_index)
    hard = keep if kept_mask is None else keep & torch.as_tensor(kept_mask, dtype=torch.bool)
    w = torch.ones(C, dtype=torch.float64) if class_weight is None else \
        torch.as_tensor(class_weight, dtype=torch.float32).double()
    tc = torch.where(keep, t, torch.zeros_like(t))
    return keep, hard.detach(), w, tc


def hard_ref(z, target, S, kept_mask, gamma, ignore_index=None, class_weight=None):
    """(loss, d loss / d up, ce, up), all fp64, from torch's CPU autograd: F.cross_entropy(reduction="none") on
    ce_ref.upsample64(z, S), modulated, weighted and summed over the given, detached hard set (`kept_mask` [B, S, S] bool, or
    None for every valid pixel; ignored pixels are never in it)."""
    up = ce_ref.upsample64(z, S).requires_grad_(True)
    keep, hard, w, tc = _setup(up, target, kept_mask, ignore_index, class_weight)
    ce = F.cross_entropy(up, tc, reduction="none")
    q = -torch.expm1(-ce)
    f = w[tc] * q.pow(float(gamma)) * ce if gamma != 0 else w[tc] * ce
    loss = (f * hard).sum() / (w[tc] * hard).sum()
    loss.backward()
    return loss.detach(), up.grad, ce.detach(), up.detach()


def focal_m(q, ce, gamma):
    """m of the header, elementwise in q's dtype; 0 where q == 0 with gamma > 0, 1 everywhere for gamma == 0."""
    if gamma == 0:
        return torch.ones_like(q)
    safe = torch.where(q == 0, torch.ones_like(q), q)
    m = safe.pow(gamma) + gamma * (1.0 - safe) * ce * safe.pow(gamma - 1.0)
    return torch.where(q == 0, torch.zeros_like(q), m)


def hard_closed_form(up, target, kept_mask, gamma, ignore_index=None, class_weight=None):
    """(loss, d loss / d up, den, ce) from the formulas above in fp64, no autograd.  Labels outside [0, C) other than
    ignore_index are not handled here."""
    up = up.double()
    C = up.shape[1]
    keep, hard, w, tc = _setup(up, target, kept_mask, ignore_index, class_weight)
    lse = torch.logsumexp(up, dim=1)
    p = torch.exp(up - lse[:, None])
    ce = lse - up.gather(1, tc[:, None])[:, 0]
    q = -torch.expm1(-ce)
    mod = torch.where(q == 0, torch.zeros_like(q), q.pow(gamma)) if gamma != 0 else torch.ones_like(q)
    wy = w[tc] * hard
    den = wy.sum()
    loss = (wy * mod * ce).sum() / den
    onehot = F.one_hot(tc, C).permute(0, 3, 1, 2).double()
    grad = (wy * focal_m(q, ce, gamma))[:, None] * (p - onehot) / den
    return loss, grad, den, ce


def select_ref(plane, valid, loss_thresh, min_kept, keep_q16):
    """(k, bits of tau, H) of the selection, exactly: `plane` fp32 [...] of per-pixel CE values (>= +0 or NaN on valid
    pixels), `valid` bool of the same shape.  The k-th largest is taken on the uint32 view, where the order of the bit
    patterns is the order of the values and NaN ranks above +inf."""
    plane = np.ascontiguousarray(np.asarray(plane, dtype=np.float32))
    valid = np.asarray(valid, dtype=bool)
    bits = plane.view(np.uint32)
    vb = bits[valid]
    assert not (vb >> 31).any(), "a valid pixel's CE has its sign bit set"
    n = int(vb.size)
    k = min(n, max(int(min_kept), (n * int(keep_q16) + 65535) >> 16))
    tau = int(np.array(loss_thresh, dtype=np.float32).view(np.uint32))
    if k > 0:
        tau = min(tau, int(np.partition(vb, n - k)[n - k]))
    return k, tau, valid & (bits >= np.uint32(tau))
