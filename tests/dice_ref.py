"""The oracle of the fused CE + soft-Dice loss (a plain helper module, imported like ce_ref.py): torch's CPU autograd in
fp64 on `ce_ref.upsample64`, the closed form the kernels implement (include/vitseg.h, vitseg_ce_dice_loss), an fp32
emulation of the kernels' arithmetic, the cases both test files run, and the error bound of the GPU test.

    keep = (y != ignore_index);  K = the classes counted (all, or 1 .. C-1 without the background)
    I_c = sum_keep p_c t_c;  P_c = sum_keep p_c;  T_c = sum_keep t_c;  N_c = 2 I_c + smooth;  D_c = P_c + T_c + smooth
    dice = mean_K [ 1 - N_c / D_c ];  loss = ce_weight CE + dice_weight dice
    a_c = -[2 t_c D_c - N_c] / (|K| D_c^2) on kept pixels for c in K, else 0
    d loss / d up_c = ce_weight (CE gradient of ce_ref.py) + dice_weight p_c (a_c - sum_k a_k p_k)

The bound (`bounds`), from U = 2^-23 and e_pix, the bound of test_gpu_ce_options._ce_bounds on the fp32 error of lse - z_c
at one pixel (4 U |lse| + 8 U |z| + 4 (C + 2) U), to first order with 1 % on top for the higher orders:
  - p_c = expf(z_c - lse) carries a relative error <= eps = e_pix + 8 U (the argument's error, expf itself).
  - I_c and P_c are sums of non-negative p's accumulated in fp64 (n 2^-53: nothing): relative error <= eps each; T_c is a
    count, exact.  So |dN_c| <= 2 eps I_c <= eps N_c and |dD_c| <= eps P_c <= eps D_c.
  - the quotient: |d(N_c / D_c)| <= |dN_c| / D_c + N_c |dD_c| / D_c^2 <= 2 eps N_c / D_c.  dice is their mean over K, formed
    in fp64 and rounded to fp32 once:  |d dice| <= 2 eps mean_K (N_c / D_c) + 2 U |dice|.
  - a_c: for t_c = 0 it is N_c / (|K| D_c^2), relative error <= 3 eps; for t_c = 1 the numerator 2 D_c - N_c >= D_c moves
    by <= 3 eps D_c, so relative error <= 5 eps; one more U for the conversion to fp32.  With A = max over c in K of
    max(N_c, 2 D_c - N_c) / (|K| D_c^2), every |a_c| <= A and |da_c| <= (5 eps + U) A.
  - S = sum_k a_k p_k is a convex combination, |S| <= A; its error is sum_k (|da_k| p_k + |a_k| |dp_k|) plus C fp32 adds
    and C products of partial sums <= A:  |dS| <= A (6 eps + (C + 2) U).
  - p_c (a_c - S): |a_c - S| <= 2 A, so the error is p_c (|da_c| + |dS|) + eps p_c 2 A + 2 U 2 A (the subtraction and the
    product) <= A (13 eps + (C + 7) U); the factor dice_weight * loss_scale and the last product add 2 U 2 A:
    |d G_dice| <= dice_weight |loss_scale| A (13 eps + (C + 12) U).
  - the CE term keeps the bounds of test_gpu_ce_options (restated in `bounds`), times ce_weight; the sum of the two terms
    is one more fp32 rounding of each side (4 U max |G|, 2 U |loss|).
"""
import functools

import torch
import torch.nn.functional as F

from ce_ref import TORCH_IGNORE, upsample64

U = 2.0 ** -23   # fp32 unit roundoff (half an ulp of 1)


def _keep(t, ignore_index):
    return torch.ones_like(t, dtype=torch.bool) if ignore_index is None else t != int(ignore_index)


def _weights64(class_weight, C):
    return torch.ones(C, dtype=torch.float64) if class_weight is None else \
        torch.as_tensor(class_weight, dtype=torch.float32).double()


def ce_dice_torch(up, target, dice_weight=1.0, ce_weight=1.0, smooth=1e-6, include_background=True, ignore_index=None,
                  class_weight=None, label_smoothing=0.0):
    """(loss, ce, dice) of the full-size logits `up` [B, C, S, S] from plain, differentiable torch ops in up's dtype and on
    its device: the definition written down.  target: [B, S, S] integer labels, each in [0, C) or equal to ignore_index.
    The weights and smooth are taken as the fp32 values the kernels read.  ce_weight == 0: no CE term is formed (ce = 0)."""
    C = up.shape[1]
    t = target.long()
    keep = _keep(t, ignore_index)
    dw, cw, sm = (float(torch.tensor(float(v), dtype=torch.float32)) for v in (dice_weight, ce_weight, smooth))
    p = torch.softmax(up, dim=1).permute(0, 2, 3, 1)[keep]          # [n_keep, C]: ignored pixels are not part of the graph
    onehot = F.one_hot(t[keep], C).to(up.dtype)
    I, P, T = (p * onehot).sum(0), p.sum(0), onehot.sum(0)
    c0 = 0 if include_background else 1
    dice = (1.0 - (2.0 * I + sm) / (P + T + sm))[c0:].mean()
    if cw != 0.0:
        w = None if class_weight is None else torch.as_tensor(class_weight, dtype=torch.float32).to(up.device, up.dtype)
        ce = F.cross_entropy(up, t, weight=w, ignore_index=TORCH_IGNORE if ignore_index is None else int(ignore_index),
                             label_smoothing=float(label_smoothing), reduction="mean")
        loss = cw * ce + dw * dice if dw != 0.0 else cw * ce
    else:
        ce = torch.zeros((), dtype=up.dtype, device=up.device)
        loss = dw * dice
    return loss, ce, dice


def ce_dice_ref(z, target, S, **kw):
    """(loss, ce, dice, d loss / d up, up), all fp64, from torch's CPU autograd on `ce_dice_torch` of the fp64 upsample of
    the low-res logits z."""
    return ce_dice_ref_up(upsample64(z, S), target, **kw)


def ce_dice_ref_up(up, target, **kw):
    """The same on given full-size logits (taken to fp64 on the CPU)."""
    up = up.detach().double().cpu().requires_grad_(True)
    loss, ce, dice = ce_dice_torch(up, target.cpu(), **kw)
    loss.backward()
    return loss.detach(), ce.detach(), dice.detach(), up.grad, up.detach()


def closed_form(up, target, dice_weight=1.0, ce_weight=1.0, smooth=1e-6, include_background=True, ignore_index=None,
                class_weight=None, label_smoothing=0.0, mutate=None, dtype=torch.float64):
    """(loss, ce, dice, grad, (I, P, T)) from the formulas above, no autograd.  dtype=torch.float64: the closed form on the
    fp64 logits.  dtype=torch.float32: the kernels' arithmetic on fp32 logits `up` (the online log-sum-exp, p = exp(z - lse),
    fp64 sums of fp32 p's, fp32 a_c and gradient terms).  `mutate`: one of the wrong formulas the bound must reject --
    "no_smooth", "no_sap" (the sum_k a_k p_k term dropped), "ignored_in_P", "K_is_C"."""
    f32 = dtype == torch.float32
    up = up.to(dtype)
    B, C = up.shape[0], up.shape[1]
    t = target.long()
    keep = _keep(t, ignore_index)
    dw, cw, sm = (float(torch.tensor(float(v), dtype=torch.float32)) for v in (dice_weight, ce_weight, smooth))
    if mutate == "no_smooth":
        sm = 0.0
    eps = float(label_smoothing)
    tc = torch.where(keep, t, torch.zeros_like(t))
    if f32:   # ce_loss_kernel's online log-sum-exp, class by class
        m = torch.full_like(up[:, 0], float("-inf"))
        ssum = torch.zeros_like(m)
        for c in range(C):
            mn = torch.maximum(m, up[:, c])
            ssum = ssum * torch.exp(m - mn) + torch.exp(up[:, c] - mn)
            m = mn
        lse = m + torch.log(ssum)
    else:
        lse = torch.logsumexp(up, dim=1)
    p = torch.exp(up - lse[:, None])
    onehot = F.one_hot(tc, C).permute(0, 3, 1, 2).to(dtype) * keep[:, None]
    kf = keep[:, None].double()
    I = (p.double() * onehot.double()).sum((0, 2, 3))
    P = (p.double() * (1.0 if mutate == "ignored_in_P" else kf)).sum((0, 2, 3))
    T = onehot.double().sum((0, 2, 3))
    c0 = 0 if include_background else 1
    nK = C if mutate == "K_is_C" else C - c0
    N, D = 2.0 * I + sm, P + T + sm
    dice = (1.0 - N / D)[c0:].sum() / nK
    counted = (torch.arange(C) >= c0).double()
    a0 = (N / (nK * D * D) * counted).to(dtype).view(1, C, 1, 1)
    a1 = (-(2.0 * D - N) / (nK * D * D) * counted).to(dtype).view(1, C, 1, 1)
    a = torch.where(onehot > 0, a1, a0)
    if f32:   # the kernel's sequential fp32 sum
        sap = torch.zeros_like(lse)
        for c in range(C):
            sap = sap + a[:, c] * p[:, c]
    else:
        sap = (a * p).sum(1)
    if mutate == "no_sap":
        sap = torch.zeros_like(sap)
    gd = torch.tensor(dw, dtype=dtype) * (p * (a - sap[:, None]))
    grad = torch.zeros_like(up)
    ce = torch.zeros((), dtype=torch.float64)
    if cw != 0.0:   # ce_ref.ce_closed_form, with the kernel's grouping in fp32
        w = _weights64(class_weight, C)
        wy = (w[tc] * keep)
        den = wy.sum()
        zy = up.gather(1, tc[:, None])[:, 0]
        wv = w.view(1, C, 1, 1)
        smooth_sum = ((lse[:, None].double() - up.double()) * wv).sum(1) * keep
        a_f = (torch.tensor(1.0 - eps, dtype=dtype) * wy.to(dtype))
        ce = ((a_f.double() * (lse - zy).double()).sum() + float(torch.tensor(eps / C, dtype=dtype)) * smooth_sum.sum()) / den
        inv = (1.0 / den).to(dtype)
        v = (a_f[:, None] * (p - (onehot > 0).to(dtype))) * inv
        if eps > 0:
            v = v + (torch.tensor(eps / C, dtype=dtype) * (p * w.sum().to(dtype) - wv.to(dtype))) * inv
        grad = torch.tensor(cw, dtype=dtype) * v
        loss = cw * ce + dw * dice if dw != 0.0 else cw * ce
    else:
        loss = dw * dice
    if dw != 0.0:
        grad = grad + gd
    grad = grad * keep[:, None]
    return loss, ce, dice, grad, (I, P, T)


def bounds(up, target, sums, loss, ce, dice, grad_max, dice_weight=1.0, ce_weight=1.0, smooth=1e-6, include_background=True,
           ignore_index=None, class_weight=None, label_smoothing=0.0, loss_scale=1.0):
    """dict(loss, ce, dice, grad): the error bounds of the module docstring for the fp64 reference values `loss`, `ce`,
    `dice`, `sums` = (I, P, T) and max |grad| = `grad_max` on the fp64 logits `up`.  Needs at least one kept pixel."""
    C = up.shape[1]
    t = target.long()
    keep = _keep(t, ignore_index)
    upk = up.permute(0, 2, 3, 1)[keep].double()
    lse = torch.logsumexp(upk, dim=1)
    e_pix = 4 * U * lse.abs().max().item() + 8 * U * upk.abs().max().item() + 4 * (C + 2) * U
    eps_p = e_pix + 8 * U
    I, P, T = (s.double() for s in sums)
    c0 = 0 if include_background else 1
    nK = C - c0
    sm = float(torch.tensor(float(smooth), dtype=torch.float32))
    N, D = (2.0 * I + sm)[c0:], (P + T + sm)[c0:]
    dice_b = 1.01 * 2 * eps_p * float((N / D).mean()) + 2 * U * abs(float(dice))
    A = float((torch.maximum(N, 2.0 * D - N) / (nK * D * D)).max())
    gdice_b = 1.01 * dice_weight * abs(loss_scale) * A * (13 * eps_p + (C + 12) * U)
    ce_b = gce_b = 0.0
    if ce_weight != 0:
        eps = float(label_smoothing)
        w = _weights64(class_weight, C)
        den = float(w[t[keep]].sum())
        Kce = (1.0 - eps) * float(w.max()) + eps * float(w.sum()) / C
        ce_b = e_pix * ((1.0 - eps) + eps * float(w.sum()) / C * int(keep.sum()) / den) + 6 * U * abs(float(ce))
        gce_b = Kce * (e_pix + 20 * U) * abs(loss_scale) / den
    if dice_weight == 0:
        dice_b = gdice_b = 0.0
    return dict(loss=ce_weight * ce_b + dice_weight * dice_b + 2 * U * abs(float(loss)), ce=ce_b, dice=dice_b,
                grad=ce_weight * gce_b + gdice_b + 4 * U * grad_max, e_pix=e_pix)


# ------------------------------------------------------------------ the cases of both test files
def _span_weights(C, gen):
    """log-uniform over 1e-3 .. 1e3 with both ends present (test_gpu_ce_options._weights "span")"""
    w = 10.0 ** (torch.rand(C, generator=gen) * 6.0 - 3.0)
    w[0], w[-1] = 1e-3, 1e3
    return w.float().tolist()


# name: (B, C, g, S, logits, options of the loss, what is done to the targets)
CASES = {
    "plain": (2, 5, 7, 28, "randn", dict(), dict()),
    "ragged, one counted class": (3, 2, 7, 28, "randn", dict(include_background=False), dict()),       # 2352 pixels
    "class 3 absent": (2, 5, 7, 28, "randn", dict(), dict(absent=3)),
    "class 3 absent, smooth 0": (2, 5, 7, 28, "randn", dict(smooth=0.0), dict(absent=3)),
    "ignored, weights, smoothing": (2, 17, 14, 224, "randn", dict(ignore_index=255, class_weight="span", label_smoothing=0.1),
                                    dict(frac=0.1, whole=0)),
    "logits at +-60": (1, 17, 14, 224, "big", dict(), dict()),
    "512": (2, 32, 32, 512, "randn", dict(), dict()),
    # 3200 blocks of the Dice sum pass: the fixed-order reduce of their partials runs its four-chain loop (> 3072)
    "512, 3200 sum blocks": (25, 2, 32, 512, "randn", dict(), dict()),
    # beyond the issue's list: a smooth that is visible in fp32, other weights, torch's ignore_index
    "smooth 1, weights 2 : 0.5": (2, 5, 7, 28, "randn", dict(smooth=1.0, dice_weight=0.5, ce_weight=2.0, ignore_index=-100,
                                                             include_background=False), dict(frac=0.1)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(z, target, S, C, g, B, kw, ref=(loss, ce, dice, grad, up)) of one of CASES: computed once, shared, not modified."""
    B, C, g, S, kind, kw, tk = CASES[name]
    gen = torch.Generator().manual_seed(1000 * B + 10 * C + g + len(name))
    z = torch.randn(B, C, g, g, generator=gen).float() * 3.0
    if kind == "big":
        z = (torch.rand(B, C, g, g, generator=gen) * 120.0 - 60.0).float()
    t = torch.randint(0, C, (B, S, S), generator=gen)
    kw = dict(kw)
    if kw.get("class_weight") == "span":
        kw["class_weight"] = _span_weights(C, gen)
    if "absent" in tk:
        t[t == tk["absent"]] = 0
    if "frac" in tk:
        t[torch.rand(B, S, S, generator=gen) < tk["frac"]] = kw["ignore_index"]
    if "whole" in tk:
        t[tk["whole"]] = kw["ignore_index"]
    ref = ce_dice_ref(z, t, S, **kw)
    return dict(z=z, target=t, B=B, C=C, g=g, S=S, kw=kw, ref=ref)
