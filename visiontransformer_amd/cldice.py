"""The soft-clDice loss (Shit et al., CVPR 2021) on device planes: `soft_skeleton`, `soft_cldice_loss` and the host-side
check of the term's options (`check_options`).  Semantics, tie rules and launches: include/vitseg_cldice.h; the fused form on the
model's logits is `ViTSegmentationModel.ce_cldice_loss`.  There is no fall-back: a plane that is not on the GPU is an error.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import _ext, _lib

MAX_ITERS = 64   # include/vitseg_cldice.h VITSEG_CLDICE_MAX_ITERS


def _sym(name):
    return _ext.ext_symbol("cldice", name)


def _check_iters(iters) -> int:
    if isinstance(iters, bool) or not isinstance(iters, int) or not 0 <= iters <= MAX_ITERS:
        raise ValueError(f"iters must be an int in 0..{MAX_ITERS}, got {iters!r}")
    return iters


def _check_smooth(smooth) -> float:
    smooth = float(smooth)
    if not (math.isfinite(smooth) and smooth > 0.0):
        raise ValueError(f"smooth must be finite and > 0, got {smooth!r}")
    return smooth


def check_options(num_classes: int, weight=0.5, classes: Optional[Sequence[int]] = None, iters=3, smooth=1.0):
    """Host-side validation of the clDice term's options (the kernels cannot raise).  Returns (weight, classes, iters,
    smooth) as vitseg_cldice_options reads them; `classes=None` is every class but 0."""
    weight = float(weight)
    if not (math.isfinite(weight) and weight >= 0.0):
        raise ValueError(f"cldice_weight must be finite and >= 0, got {weight!r}")
    if classes is None:
        classes = list(range(1, num_classes))
        if not classes:
            raise ValueError("cldice_classes=None needs at least two classes (every class but 0)")
    classes = [int(c) for c in classes]
    if not 1 <= len(classes) <= num_classes:
        raise ValueError(f"cldice_classes must list 1..{num_classes} classes, got {len(classes)}")
    if len(set(classes)) != len(classes):
        raise ValueError(f"cldice_classes lists a class twice: {classes}")
    for c in classes:
        if not 0 <= c < num_classes:
            raise ValueError(f"cldice class {c} outside [0, {num_classes})")
    return weight, classes, _check_iters(iters), _check_smooth(smooth)


def _planes(p: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(p, torch.Tensor) or not p.is_cuda:
        raise ValueError(f"{what} must be a tensor on the GPU (there is no host fall-back)")
    if p.dtype != torch.float32 or p.dim() not in (2, 3):
        raise ValueError(f"{what} must be float32 [n, H, W] or [H, W], got {p.dtype} {tuple(p.shape)}")
    if p.numel() == 0 or p.numel() >= 2 ** 31:
        raise ValueError(f"{what} holds {p.numel()} pixels (1 .. 2^31 - 1)")
    return p.contiguous().view((-1,) + tuple(p.shape[-2:]))


@torch.no_grad()
def soft_skeleton(p: torch.Tensor, iters: int = 3) -> torch.Tensor:
    """The soft skeleton of fp32 planes [n, H, W] (or [H, W]) by `iters` rounds of min / max pooling: bit for bit the
    published soft_skel in torch's fp32.  No gradient (use `soft_cldice_loss`)."""
    iters = _check_iters(iters)
    q = _planes(p, "p")
    n, H, W = q.shape
    out = torch.empty_like(q)
    with torch.cuda.device(q.device):
        scratch = torch.empty(int(_sym("vitseg_soft_skeleton_scratch_bytes")(n, H, W)), dtype=torch.uint8, device=q.device)
        _lib.check(_sym("vitseg_soft_skeleton")(q.data_ptr(), n, H, W, iters, out.data_ptr(), scratch.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream))
    return out.view(p.shape)


def _plane_loss(prob, truth, iters, smooth, grad_scale, want_grad):
    """One vitseg_soft_cldice call: (terms float[4] on the device, the gradient or None)."""
    n, H, W = prob.shape
    dev = prob.device
    with torch.cuda.device(dev):
        scratch = torch.empty(int(_sym("vitseg_soft_cldice_scratch_bytes")(n, H, W, iters)), dtype=torch.uint8, device=dev)
        terms = torch.empty(4, dtype=torch.float32, device=dev)
        grad = torch.empty_like(prob) if want_grad else None
        _lib.check(_sym("vitseg_soft_cldice")(prob.data_ptr(), truth.data_ptr(), n, H, W, iters, smooth, grad_scale,
                                              scratch.data_ptr(), terms.data_ptr(), grad.data_ptr() if want_grad else None,
                                              torch.cuda.current_stream().cuda_stream))
    return terms, grad


class _SoftClDiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prob, truth, iters, smooth):
        q = _planes(prob, "prob")
        terms, grad = _plane_loss(q, truth, iters, smooth, 1.0, prob.requires_grad)
        ctx.grad, ctx.shape = grad, prob.shape
        return terms[0].clone()

    @staticmethod
    def backward(ctx, dloss):
        grad, ctx.grad = ctx.grad, None
        return (grad * dloss).view(ctx.shape) if grad is not None else None, None, None, None


def soft_cldice_loss(prob: torch.Tensor, target: torch.Tensor, iters: int = 3, smooth: float = 1.0) -> torch.Tensor:
    """The soft-clDice loss of one class on device planes, differentiable w.r.t. `prob`: `prob` fp32 [n, H, W] (or [H, W])
    probabilities of the class, `target` uint8 or bool of the same shape (1 / True = the class, 255 = void: no part in the
    sums, gradient 0).  The sums run over all n planes.  Returns a device scalar."""
    iters, smooth = _check_iters(iters), _check_smooth(smooth)
    _planes(prob, "prob")
    if not isinstance(target, torch.Tensor) or target.dtype not in (torch.uint8, torch.bool) or target.shape != prob.shape:
        raise ValueError(f"target must be uint8 / bool of prob's shape {tuple(prob.shape)}")
    truth = target.to(device=prob.device, dtype=torch.uint8).contiguous()
    return _SoftClDiceFn.apply(prob, truth, iters, smooth)
