"""The Lovasz-Softmax loss (Berman, Triki and Blaschko, CVPR 2018) on device planes: `lovasz_softmax_planes`, `sort_planes`
and the host-side check of the term's options (`check_options`).  Semantics, the order of equal errors and the launches:
include/vitseg_lovasz.h; the fused form on the model's logits is `ViTSegmentationModel.ce_lovasz_loss`.  There is no fall-back: a
plane that is not on the GPU is an error.
"""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import _ext, _lib

TILE = 2048   # include/vitseg_lovasz.h VITSEG_LOVASZ_TILE
MAX_SEGMENTS = 1 << 20


def _sym(name):
    return _ext.ext_symbol("lovasz", name)


def check_options(num_classes: int, weight=0.5, classes: Optional[Sequence[int]] = None, per_image=False, present=True):
    """Host-side validation of the Lovasz term's options (the kernels cannot raise).  Returns (weight, classes, per_image,
    present_only) as vitseg_lovasz_options reads them; `classes=None` is every class (the published classes='present' with
    `present=True`, 'all' without)."""
    weight = float(weight)
    if not (math.isfinite(weight) and weight >= 0.0):
        raise ValueError(f"lovasz_weight must be finite and >= 0, got {weight!r}")
    if classes is None:
        classes = list(range(num_classes))
    classes = [int(c) for c in classes]
    if not 1 <= len(classes) <= num_classes:
        raise ValueError(f"lovasz_classes must list 1..{num_classes} classes, got {len(classes)}")
    if len(set(classes)) != len(classes):
        raise ValueError(f"lovasz_classes lists a class twice: {classes}")
    for c in classes:
        if not 0 <= c < num_classes:
            raise ValueError(f"lovasz class {c} outside [0, {num_classes})")
    for name, v in (("lovasz_per_image", per_image), ("lovasz_present", present)):
        if not isinstance(v, (bool, int)) or v not in (0, 1):
            raise ValueError(f"{name} must be a bool, got {v!r}")
    return weight, classes, int(per_image), int(present)


def _segments(p: torch.Tensor, what: str) -> torch.Tensor:
    if not isinstance(p, torch.Tensor) or not p.is_cuda:
        raise ValueError(f"{what} must be a tensor on the GPU (there is no host fall-back)")
    if p.dtype != torch.float32 or p.dim() not in (1, 2):
        raise ValueError(f"{what} must be float32 [n, L] or [L], got {p.dtype} {tuple(p.shape)}")
    if p.numel() == 0 or p.numel() >= 2 ** 31:
        raise ValueError(f"{what} holds {p.numel()} pixels (1 .. 2^31 - 1)")
    q = p.contiguous().view(-1, p.shape[-1])
    if q.shape[0] > MAX_SEGMENTS:
        raise ValueError(f"{what} holds {q.shape[0]} segments (at most {MAX_SEGMENTS})")
    return q


def _truth(target, prob) -> torch.Tensor:
    if not isinstance(target, torch.Tensor) or target.dtype not in (torch.uint8, torch.bool) or target.shape != prob.shape:
        raise ValueError(f"target must be uint8 / bool of prob's shape {tuple(prob.shape)}")
    return target.to(device=prob.device, dtype=torch.uint8).contiguous()


def _planes_call(prob, truth, grad_scale, want_grad, want_order):
    """One vitseg_lovasz_planes call: (terms float[n] on the device, the gradient or None, the order or None)."""
    n, L = prob.shape
    dev = prob.device
    with torch.cuda.device(dev):
        scratch = torch.empty(int(_sym("vitseg_lovasz_planes_scratch_bytes")(n, L)), dtype=torch.uint8, device=dev)
        terms = torch.empty(n, dtype=torch.float32, device=dev)
        grad = torch.empty_like(prob) if want_grad else None
        order = torch.empty((n, L), dtype=torch.int32, device=dev) if want_order else None
        _lib.check(_sym("vitseg_lovasz_planes")(prob.data_ptr(), truth.data_ptr(), n, L, grad_scale, scratch.data_ptr(),
                                                terms.data_ptr(), grad.data_ptr() if want_grad else None,
                                                order.data_ptr() if want_order else None,
                                                torch.cuda.current_stream().cuda_stream))
    return terms, grad, order


@torch.no_grad()
def sort_planes(prob: torch.Tensor, target: torch.Tensor):
    """(terms fp32 [n], grad fp32 like prob, order int32 like prob) of `prob` fp32 [n, L] (or [L]): per segment the Lovasz
    loss, its gradient w.r.t. prob and the pixel at each rank of the stable descending order of the errors (-1 past the valid
    pixels).  `target`: uint8 / bool, 1 = the class, 255 = void."""
    q = _segments(prob, "prob")
    terms, grad, order = _planes_call(q, _truth(target, prob).view(q.shape), 1.0, True, True)
    return terms, grad.view(prob.shape), order.view(prob.shape)


class _LovaszPlanesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prob, truth):
        q = _segments(prob, "prob")
        terms, grad, _ = _planes_call(q, truth.view(q.shape), 1.0, prob.requires_grad, False)
        ctx.grad, ctx.shape = grad, prob.shape
        return terms

    @staticmethod
    def backward(ctx, dterms):
        grad, ctx.grad = ctx.grad, None
        return (grad * dterms[:, None]).view(ctx.shape) if grad is not None else None, None


def lovasz_softmax_planes(prob: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """The Lovasz loss of one class per segment on device planes, differentiable w.r.t. `prob`: `prob` fp32 [n, L] (or [L])
    probabilities of the class, `target` uint8 or bool of the same shape (1 / True = the class, 255 = void: no rank, gradient
    0).  Every row is a segment of its own.  Returns the device vector [n] of the per-segment losses (the binary trainer's
    probabilities go here: the mean of the foreground row is the published Lovasz loss of that class)."""
    _segments(prob, "prob")
    return _LovaszPlanesFn.apply(prob, _truth(target, prob))
