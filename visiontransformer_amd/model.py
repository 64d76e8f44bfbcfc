"""`ViTSegmentationModel` -- drop-in mirror of the reference class
(/root/reference/model/CE/classes.py:221-262; byte-identical copy at model/PAED/classes.py:372-413).

Same positional constructor, same `forward(x[B,3,H,W]) -> logits[B,C,H,W]`, same state-dict key
schema, same ValueErrors; the arithmetic runs in libvitseg.so (hand-written gfx950 kernels) on
the tensor's HIP stream.  PyTorch is storage only: one flat fp32 parameter arena (a single
nn.Parameter), a cached workspace tensor and the output tensor.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from collections import OrderedDict
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _ext, _lib, params as _params
from .config import ViTSegConfig

_PRECISION = {"fp32": _lib.F32, "f32": _lib.F32, "float32": _lib.F32, "bf16": _lib.BF16, "bfloat16": _lib.BF16,
              "fp16": _lib.F16, "f16": _lib.F16, "float16": _lib.F16, "half": _lib.F16,
              "fp32x3": _lib.F32X3, "f32x3": _lib.F32X3}


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def check_ce_options(num_classes: int, ignore_index=None, class_weight=None, label_smoothing: float = 0.0):
    """Host-side validation of `ce_loss`'s options (the kernels cannot raise).  Returns None when all three are at their
    defaults -- the caller then takes the plain calls -- else (ignore_index or None, fp32 CPU tensor [C] or None, eps).
    ValueError: an `ignore_index` that is not an integer (of int64 range), a `class_weight` that is not `num_classes`
    finite values >= 0, a `label_smoothing` outside [0, 1]."""
    if ignore_index is not None:
        if isinstance(ignore_index, bool) or not isinstance(ignore_index, numbers.Integral):
            raise ValueError(f"ignore_index must be an integer or None, got {ignore_index!r}")
        ignore_index = int(ignore_index)
        if not -2 ** 63 <= ignore_index < 2 ** 63:
            raise ValueError(f"ignore_index {ignore_index} does not fit int64")
    try:
        eps = float(label_smoothing)
    except (TypeError, ValueError):
        raise ValueError(f"label_smoothing must be a number in [0, 1], got {label_smoothing!r}") from None
    if not 0.0 <= eps <= 1.0:   # (a NaN fails both comparisons)
        raise ValueError(f"label_smoothing must lie in [0, 1], got {label_smoothing!r}")
    w = None
    if class_weight is not None:
        try:
            w = torch.as_tensor(class_weight).detach().to("cpu", torch.float64)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"class_weight must be a sequence or tensor of {num_classes} numbers") from None
        if w.dim() != 1 or w.numel() != num_classes:
            raise ValueError(f"class_weight must hold one weight per class ({num_classes}), got shape {tuple(w.shape)}")
        w = w.to(torch.float32)   # what the kernels read: a value beyond the fp32 range is not finite there
        if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
            raise ValueError("class_weight must be finite and >= 0")
    if ignore_index is None and w is None and eps == 0.0:
        return None
    return ignore_index, w, eps


def check_dice_options(num_classes: int, dice_weight=1.0, ce_weight=1.0, smooth=1e-6, include_background=True):
    """Host-side validation of `ce_dice_loss`'s Dice options (the kernels cannot raise).  Returns (dice_weight, ce_weight,
    smooth, include_background) as the fp32 values and the flag the kernels read.  ValueError: a weight or `smooth` that is
    not a finite number >= 0 (in fp32), both weights 0, `include_background=False` with fewer than 2 classes."""
    out = []
    for name, v in (("dice_weight", dice_weight), ("ce_weight", ce_weight), ("smooth", smooth)):
        try:
            f = float(torch.tensor(float(v), dtype=torch.float32))   # what the kernels read
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}") from None
        if not (0.0 <= f < float("inf")):   # (a NaN fails both comparisons)
            raise ValueError(f"{name} must be a finite number >= 0, got {v!r}")
        out.append(f)
    if out[0] == 0.0 and out[1] == 0.0:
        raise ValueError("dice_weight and ce_weight are both 0: there is no loss to form")
    if not include_background and num_classes < 2:
        raise ValueError("include_background=False needs at least 2 classes")
    return out[0], out[1], out[2], bool(include_background)


def check_hard_options(focal_gamma=0.0, ohem_thresh=None, ohem_min_kept=0, ohem_keep_fraction=0.0):
    """Host-side validation of `ce_loss`'s focal / OHEM options (the kernels cannot raise).  Returns None when all four are
    at their defaults -- the caller then takes the calls it took before -- else (gamma, loss_thresh, min_kept, keep_q16) as
    vitseg_hard_options reads them: the fp32 exponent, the threshold as the fp32 CE value float32(-log(ohem_thresh)) (+inf
    for None), the floor as a count and as rint(ohem_keep_fraction * 65536).
    ValueError: a `focal_gamma` that is not a finite number >= 0 (in fp32), an `ohem_thresh` that is not None or a
    probability in (0, 1], an `ohem_min_kept` that is not an integer in [0, 2^63), an `ohem_keep_fraction` outside [0, 1]."""
    for name, v in (("focal_gamma", focal_gamma), ("ohem_thresh", ohem_thresh), ("ohem_keep_fraction", ohem_keep_fraction)):
        if isinstance(v, (str, bytes, bool)):
            raise ValueError(f"{name} must be a number, got {v!r}")
    try:
        gamma = float(torch.tensor(float(focal_gamma), dtype=torch.float32))   # what the kernels read
    except (TypeError, ValueError, RuntimeError):
        raise ValueError(f"focal_gamma must be a finite number >= 0, got {focal_gamma!r}") from None
    if not (0.0 <= gamma < float("inf")):   # (a NaN fails both comparisons)
        raise ValueError(f"focal_gamma must be a finite number >= 0, got {focal_gamma!r}")
    loss_thresh = float("inf")
    if ohem_thresh is not None:
        try:
            t = float(ohem_thresh)
        except (TypeError, ValueError):
            raise ValueError(f"ohem_thresh must be None or a probability in (0, 1], got {ohem_thresh!r}") from None
        if not (0.0 < t <= 1.0):
            raise ValueError(f"ohem_thresh must be None or a probability in (0, 1], got {ohem_thresh!r}")
        loss_thresh = float(torch.tensor(-math.log(t) + 0.0, dtype=torch.float32))   # (+ 0.0: -log(1) is -0.0)
    if isinstance(ohem_min_kept, bool) or not isinstance(ohem_min_kept, numbers.Integral) or not 0 <= int(ohem_min_kept) < 2 ** 63:
        raise ValueError(f"ohem_min_kept must be an integer in [0, 2^63), got {ohem_min_kept!r}")
    try:
        frac = float(ohem_keep_fraction)
    except (TypeError, ValueError):
        raise ValueError(f"ohem_keep_fraction must be a number in [0, 1], got {ohem_keep_fraction!r}") from None
    if not (0.0 <= frac <= 1.0):
        raise ValueError(f"ohem_keep_fraction must be a number in [0, 1], got {ohem_keep_fraction!r}")
    keep_q16 = int(round(frac * 65536.0))   # round half to even: rint
    if gamma == 0.0 and ohem_thresh is None and int(ohem_min_kept) == 0 and frac == 0.0:
        return None
    return gamma, loss_thresh, int(ohem_min_kept), keep_q16


class _LogitsFn(torch.autograd.Function):
    """logits = forward(x) with libvitseg's backward: d loss / d logits -> d loss / d arena."""

    @staticmethod
    def forward(ctx, arena, model, x, interp=False):
        ctx.model, ctx.x, ctx.interp = model, x, interp
        ctx.drop = model._next_dropout()
        return model._forward_train(x, want_logits=True, drop=ctx.drop, interp=interp)

    @staticmethod
    def backward(ctx, dlogits):
        grads, _ = ctx.model._backward(ctx.x, grad_logits=dlogits.to(torch.float32).contiguous(), drop=ctx.drop,
                                       interp=ctx.interp)
        return ctx.model._deliver_grad(grads), None, None, None


class _CELossFn(torch.autograd.Function):
    """Fused CE: forward + loss + backward in one go (no [B,C,S,S] logits tensor is returned).  With `grad_scale` the
    factor is folded into the CE gradient at its source (vitseg_backward's loss_scale) and the upstream gradient of the
    returned loss is taken to be 1: no arena-sized multiply.  The gradient is delivered by `_deliver_grad` (installed as
    `arena.grad` or added to it), not returned to autograd: AccumulateGrad would clone an arena-sized tensor it cannot
    steal (the model keeps a reference to its persistent buffer)."""

    @staticmethod
    def forward(ctx, arena, model, x, target, grad_scale, interp=False, ce_opts=None):
        drop = model._next_dropout()
        model._forward_train(x, want_logits=False, drop=drop, interp=interp)
        grads, loss = model._backward(x, target=target, drop=drop, loss_scale=1.0 if grad_scale is None else grad_scale,
                                      interp=interp, ce_opts=ce_opts)
        ctx.grads, ctx.model = grads, model
        ctx.prescaled = grad_scale is not None
        return loss

    @staticmethod
    def backward(ctx, dloss):
        grads, ctx.grads = ctx.grads, None
        if not ctx.prescaled:
            grads.mul_(dloss)   # in place: the buffer is ours until it is delivered
        return ctx.model._deliver_grad(grads), None, None, None, None, None, None


class _HardCELossFn(torch.autograd.Function):
    """`_CELossFn` for the focal / OHEM loss (vitseg_backward_hard): returns (loss, stats), stats the device int64[4]
    {n_valid, k, |H|, bits of tau} (no gradient); the arena gradient is delivered the same way."""

    @staticmethod
    def forward(ctx, arena, model, x, target, grad_scale, interp, ce_opts, hard_opts):
        drop = model._next_dropout()
        model._forward_train(x, want_logits=False, drop=drop, interp=interp)
        grads, (loss, stats) = model._backward(x, target=target, drop=drop, loss_scale=1.0 if grad_scale is None else grad_scale,
                                               interp=interp, ce_opts=ce_opts, hard_opts=hard_opts)
        ctx.grads, ctx.model = grads, model
        ctx.prescaled = grad_scale is not None
        ctx.mark_non_differentiable(stats)
        return loss, stats

    @staticmethod
    def backward(ctx, dloss, _dstats):
        grads, ctx.grads = ctx.grads, None
        if not ctx.prescaled:
            grads.mul_(dloss)   # in place: the buffer is ours until it is delivered
        return ctx.model._deliver_grad(grads), None, None, None, None, None, None, None


class _CEClDiceLossFn(torch.autograd.Function):
    """`_CEDiceLossFn` with the soft-clDice term (vitseg_backward_cldice) or, `cld_opts` being an `_ext.CLovaszOptions`, the
    Lovasz-Softmax term (vitseg_backward_lovasz): returns the device float[4] {loss, CE, dice, cldice or lovasz}; only
    element 0 carries a gradient."""

    @staticmethod
    def forward(ctx, arena, model, x, target, grad_scale, interp, ce_opts, dice_opts, cld_opts):
        drop = model._next_dropout()
        model._forward_train(x, want_logits=False, drop=drop, interp=interp)
        grads, terms = model._backward(x, target=target, drop=drop, loss_scale=1.0 if grad_scale is None else grad_scale,
                                       interp=interp, ce_opts=ce_opts, dice_opts=dice_opts, cld_opts=cld_opts)
        ctx.grads, ctx.model = grads, model
        ctx.prescaled = grad_scale is not None
        return terms

    @staticmethod
    def backward(ctx, dterms):
        grads, ctx.grads = ctx.grads, None
        if not ctx.prescaled:
            grads.mul_(dterms[0])   # in place: the buffer is ours until it is delivered
        return ctx.model._deliver_grad(grads), None, None, None, None, None, None, None, None


class _CEDiceLossFn(torch.autograd.Function):
    """`_CELossFn` for ce_weight CE + dice_weight dice (vitseg_backward_dice): returns the device float[3] {loss, CE, dice};
    only element 0 carries a gradient (the other two are reported values), delivered the same way."""

    @staticmethod
    def forward(ctx, arena, model, x, target, grad_scale, interp, ce_opts, dice_opts):
        drop = model._next_dropout()
        model._forward_train(x, want_logits=False, drop=drop, interp=interp)
        grads, terms = model._backward(x, target=target, drop=drop, loss_scale=1.0 if grad_scale is None else grad_scale,
                                       interp=interp, ce_opts=ce_opts, dice_opts=dice_opts)
        ctx.grads, ctx.model = grads, model
        ctx.prescaled = grad_scale is not None
        return terms

    @staticmethod
    def backward(ctx, dterms):
        grads, ctx.grads = ctx.grads, None
        if not ctx.prescaled:
            grads.mul_(dterms[0])   # in place: the buffer is ours until it is delivered
        return ctx.model._deliver_grad(grads), None, None, None, None, None, None, None


class ViTSegmentationModel(nn.Module):
    def __init__(self, num_classes, patch_size, hidden_size, num_hidden_layers, num_attention_heads, *,
                 image_size: int = 224, intermediate_size: int = 3072, precision: str = "fp32",
                 dropout: float = 0.1, layer_norm_eps: float = 1e-12, device=None):
        super().__init__()
        # layer_norm_eps: 1e-12 is the reference's (configuration_vit.py:58); a checkpoint trained with another (timm: 1e-6) sets it
        self.cfg = ViTSegConfig(num_classes, patch_size, hidden_size, num_hidden_layers, num_attention_heads,
                                image_size=image_size, intermediate_size=intermediate_size, layer_norm_eps=float(layer_norm_eps))
        self.precision = _PRECISION[precision]
        # hidden_dropout_prob = attention_probs_dropout_prob = 0.1 in the reference (classes.py:233-234); active only
        # in train() mode with autograd on, like nn.Dropout.  `dropout_seed` + a step counter select the masks.
        self.dropout = float(dropout)
        self.dropout_seed = 0x5EED
        self._dropout_step = 0
        # data-parallel gradient exchange: "overlap" = bucketed all-reduce behind events inside the backward,
        # "after" = one flat all-reduce by the caller (dist.allreduce_grads), see dist.sync_grads
        self.grad_sync = "overlap"
        self.grad_bucket_mb = 48.0
        self._buckets = None
        self._grads_reduced = False
        self._require_sync = True
        self._graphs = {}   # (batch, with logits) -> captured hipGraph of the forward (predict_mask_graphed)
        n = _lib.param_count(self.cfg)  # validates the configuration (ValueError on unsupported shapes)
        self.arena = nn.Parameter(torch.zeros(n, dtype=torch.float32, device=device))
        self._views: Optional[Dict[str, torch.Tensor]] = None
        self._views_key = None
        self._ws = {}
        self._arena_bf16 = None
        self._bf16_version = None
        self.reset_parameters()

    # ------------------------------------------------------------------ parameters
    def named_views(self) -> Dict[str, torch.Tensor]:
        """reference parameter name -> live view into the arena."""
        key = (self.arena.data_ptr(), self.arena.device)
        if self._views is None or self._views_key != key:
            self._views = _params.arena_views(self.cfg, self.arena.data)
            self._views_key = key
        return self._views

    @torch.no_grad()
    def reset_parameters(self, seed: int = 0):
        """Initialisers of the reference: HF ViT init (N(0, 0.02) weights, zero biases, LayerNorm 1/0,
        trunc-normal cls/pos; modeling_vit.py:324-332) and torch's Conv2d default for seg_head."""
        g = torch.Generator().manual_seed(seed)
        self.arena.zero_()
        for name, v in self.named_views().items():
            if name.startswith("seg_head."):
                w = self.named_views()[name.rsplit(".", 1)[0] + ".weight"]
                fan_in = w.shape[1] * w.shape[2] * w.shape[3]
                bound = 1.0 / fan_in ** 0.5
                v.copy_((torch.rand(v.shape, generator=g) * 2 - 1) * bound)
            elif "layernorm" in name:
                v.fill_(1.0 if name.endswith("weight") else 0.0)
            elif name.endswith(".bias"):
                v.zero_()
            elif name.endswith("cls_token") or name.endswith("position_embeddings"):
                v.copy_(torch.nn.init.trunc_normal_(torch.empty(v.shape), std=0.02, generator=g))
            else:
                v.copy_(torch.randn(v.shape, generator=g) * 0.02)

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        out = OrderedDict() if destination is None else destination
        for k, v in self.named_views().items():
            out[prefix + k] = v if keep_vars else v.detach().clone()
        return out

    @torch.no_grad()
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        views = self.named_views()
        seen, unexpected = set(), []
        for k, v in state_dict.items():
            ck = _params.canonical_key(k)
            if ck.startswith("backbone.pooler."):
                continue  # computed then discarded by the reference (modeling_vit.py:386)
            if ck not in views:
                unexpected.append(k)
                continue
            if tuple(v.shape) != tuple(views[ck].shape):
                raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(v.shape)} vs model "
                                   f"{tuple(views[ck].shape)}")
            views[ck].copy_(torch.as_tensor(v).to(views[ck].device, torch.float32))
            seen.add(ck)
        missing = [k for k in views if k not in seen]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict: missing {missing}, unexpected {unexpected}")
        self._bf16_version = None
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def _apply(self, fn, *a, **kw):
        r = super()._apply(fn, *a, **kw)
        self._views = None
        self._ws.clear()
        self._arena_bf16 = None
        self._bf16_version = None
        return r

    # ------------------------------------------------------------------ launch plumbing
    def _check_input(self, x: torch.Tensor, interp: bool = False):
        """`interp` (interpolate_pos_encoding): any square input whose side is a multiple of the patch size; the
        position table is resampled to its grid (HF ViTEmbeddings.interpolate_pos_encoding)."""
        cfg = self.cfg
        if x.dim() != 4:
            raise ValueError(f"expected a [B, C, H, W] tensor, got shape {tuple(x.shape)}")
        if x.shape[1] != cfg.num_channels:  # modeling_vit.py:63-68
            raise ValueError("Make sure that the channel dimension of the pixel values match with the one set in the "
                             f"configuration. Expected {cfg.num_channels} but got {x.shape[1]}.")
        if interp:
            H, W, P = x.shape[2], x.shape[3], cfg.patch_size
            if H != W:   # the reference's h = w = sqrt(num_patches) (classes.py:253-255) cannot reshape other grids
                raise ValueError(f"interpolate_pos_encoding needs a square input, got {H}*{W}.")
            if H < P or H % P:
                raise ValueError(f"Input image size ({H}*{W}) is not a positive multiple of the patch size {P}.")
        elif x.shape[2] != cfg.image_size or x.shape[3] != cfg.image_size:  # modeling_vit.py:152-156
            raise ValueError(f"Input image size ({x.shape[2]}*{x.shape[3]}) doesn't match model "
                             f"({cfg.image_size}*{cfg.image_size}).")
        if not x.is_cuda or x.device != self.arena.device:
            raise RuntimeError("ViTSegmentationModel runs on the MI355X only: move the model and the input to the "
                               f"same HIP device (input on {x.device}, parameters on {self.arena.device}). "
                               "There is no CPU fallback.")

    def forward_route(self, batch: int, image_size: Optional[int] = None) -> str:
        """"small" / "large": the kernel family an inference forward of this batch size runs on (results are bit-identical for
        every batch size inside one route); `image_size`: the input's side (interpolate_pos_encoding), default the model's."""
        return _lib.forward_route(self.cfg, batch, self.precision, image_size)

    def _size_in(self, x: torch.Tensor, interp: bool) -> int:
        return int(x.shape[-1]) if interp else self.cfg.image_size

    def workspace(self, batch: int, image_size: Optional[int] = None) -> torch.Tensor:
        S = self.cfg.image_size if image_size is None else int(image_size)
        key = (batch, self.precision, S)
        ws = self._ws.get(key)
        if ws is None:
            nbytes = _lib.query_workspace(self.cfg, batch, self.precision, S)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.arena.device)
            self._ws = {key: ws}  # keep one: a new batch size replaces the old workspace
        return ws

    def _bf16_arena(self):
        """Shadow of the arena in the operand format of `self.precision`: bf16 / IEEE half (2 bytes per value) or, for
        fp32x3, the pre-split (hi | lo halves) image with the fp32 arena's size and offsets.  Refreshed when the fp32
        master changes."""
        if self.precision == _lib.F32:
            return None
        ver = (self.arena._version, self.arena.data_ptr())
        if self._arena_bf16 is None or self._bf16_version != ver:
            dt, cast = {_lib.BF16: (torch.bfloat16, _lib.lib().vitseg_cast_params_bf16),
                        _lib.F16: (torch.float16, _lib.lib().vitseg_cast_params_f16),
                        _lib.F32X3: (torch.float32, _lib.lib().vitseg_cast_params_split)}[self.precision]
            if self._arena_bf16 is None:
                self._arena_bf16 = torch.empty(self.arena.numel(), dtype=dt, device=self.arena.device)
            _lib.check(cast(self.arena.data_ptr(), self._arena_bf16.data_ptr(), self.arena.numel(),
                            torch.cuda.current_stream().cuda_stream))
            self._bf16_version = ver
        return self._arena_bf16

    def _run(self, x: torch.Tensor, want_logits: bool, want_mask: bool, ws: Optional[torch.Tensor] = None,
             interp: bool = False):
        self._check_input(x, interp)
        x = x.to(torch.float32).contiguous()  # modeling_vit.py:369-371 casts to the weight dtype
        B, S, Cc = x.shape[0], self._size_in(x, interp), self.cfg.num_classes
        logits = torch.empty((B, Cc, S, S), dtype=torch.float32, device=x.device) if want_logits else None
        mask = torch.empty((B, S, S), dtype=torch.uint8, device=x.device) if want_mask else None
        if ws is None:
            ws = self.workspace(B, S)
        lp = self._bf16_arena()
        cfg = C.byref(_lib.CConfig.from_config(self.cfg))
        with torch.cuda.device(x.device):
            stream = torch.cuda.current_stream().cuda_stream
            if S == self.cfg.image_size:
                rc = _lib.lib().vitseg_forward(cfg, self.arena.data_ptr(), _ptr(lp), x.data_ptr(), B, self.precision,
                                               _ptr(logits), _ptr(mask), ws.data_ptr(), ws.numel(), stream)
            else:
                rc = _lib.symbol("vitseg_forward_at")(cfg, S, self.arena.data_ptr(), _ptr(lp), x.data_ptr(), B,
                                                      self.precision, _ptr(logits), _ptr(mask), ws.data_ptr(),
                                                      ws.numel(), stream)
        _lib.check(rc)
        return logits, mask

    # ------------------------------------------------------------------ training plumbing
    def _train_workspace(self, batch: int, image_size: Optional[int] = None) -> torch.Tensor:
        S = self.cfg.image_size if image_size is None else int(image_size)
        key = ("train", batch, S)
        ws = self._ws.get(key)
        if ws is None:
            ws = torch.empty(_lib.train_workspace(self.cfg, batch, self.precision, S), dtype=torch.uint8,
                             device=self.arena.device)
            self._ws = {key: ws}
        return ws

    def _next_dropout(self):
        """(p, seed) of the next training forward; p = 0 outside train() mode."""
        if not self.training or self.dropout <= 0.0:
            return (0.0, 0)
        self._dropout_step += 1
        rank = torch.distributed.get_rank() if torch.distributed.is_available() and torch.distributed.is_initialized() else 0
        return (self.dropout, (self.dropout_seed * 0x9E3779B97F4A7C15 + self._dropout_step * 0x100000001B3 + rank) & (2 ** 64 - 1))

    def _forward_train(self, x: torch.Tensor, want_logits: bool, drop=(0.0, 0), interp: bool = False):
        self._check_input(x, interp)
        x = x.to(torch.float32).contiguous()
        B, S = x.shape[0], self._size_in(x, interp)
        ws = self._train_workspace(B, S)
        logits = torch.empty((B, self.cfg.num_classes, S, S), dtype=torch.float32, device=x.device) \
            if want_logits else None
        args = (self.arena.data_ptr(), _ptr(self._bf16_arena()), x.data_ptr(), B, self.precision, drop[0], drop[1],
                _ptr(logits), ws.data_ptr(), ws.numel())
        cfg = C.byref(_lib.CConfig.from_config(self.cfg))
        with torch.cuda.device(x.device):
            stream = torch.cuda.current_stream().cuda_stream
            if S == self.cfg.image_size:
                _lib.check(_lib.lib().vitseg_forward_train(cfg, *args, stream))
            else:
                _lib.check(_lib.symbol("vitseg_forward_train_at")(cfg, S, *args, stream))
        return logits

    def no_sync(self):
        """Context manager for gradient accumulation (what DDP's `no_sync` is for): backwards inside it only accumulate
        locally; the all-reduce happens once, on the first backward outside (`dist.sync_grads` after it)."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            old, self._require_sync = self._require_sync, False
            try:
                yield
            finally:
                self._require_sync = old
        return ctx()

    def _overlap_active(self) -> bool:
        """Bucketed all-reduce inside the backward: "overlap" = whenever a process group with > 1 rank exists,
        "force" = also with one rank (tests), "after" = never (callers use dist.allreduce_grads).  Never inside
        `no_sync()`, and never while a locally accumulated gradient is pending (`arena.grad` set): the kernels write
        THIS micro-batch's gradient, the sum over micro-batches only exists after autograd has accumulated it, so that
        step is reduced once, flat, by `dist.sync_grads`."""
        import torch.distributed as td
        if not self._require_sync or self.arena.grad is not None:
            return False
        if self.grad_sync == "force":
            return td.is_available() and td.is_initialized()
        return self.grad_sync == "overlap" and td.is_available() and td.is_initialized() and td.get_world_size() > 1

    def _bucket_state(self):
        if self._buckets is None:
            from .dist import BucketReducer
            ranges = _lib.grad_buckets(self.cfg)
            events = [torch.cuda.Event() for _ in ranges]
            for e in events:
                e.record()  # instantiates the hipEvent_t so its handle can cross the C ABI
            handles = (C.c_void_p * len(events))(*[e.cuda_event for e in events])
            self._buckets = (BucketReducer(ranges, self.grad_bucket_mb), events, handles, torch.cuda.Stream())
        return self._buckets

    def _take_grad_buffer(self) -> torch.Tensor:
        """The arena-sized buffer vitseg_backward writes: ONE persistent tensor, reused step after step.  It cannot be
        reused while it is still somebody's gradient: handed to an autograd node whose backward has not run yet
        (`_grad_busy`, cleared by `_release_grad_buffer`), or installed as `arena.grad` (accumulation pending, or
        `zero_grad(set_to_none=False)`); then this call gets a temporary of its own."""
        buf = getattr(self, "_grad_buf", None)
        pending = self.arena.grad
        usable = (buf is not None and buf.shape == self.arena.shape and buf.device == self.arena.device
                  and not getattr(self, "_grad_busy", False)
                  and (pending is None or pending.data_ptr() != buf.data_ptr()))
        if usable:
            self._grad_busy = True
            return buf
        fresh = torch.empty_like(self.arena.data)
        if buf is None or buf.shape != self.arena.shape or buf.device != self.arena.device:
            self._grad_buf, self._grad_busy = fresh, True
        return fresh

    def _release_grad_buffer(self, grads: torch.Tensor) -> None:
        if getattr(self, "_grad_buf", None) is not None and grads.data_ptr() == self._grad_buf.data_ptr():
            self._grad_busy = False

    def _deliver_grad(self, grads: torch.Tensor) -> None:
        """Hands d loss / d arena to the parameter from inside an autograd backward and returns None for autograd (= no
        gradient through the graph edge): with no gradient pending, the buffer vitseg_backward wrote BECOMES `arena.grad`
        -- no copy; `_take_grad_buffer` will not hand it out again while it is installed -- otherwise it is added to the
        pending one (gradient accumulation), after which the buffer is free again."""
        with torch.no_grad():
            if self.arena.grad is None:
                self.arena.grad = grads
            else:
                self.arena.grad.add_(grads)
        self._release_grad_buffer(grads)
        return None

    def _backward(self, x: torch.Tensor, target: Optional[torch.Tensor] = None,
                  grad_logits: Optional[torch.Tensor] = None, drop=(0.0, 0), loss_scale: float = 1.0,
                  interp: bool = False, ce_opts=None, dice_opts=None, hard_opts=None, cld_opts=None):
        """`ce_opts`: a `_lib.CCEOptions` from `_ce_options` (fused CE only), or None for the plain calls.  `dice_opts`: a
        `_lib.CDiceOptions` from `_dice_options` (fused loss only): the second value returned is then the device float[3]
        {loss, CE, dice} of vitseg_backward_dice instead of the scalar loss.  `hard_opts`: an `_ext.CHardOptions` from
        `_hard_options` (fused loss only, not with `dice_opts`): the second value is then (loss, the device int64[4] stats
        of vitseg_backward_hard).  `cld_opts`: an `_ext.CClDiceOptions` from `_cldice_options` (fused loss only, `dice_opts`
        optional, not with `hard_opts`): the second value is the device float[4] {loss, CE, dice, cldice} of
        vitseg_backward_cldice; an `_ext.CLovaszOptions` from `_lovasz_options` in its place: {loss, CE, dice, lovasz} of
        vitseg_backward_lovasz."""
        x = x.to(torch.float32).contiguous()
        B, S = x.shape[0], self._size_in(x, interp)
        ws = self._train_workspace(B, S)
        grads = self._take_grad_buffer()
        loss = torch.zeros((), dtype=torch.float32, device=x.device) if target is not None else None
        overlap = self._overlap_active()
        with torch.cuda.device(x.device):
            reducer, events, handles, comm = self._bucket_state() if overlap else (None, None, None, None)
            args = (self.arena.data_ptr(), _ptr(self._bf16_arena()), x.data_ptr(), B, self.precision, drop[0], drop[1],
                    _ptr(target), int(target is not None and target.dtype == torch.uint8), _ptr(grad_logits),
                    grads.data_ptr(), _ptr(loss), float(loss_scale), handles, ws.data_ptr(), ws.numel(),
                    torch.cuda.current_stream().cuda_stream)
            cfg = C.byref(_lib.CConfig.from_config(self.cfg))
            if cld_opts is not None:
                terms = torch.zeros(4, dtype=torch.float32, device=x.device)
                entry = (("lovasz", "vitseg_backward_lovasz") if isinstance(cld_opts, _ext.CLovaszOptions)
                         else ("cldice", "vitseg_backward_cldice"))
                _lib.check(_ext.ext_symbol(*entry)(
                    cfg, S, *args, C.byref(ce_opts) if ce_opts is not None else None,
                    C.byref(dice_opts) if dice_opts is not None else None, C.byref(cld_opts), terms.data_ptr()))
                loss = terms
            elif dice_opts is not None:
                terms = torch.zeros(3, dtype=torch.float32, device=x.device)
                _lib.check(_lib.symbol("vitseg_backward_dice")(
                    cfg, S, *args, C.byref(ce_opts) if ce_opts is not None else None, C.byref(dice_opts), terms.data_ptr()))
                loss = terms
            elif hard_opts is not None:
                stats = torch.zeros(4, dtype=torch.int64, device=x.device)
                _lib.check(_ext.ext_symbol("hardloss", "vitseg_backward_hard")(
                    cfg, S, *args, C.byref(ce_opts) if ce_opts is not None else None, C.byref(hard_opts), stats.data_ptr()))
                loss = (loss, stats)
            elif ce_opts is not None:
                _lib.check(_lib.symbol("vitseg_backward_opts")(cfg, S, *args, C.byref(ce_opts)))
            elif S == self.cfg.image_size:
                _lib.check(_lib.lib().vitseg_backward(cfg, *args))
            else:
                _lib.check(_lib.symbol("vitseg_backward_at")(cfg, S, *args))
            if overlap:
                # the whole backward is enqueued by now; each ring starts when its bucket's event fires and the
                # compute stream only rejoins after the last one (what DDP's finalize does)
                for w in reducer.reduce(grads, events, comm):
                    w.wait()
                self._grads_reduced = True
        return grads, loss

    def _needs_grad(self) -> bool:
        return torch.is_grad_enabled() and self.arena.requires_grad

    # ------------------------------------------------------------------ reference surface
    def forward(self, x: torch.Tensor, interpolate_pos_encoding: bool = False) -> torch.Tensor:
        """logits [B, C, H, W] (model/CE/classes.py:246-262).  Differentiable w.r.t. the parameters when
        autograd is on (the backward runs in libvitseg, see vitseg_backward).  In train() mode dropout
        (`self.dropout`, reference 0.1) is applied at the four HF sites with a counter-based generator.
        `interpolate_pos_encoding` (HF ViTModel.forward's keyword): any square input whose side is a multiple of the
        patch size; the position table, which keeps the model's geometry, is resampled bicubically to the input's
        patch grid on every call, and its gradient flows back to the table (vitseg_forward_at / vitseg_backward_at)."""
        interp = bool(interpolate_pos_encoding)
        if self._needs_grad():
            return _LogitsFn.apply(self.arena, self, x, interp)
        logits, _ = self._run(x, True, False, interp=interp)
        return logits

    @torch.no_grad()
    def predict_mask(self, x: torch.Tensor, return_logits: bool = False, interpolate_pos_encoding: bool = False):
        """uint8 [B, H, W] = argmax_c sigmoid(logits) with first-index ties, i.e. the reference scripts'
        `logits.sigmoid()` + `argmax` (model/CE/testViTModel.py:122-126), fused into the decoder tail.
        `interpolate_pos_encoding`: as in `forward`."""
        logits, mask = self._run(x, return_logits, True, interp=bool(interpolate_pos_encoding))
        return (mask, logits) if return_logits else mask

    def _lowres_and_mask(self, x: torch.Tensor, interp: bool = False):
        """(lowres fp32 [B, C, g, g], mask uint8 [B, S, S]) of one encoder pass: the forward that stops at the head output
        (vitseg_forward_lowres) and a one-tile blend, whose single-tile rule returns the bilinear value unchanged -- the
        mask is `predict_mask`'s bit for bit, and no full-size logits are written."""
        self._check_input(x, interp)
        S, B = self._size_in(x, interp), int(x.shape[0])
        plan = self._window_lowres(x.to(torch.float32), False, S, S, "uniform", B)
        return plan["lowres"], self._window_blend(plan, False, True)

    @torch.no_grad()
    def predict_confidence(self, x: torch.Tensor, kind: str = "prob", quantised: bool = False,
                           interpolate_pos_encoding: bool = False):
        """(mask uint8 [B, H, W], conf [B, H, W]): `predict_mask`'s mask and every pixel's score (confidence.confidence_map:
        fp32 p, or uint16 q = rint(p * 65535) with `quantised`).  kind "prob": the sigmoid that won, exactly
        `logits.sigmoid().max(dim=1).values` of `predict_mask(return_logits=True)`'s logits; "margin": its lead over the best
        other class.  The encoder runs once and the scores are re-generated from the low-res head output: the full-size
        logits are never written."""
        from . import confidence as _conf
        if kind not in _conf.KINDS:
            raise ValueError(f"kind must be one of {sorted(_conf.KINDS)}, got {kind!r}")
        lowres, mask = self._lowres_and_mask(x, bool(interpolate_pos_encoding))
        return mask, _conf.confidence_map(lowres, mask, kind=kind, quantised=quantised)

    @torch.no_grad()
    def pr_counts(self, x: torch.Tensor, gt, cls: int = 1, bins: int = 256, tolerance=0, ignore_label=None, kind: str = "prob",
                  interpolate_pos_encoding: bool = False):
        """The precision-recall counts of class `cls`' score map against the ground truth `gt` (uint8 [B, H, W]) over all
        thresholds (curves.pr_counts: int64 numpy [B, bins, 3] of (pred, hit, found), `tolerance` in pixels): the forward that
        stops at the head output (vitseg_forward_lowres) and one launch that re-generates the scores from it; neither the
        full-size logits nor a mask are written.  `curves.summary` turns the counts into ODS, OIS and AP."""
        from . import curves as _curves
        _curves.check_options(cls, bins, tolerance, ignore_label)
        interp = bool(interpolate_pos_encoding)
        self._check_input(x, interp)
        S, B = self._size_in(x, interp), int(x.shape[0])
        lowres = self._window_lowres(x.to(torch.float32), False, S, S, "uniform", B)["lowres"]
        return _curves.pr_counts(lowres, gt, cls=cls, bins=bins, tolerance=tolerance, ignore_label=ignore_label, kind=kind)

    def _lowres_and_threshold(self, x: torch.Tensor, cls, threshold, low, connectivity, kind, over_argmax, interp: bool = False):
        """(lowres fp32 [B, C, g, g], mask uint8 [B, S, S]) of one encoder pass: the forward that stops at the head output and
        decide.threshold_mask on it -- over `_lowres_and_mask`'s argmax mask with `over_argmax`, else over nothing (no other
        mask is written).  A kept pixel states decide.check_model_options' value."""
        from . import decide as _decide
        value = _decide.check_model_options(self.cfg.num_classes, cls, threshold, low, connectivity, kind)
        if over_argmax:
            lowres, base = self._lowres_and_mask(x, interp)
        else:
            self._check_input(x, interp)
            S, B = self._size_in(x, interp), int(x.shape[0])
            lowres, base = self._window_lowres(x.to(torch.float32), False, S, S, "uniform", B)["lowres"], None
        mask = _decide.threshold_mask(lowres, cls=cls, threshold=threshold, low=low, connectivity=connectivity, kind=kind,
                                      base=base, value=value, size=self._size_in(x, interp))
        return lowres, mask

    @torch.no_grad()
    def predict_threshold(self, x: torch.Tensor, cls: int = 1, threshold=0.5, low=None, connectivity: int = 4,
                          kind: str = "prob", over_argmax: bool = False, interpolate_pos_encoding: bool = False,
                          min_area: int = 0, fill_holes: bool = False, max_hole_area: int = 0):
        """uint8 [B, H, W]: class `cls` decided by threshold instead of by the argmax (decide.threshold_mask).  A pixel is kept
        when its score (`kind`, as in `predict_confidence`) reaches `threshold` -- e.g. `curves.ods(...)["threshold"]` --, or,
        with `low`, when it reaches `low` and is `connectivity`-connected through such pixels to one that reaches `threshold`
        (hysteresis).  Kept pixels state `cls` (1 for a one-class model), the others 0; with `over_argmax` the others keep
        what `predict_mask` states, except that a pixel it gave to `cls` becomes 0.  The encoder runs once and the scores are
        re-generated from the low-res head output: the full-size logits are never written.  `min_area` / `fill_holes` /
        `max_hole_area` (defaults: off): the mask is then cleaned by clean.clean_mask with this call's `connectivity`, on the
        same stream."""
        from . import clean as _clean
        min_area, fill_holes, max_hole_area = _clean.check_options(min_area, fill_holes, max_hole_area)
        _, mask = self._lowres_and_threshold(x, cls, threshold, low, connectivity, kind, bool(over_argmax),
                                             bool(interpolate_pos_encoding))
        if _clean.active(min_area, fill_holes):
            mask = _clean.clean_mask(mask, min_area=min_area, fill_holes=fill_holes, max_hole_area=max_hole_area,
                                     connectivity=connectivity)
        return mask

    @torch.no_grad()
    def predict_regions(self, x: torch.Tensor, *, background: int = 0, connectivity: int = 4, return_mask: bool = False,
                        interpolate_pos_encoding: bool = False, min_area: int = 0, fill_holes: bool = False,
                        max_hole_area: int = 0, props: bool = False, skeleton_classes=None, scores: bool = False,
                        score_kind: str = "prob", low: float = 0.5):
        """The regions of each image's predicted mask: a list of int32 [k, 7] numpy arrays, rows (class, y_min, x_min,
        y_max, x_max, area, first) in (class, first) order (regions.region_boxes) -- the reference's "Predicted Regions
        with Boxes" (model/CE/testViTModel.py:34-42,171-185).  The forward, the mask and the labelling are enqueued on one
        stream; the host waits once, for the region counts.  `return_mask`: also the uint8 [B, H, W] device mask.
        `min_area` / `fill_holes` / `max_hole_area` (defaults: off): the regions, and the mask returned, are those of the
        mask cleaned by clean.clean_mask with this call's `connectivity` and `background`, enqueued on the same stream.
        `props` (default off): the list holds the int64 [k, 20] measurement rows of regions.region_props instead (the same
        regions in the same order; `skeleton_classes` as there), again of the cleaned mask when the clean-up is on.
        `scores` (default off): the result is (records or props, score_rows[, mask]) -- per image the int64 [k, 4] rows
        (pixels, sum_q, max_deficit, n_low) of confidence.region_scores for the same regions in the same order (`score_kind`,
        `low` as there), scored on the cleaned mask when the clean-up is on: a filled hole carries a class that did not win
        and scores accordingly.  The encoder still runs once; the mask is `predict_mask`'s bit for bit."""
        from . import clean as _clean, regions as _regions
        if skeleton_classes is not None and not props:
            raise ValueError("skeleton_classes needs props=True")
        lowres = None
        if scores:
            from . import confidence as _conf
            if score_kind not in _conf.KINDS:
                raise ValueError(f"score_kind must be one of {sorted(_conf.KINDS)}, got {score_kind!r}")
            _conf.low_to_q(low)
            lowres, mask = self._lowres_and_mask(x, bool(interpolate_pos_encoding))
        else:
            mask = self.predict_mask(x, interpolate_pos_encoding=interpolate_pos_encoding)
        if min_area or fill_holes or max_hole_area:   # with both steps off clean_mask checks its arguments and launches nothing
            mask = _clean.clean_mask(mask, min_area=min_area, fill_holes=fill_holes, max_hole_area=max_hole_area,
                                     connectivity=connectivity, background=background)
        if props:
            recs = _regions.region_props(mask, skeleton_classes=skeleton_classes, background=background,
                                         connectivity=connectivity)
        elif not scores:
            recs = _regions.region_boxes(mask, background=background, connectivity=connectivity)
        if scores:
            boxes, rows = _conf.region_scores(lowres, mask, kind=score_kind, low=low, background=background,
                                              connectivity=connectivity)
            if not props:
                recs = boxes
            return (recs, rows, mask) if return_mask else (recs, rows)
        return (recs, mask) if return_mask else recs

    @torch.no_grad()
    def predict_polygons(self, x: torch.Tensor, *, background: int = 0, connectivity: int = 4,
                         interpolate_pos_encoding: bool = False, min_area: int = 0, fill_holes: bool = False,
                         max_hole_area: int = 0, return_mask: bool = False, simplify=None):
        """The outlines of the regions of each image's predicted mask: a list of (records, polygons) pairs, `records` the int32
        [k, 7] rows of `predict_regions`, `polygons[i]` the rings of region i as int32 [v, 2] arrays of (y, x) pixel corners,
        the outer ring first, then the holes (polygons.region_polygons).  The forward, the mask and the outlining are enqueued
        on one stream; the host waits once, for the counts.  `min_area` / `fill_holes` / `max_hole_area` (defaults: off): the
        outlines, and the mask returned, are those of the mask cleaned by clean.clean_mask with this call's `connectivity` and
        `background`.  `return_mask`: also the uint8 [B, H, W] device mask.  `simplify`: a tolerance in pixels, the rings thinned
        on the device before the copy back (polygons.region_polygons)."""
        from . import clean as _clean, polygons as _polygons, simplify as _simplify
        if simplify is not None:
            _simplify.tol2_q8(simplify)   # before the forward
        mask = self.predict_mask(x, interpolate_pos_encoding=interpolate_pos_encoding)
        if min_area or fill_holes or max_hole_area:
            mask = _clean.clean_mask(mask, min_area=min_area, fill_holes=fill_holes, max_hole_area=max_hole_area,
                                     connectivity=connectivity, background=background)
        out = _polygons.region_polygons(mask, background=background, connectivity=connectivity, simplify=simplify)
        return (out, mask) if return_mask else out

    @torch.no_grad()
    def predict_centerlines(self, x: torch.Tensor, classes, *, route: str = "auto", background: int = 0, connectivity: int = 4,
                            interpolate_pos_encoding: bool = False, min_area: int = 0, fill_holes: bool = False,
                            max_hole_area: int = 0, return_mask: bool = False, simplify=None):
        """The centre-line graph of the label values `classes` in each image's predicted mask: a list of dicts class ->
        (nodes, branches, points), the rows of centerlines.trace on the skeleton of {mask == class}.  `min_area` /
        `fill_holes` / `max_hole_area` (defaults: off): the graph, and the mask returned, are those of the mask cleaned by
        clean.clean_mask with this call's `connectivity` and `background`.  `return_mask`: also the uint8 [B, H, W] device
        mask.  `simplify`: a tolerance in pixels, the polylines thinned on the device before the copy back (centerlines.trace)."""
        from . import centerlines as _centerlines, clean as _clean, simplify as _simplify
        if simplify is not None:
            _simplify.tol2_q8(simplify)   # before the forward
        if classes is None:
            raise ValueError("classes must be a sequence of label values")
        _centerlines.check_options(classes, True, route)   # before the forward
        _clean.check_options(min_area, fill_holes, max_hole_area)
        mask = self.predict_mask(x, interpolate_pos_encoding=interpolate_pos_encoding)
        if min_area or fill_holes or max_hole_area:
            mask = _clean.clean_mask(mask, min_area=min_area, fill_holes=fill_holes, max_hole_area=max_hole_area,
                                     connectivity=connectivity, background=background)
        out = _centerlines.trace(mask, classes=classes, route=route, simplify=simplify)
        return (out, mask) if return_mask else out

    @torch.no_grad()
    def predict_mask_graphed(self, x: torch.Tensor, return_logits: bool = False, interpolate_pos_encoding: bool = False):
        """`predict_mask` replayed from a captured hipGraph (one per batch size and output set): the ~110 kernel
        launches of a forward become one graph launch.  Measured (tools/latency_probe.py, ViT-B/16): no gain at batch
        1-8 -- 1.4 ms (bf16) to 5.9 ms (fp32) per forward at 224x224 is GPU time of under-filled GEMM launches, not host
        launch time -- so nothing uses it by default; it is there for smaller models / faster hosts, and bit-identical
        to the eager path.  Inputs are copied into the graph's static buffer; the returned tensors are the graph's
        static outputs and are overwritten by the next call with the same batch size (clone them to keep them).
        Re-captured automatically when the parameters change.  Native size only: another input size (interpolated
        position embeddings) raises ValueError -- use `predict_mask(..., interpolate_pos_encoding=True)`."""
        if interpolate_pos_encoding and tuple(x.shape[2:]) != (self.cfg.image_size, self.cfg.image_size):
            raise ValueError(f"predict_mask_graphed runs at the model's image size {self.cfg.image_size} only, got "
                             f"{tuple(x.shape[2:])}: use predict_mask(..., interpolate_pos_encoding=True)")
        self._check_input(x)
        key = (int(x.shape[0]), bool(return_logits))
        ver = (self.arena._version, self.arena.data_ptr())
        g = self._graphs.get(key)
        if g is None or g["ver"] != ver:
            xs = x.to(torch.float32).contiguous().clone()
            ws = torch.empty(_lib.query_workspace(self.cfg, key[0], self.precision), dtype=torch.uint8,
                             device=self.arena.device)   # owned by the graph: `workspace()` recycles its buffer
            side = torch.cuda.Stream(device=xs.device)
            side.wait_stream(torch.cuda.current_stream(xs.device))
            with torch.cuda.stream(side):            # warm-up outside the capture: workspace, shadow arena, attributes
                for _ in range(2):
                    self._run(xs, return_logits, True, ws)
            torch.cuda.current_stream(xs.device).wait_stream(side)
            graph = torch.cuda.CUDAGraph(keep_graph=True)   # the hipGraph_t stays readable (graph_nodes)
            with torch.cuda.graph(graph):
                logits, mask = self._run(xs, return_logits, True, ws)
            graph.instantiate()
            g = dict(graph=graph, x=xs, ws=ws, logits=logits, mask=mask, ver=ver)
            self._graphs[key] = g
        g["x"].copy_(x, non_blocking=True)
        g["graph"].replay()
        return (g["mask"], g["logits"]) if return_logits else g["mask"]

    def graph_nodes(self, batch: int, return_logits: bool = False) -> Optional[int]:
        """Launches per forward = nodes of the hipGraph `predict_mask_graphed` captured for this batch size (None if it
        has not been captured yet)."""
        g = self._graphs.get((int(batch), bool(return_logits)))
        if g is None:
            return None
        hip = C.CDLL("libamdhip64.so")
        hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
        n = C.c_size_t()
        rc = hip.hipGraphGetNodes(C.c_void_p(g["graph"].raw_cuda_graph()), None, C.byref(n))
        if rc != 0:
            raise RuntimeError(f"hipGraphGetNodes failed with {rc}")
        return int(n.value)

    @torch.no_grad()
    def predict_mask_tiled(self, x: torch.Tensor) -> torch.Tensor:
        """Masks for images LARGER than the model's image size by spatial tiling (BASELINE configs[4]: 1024x1024
        inputs through an image_size=512 model as four 512x512 tiles per image; build-defined).
        x: [B, 3, H, W] with H, W multiples of image_size -> uint8 [B, H, W].  Tiles are independent units, so they
        simply extend the batch; each tile sees only its own pixels (no cross-tile attention)."""
        S = self.cfg.image_size
        B, Cc, H, W = x.shape
        if H % S or W % S:
            raise ValueError(f"tiled prediction needs H and W to be multiples of {S}, got {H}x{W}")
        ty, tx = H // S, W // S
        tiles = x.reshape(B, Cc, ty, S, tx, S).permute(0, 2, 4, 1, 3, 5).reshape(B * ty * tx, Cc, S, S).contiguous()
        m = self.predict_mask(tiles)
        return m.reshape(B, ty, tx, S, S).permute(0, 1, 3, 2, 4).reshape(B, H, W).contiguous()

    @torch.no_grad()
    def predict_mask_windowed(self, x: torch.Tensor, *, stride: Optional[int] = None, weights: str = "linear",
                              tile_batch: int = 32, window_size: Optional[int] = None, return_logits: bool = False):
        """Masks for images of ANY size >= the window by overlapping sliding-window inference: the image is covered by
        S x S windows `stride` apart (the last one of an axis shifted back to end at the edge), every window runs through
        the model as a tile, and the tiles' low-resolution head outputs are blended on the device -- each covering tile
        upsampled on the fly with the decoder tail's arithmetic, weighted, normalised, then sigmoid -> argmax
        (vitseg_window_blend, include/vitseg.h); the per-tile full-resolution logits are never materialised.
        x: [B, 3, H, W] fp32 or [B, H, W, 3] uint8 (decoded bytes; converted as ToTensor does while the tiles are gathered)
        -> uint8 [B, H, W], and the blended fp32 logits [B, C, H, W] with `return_logits`.
        `stride`: default 3 S / 4 rounded down to a multiple of the patch size.  `weights`: "uniform" (all ones: the mean of
        the covering tiles) or "linear" (min(i + 1, S - i) along each axis: a tile counts most at its centre, so the hard
        tile edges, where the ViT had no context, fade out).  `window_size`: the window's side S, default the model's image
        size; another size runs with the position table resampled (interpolate_pos_encoding).  `tile_batch`: tiles per
        forward; the result does not depend on it (a short last chunk that would take another kernel route than the full
        ones is padded with repeated tiles).  With H = W = S the result is `predict_mask`'s, bit for bit."""
        cfg = self.cfg
        S = cfg.image_size if window_size is None else int(window_size)
        u8 = x.dtype == torch.uint8
        if x.dim() != 4 or (x.shape[-1] if u8 else x.shape[1]) != cfg.num_channels:
            raise ValueError(f"expected [B, {cfg.num_channels}, H, W] fp32 or [B, H, W, {cfg.num_channels}] uint8, got "
                             f"{x.dtype} {tuple(x.shape)}")
        if not x.is_cuda or x.device != self.arena.device:
            raise RuntimeError("ViTSegmentationModel runs on the MI355X only: move the model and the input to the "
                               f"same HIP device (input on {x.device}, parameters on {self.arena.device}). "
                               "There is no CPU fallback.")
        B, (H, W) = int(x.shape[0]), ((x.shape[1], x.shape[2]) if u8 else (x.shape[2], x.shape[3]))
        H, W, P = int(H), int(W), cfg.patch_size
        if S < P or S % P:
            raise ValueError(f"window size {S} is not a positive multiple of the patch size {P}.")
        if H < S or W < S:
            raise ValueError(f"image {H}x{W} is smaller than the {S}x{S} window")
        if stride is None:
            stride = max(P, (3 * S // 4) // P * P)
        if weights not in ("uniform", "linear"):
            raise ValueError(f'weights must be "uniform" or "linear", got {weights!r}')
        if int(tile_batch) < 1:
            raise ValueError(f"tile_batch must be >= 1, got {tile_batch}")
        plan = self._window_lowres(x, u8, S, int(stride), weights, int(tile_batch))
        return self._window_blend(plan, return_logits, True)

    def _window_lowres(self, x, u8: bool, S: int, stride: int, weights: str, tile_batch: int) -> dict:
        """The tiles of `x` gathered and forwarded `tile_batch` at a time into one low-res buffer [T, C, g, g]; returns what
        `_window_blend` needs (tools/window_probe.py times the two halves apart)."""
        cfg, P = self.cfg, self.cfg.patch_size
        B, (H, W) = int(x.shape[0]), ((int(x.shape[1]), int(x.shape[2])) if u8 else (int(x.shape[2]), int(x.shape[3])))
        oy, ox = _lib.window_origins(H, S, stride), _lib.window_origins(W, S, stride)   # ValueError on a bad stride
        ny, nx = len(oy), len(ox)
        T, g, Cc, dev = B * ny * nx, S // P, cfg.num_classes, x.device
        x = x.contiguous() if u8 else x.to(torch.float32).contiguous()
        tab = torch.tensor(oy + ox, dtype=torch.int32).to(dev)
        i = torch.arange(S, dtype=torch.float32)
        wtab = (torch.ones(S) if weights == "uniform" else torch.minimum(i + 1, S - i)).to(dev)
        chunk = min(int(tile_batch), T)
        tiles = torch.empty((chunk, cfg.num_channels, S, S), dtype=torch.float32, device=dev)
        lowres = torch.empty((T, Cc, g, g), dtype=torch.float32, device=dev)
        ws, lp = self.workspace(chunk, S), self._bf16_arena()
        ccfg = C.byref(_lib.CConfig.from_config(cfg))
        gather, fwd = _lib.symbol("vitseg_window_gather"), _lib.symbol("vitseg_forward_lowres")
        route = self.forward_route(chunk, S)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            for first in range(0, T, chunk):
                cnt = min(chunk, T - first)
                _lib.check(gather(x.data_ptr(), int(u8), B, H, W, S, tab.data_ptr(), ny, tab[ny:].data_ptr(), nx, first, cnt,
                                  tiles.data_ptr(), stream))
                # results are bit-identical across batch sizes inside one route only: a short chunk on another route is
                # padded to the full size with repeats of its first tile, and the extras are dropped
                run = cnt if cnt == chunk or self.forward_route(cnt, S) == route else chunk
                if run != cnt:
                    tiles[cnt:] = tiles[0]
                out = lowres[first:first + cnt] if run == cnt else torch.empty((run, Cc, g, g), dtype=torch.float32, device=dev)
                wsr = ws if run == chunk else self.workspace(run, S)
                _lib.check(fwd(ccfg, S, self.arena.data_ptr(), _ptr(lp), tiles.data_ptr(), run, self.precision, out.data_ptr(),
                               wsr.data_ptr(), wsr.numel(), stream))
                if run != cnt:
                    lowres[first:first + cnt] = out[:cnt]
        return dict(lowres=lowres, tab=tab, ny=ny, nx=nx, wtab=wtab, B=B, g=g, S=S, H=H, W=W)

    def _window_blend(self, p: dict, want_logits: bool, want_mask: bool):
        """One vitseg_window_blend launch over the low-res tiles of `_window_lowres`."""
        B, H, W, Cc, dev = p["B"], p["H"], p["W"], self.cfg.num_classes, p["lowres"].device
        logits = torch.empty((B, Cc, H, W), dtype=torch.float32, device=dev) if want_logits else None
        mask = torch.empty((B, H, W), dtype=torch.uint8, device=dev) if want_mask else None
        with torch.cuda.device(dev):
            _lib.check(_lib.symbol("vitseg_window_blend")(p["lowres"].data_ptr(), p["tab"].data_ptr(), p["ny"],
                                                          p["tab"][p["ny"]:].data_ptr(), p["nx"], p["wtab"].data_ptr(), B,
                                                          Cc, p["g"], p["S"], H, W, _ptr(logits), _ptr(mask),
                                                          torch.cuda.current_stream().cuda_stream))
        return (mask, logits) if want_logits and want_mask else (mask if want_mask else logits)

    # ------------------------------------------------------------------ test-time augmentation
    @torch.no_grad()
    def predict_mask_tta(self, x: torch.Tensor, tta="d4", sizes=None, weights=None, merge: str = "logits",
                         return_merged: bool = False):
        """Masks by test-time augmentation: the model runs on flipped, quarter-turned and rescaled copies of the batch (the
        views), and ONE launch brings every view's low-resolution head output back to the image's frame -- upsampled on
        the fly with the decoder tail's arithmetic --, averages them and takes sigmoid -> argmax (vitseg_tta_blend,
        include/vitseg.h); no per-view full-size tensor is materialised.
        x: fp32 [B, 3, S, S] or uint8 [B, S, S, 3] (decoded bytes, converted as ToTensor does), square, S the output size
        -> uint8 [B, S, S], and with `return_merged` the merged fp32 [B, C, S, S] (logits, or probabilities for
        merge="probs").
        `tta`: "none" (op 0), "hflip" (0, 4), "flip" (0, 2, 4, 6), "d4" (0..7) or a sequence of ops; an op's `op >> 2` is a
        horizontal flip applied first and `op & 3` the number of counter-clockwise quarter turns (tta.py).  `sizes`: the
        sides the views are resampled to, multiples of the patch size, default (S,); `weights`: one per size, default 1.
        The views are sizes x ops, size-major.  `merge`: "logits" (the mean of the views' logits) or "probs" (the mean of
        their sigmoids).
        The view images come from the training augmentation's launch (vitseg_augment, edge border, no colour step): flips
        and quarter turns at the image's own size are bit-exact permutations; a rescale is that kernel's plain two-tap
        bilinear WITHOUT anti-aliasing, so sizes below half the input alias.  Every view is forwarded on its own at the
        caller's batch (vitseg_forward_lowres: the kernel route of `predict_mask` at that size), so tta="none" reproduces
        `predict_mask` bit for bit.  Everything is enqueued on the current stream; the host never waits."""
        from . import tta as _tta
        _tta.merge_mode(merge)   # (refused before anything is launched)
        plan = self._tta_lowres(x, tta, sizes, weights)
        return self._tta_blend(plan, merge, bool(return_merged), True)

    def _tta_matrix(self, op: int, src: int, dst: int, n: int) -> torch.Tensor:
        """Device int64 [n, 6]: the Q16 matrix of view(., op) from a src x src image to a dst x dst view, once per sample;
        cached, so a repeated call uploads nothing."""
        cache = self.__dict__.setdefault("_tta_tabs", {})
        key = (op, src, dst, n)
        tab = cache.get(key)
        if tab is None:
            if len(cache) >= 64:
                cache.clear()
            m = _lib.augment_matrix(_lib.tta_affine(op), (src, src), (dst, dst))
            tab = cache[key] = torch.tensor([m] * n, dtype=torch.int64).to(self.arena.device)
        return tab

    def _tta_view_image(self, x: torch.Tensor, u8: bool, op: int, size: int, out: torch.Tensor) -> torch.Tensor:
        """view(x, op) resampled to size x size as fp32 NCHW, by one vitseg_augment launch into `out`.  An fp32 batch's
        identity view at its own size is the batch itself: no launch."""
        B, S = int(x.shape[0]), int(x.shape[2])
        if op == 0 and size == S and not u8:
            return x
        tab = self._tta_matrix(op, S, size, B)
        none = (_lib.CAugmentMask * 1)()
        with torch.cuda.device(x.device):
            _lib.check(_lib.symbol("vitseg_augment")(
                x.data_ptr(), _lib.AUGMENT_U8_NHWC if u8 else _lib.AUGMENT_F32_NCHW, B, S, S, size, size, tab.data_ptr(),
                None, out.data_ptr(), none, 0, _lib.AUGMENT_EDGE, None, 0, torch.cuda.current_stream().cuda_stream))
        return out

    def _tta_lowres(self, x: torch.Tensor, tta, sizes, weights) -> dict:
        """The views of `x` built and forwarded one by one to their low-res maps [B, C, g, g]; returns what `_tta_blend`
        needs (tools/tta_probe.py times the two halves apart)."""
        from . import tta as _tta
        cfg = self.cfg
        u8 = x.dtype == torch.uint8
        if x.dim() != 4 or (x.shape[-1] if u8 else x.shape[1]) != cfg.num_channels or x.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f"expected [B, {cfg.num_channels}, S, S] fp32 or [B, S, S, {cfg.num_channels}] uint8, got "
                             f"{x.dtype} {tuple(x.shape)}")
        H, W = (int(x.shape[1]), int(x.shape[2])) if u8 else (int(x.shape[2]), int(x.shape[3]))
        if H != W:
            raise ValueError(f"test-time augmentation needs a square input, got {H}*{W}.")
        if int(x.shape[0]) < 1:
            raise ValueError("empty batch")
        views = _tta.view_list(tta, sizes, weights, H, cfg.patch_size)
        if not x.is_cuda or x.device != self.arena.device:
            raise RuntimeError("ViTSegmentationModel runs on the MI355X only: move the model and the input to the "
                               f"same HIP device (input on {x.device}, parameters on {self.arena.device}). "
                               "There is no CPU fallback.")
        x = x.contiguous()
        B, Cc, P, dev = int(x.shape[0]), cfg.num_classes, cfg.patch_size, x.device
        lp = self._bf16_arena()
        ccfg = C.byref(_lib.CConfig.from_config(cfg))
        fwd = _lib.symbol("vitseg_forward_lowres")
        bufs, out = {}, []
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            for op, size, w in views:
                if size not in bufs:   # one image buffer per size: the stream orders its reuse
                    bufs[size] = torch.empty((B, cfg.num_channels, size, size), dtype=torch.float32, device=dev)
                xv = self._tta_view_image(x, u8, op, size, bufs[size])
                g = size // P
                low = torch.empty((B, Cc, g, g), dtype=torch.float32, device=dev)
                ws = self.workspace(B, size)
                _lib.check(fwd(ccfg, size, self.arena.data_ptr(), _ptr(lp), xv.data_ptr(), B, self.precision, low.data_ptr(),
                               ws.data_ptr(), ws.numel(), stream))
                out.append((low, g, op, w))
        return dict(views=out, B=B, S=H)

    def _tta_blend(self, p: dict, merge: str, want_merged: bool, want_mask: bool):
        """One vitseg_tta_blend launch over the low-res maps of `_tta_lowres`."""
        from . import tta as _tta
        mode = _tta.merge_mode(merge)
        B, S, Cc, views = p["B"], p["S"], self.cfg.num_classes, p["views"]
        dev = views[0][0].device
        merged = torch.empty((B, Cc, S, S), dtype=torch.float32, device=dev) if want_merged else None
        mask = torch.empty((B, S, S), dtype=torch.uint8, device=dev) if want_mask else None
        descs = (_lib.CTTAView * len(views))(*[_lib.CTTAView(low.data_ptr(), g, op, w) for low, g, op, w in views])
        with torch.cuda.device(dev):
            _lib.check(_lib.symbol("vitseg_tta_blend")(descs, len(views), B, Cc, S, mode, _ptr(merged), _ptr(mask),
                                                       torch.cuda.current_stream().cuda_stream))
        return (mask, merged) if want_merged and want_mask else (mask if want_mask else merged)

    _CE_CACHE_ENTRIES = 8  # device weight vectors / scratch buffers kept per model, least recently used first out

    def _ce_cached(self, kind: str, key, make):
        """The device tensor cached under `key`, made by `make()` on a miss; each kind keeps the `_CE_CACHE_ENTRIES`
        most recently used."""
        cache = self.__dict__.setdefault("_ce_opt_cache", {}).setdefault(kind, OrderedDict())
        t = cache.get(key)
        if t is None:
            t = cache[key] = make()
            while len(cache) > self._CE_CACHE_ENTRIES:
                cache.popitem(last=False)
        else:
            cache.move_to_end(key)
        return t

    def _ce_options(self, B: int, S: int, ignore_index, class_weight, label_smoothing):
        """The `_lib.CCEOptions` of a `ce_loss` call, or None when all three options are at their defaults (the plain
        calls).  The options are validated on the host on every call (C <= 255 numbers).  The device copy of the weights
        is cached under the fp32 VALUES the kernels are to read, never under the identity of what was passed: another
        tensor at a recycled address, or one edited in place, has other values and so another entry.  The small scratch
        of the count pass is cached per (batch, size).  Both caches are bounded; the returned struct holds its tensors."""
        checked = check_ce_options(self.cfg.num_classes, ignore_index, class_weight, label_smoothing)
        if checked is None:
            return None
        ii, w, eps = checked
        dev = self.arena.device
        wdev = None
        if w is not None:
            wdev = self._ce_cached("weight", (w.numpy().tobytes(), dev), lambda: w.to(dev).contiguous())
        nbytes = int(_lib.symbol("vitseg_ce_options_scratch_bytes")(B, S))
        scratch = self._ce_cached("scratch", (B, S, dev), lambda: torch.empty(nbytes, dtype=torch.uint8, device=dev))
        opts = _lib.CCEOptions(int(ii is not None), 0, 0 if ii is None else ii, _ptr(wdev), eps, scratch.data_ptr(),
                               scratch.numel())
        opts._tensors = (wdev, scratch)   # the struct holds raw addresses: an eviction must not free them under it
        return opts

    def _hard_options(self, B: int, S: int, focal_gamma, ohem_thresh, ohem_min_kept, ohem_keep_fraction, force: bool = False):
        """The `_ext.CHardOptions` of a `ce_loss` call (validated on the host), or None when the four options are at their
        defaults and `force` is off (the calls without them).  Its scratch is cached per (batch, size)."""
        checked = check_hard_options(focal_gamma, ohem_thresh, ohem_min_kept, ohem_keep_fraction)
        if checked is None:
            if not force:
                return None
            checked = (0.0, float("inf"), 0, 0)
        dev = self.arena.device
        nbytes = int(_ext.ext_symbol("hardloss", "vitseg_hard_loss_scratch_bytes")(B, S))
        if nbytes == 0:
            raise ValueError(f"the focal / OHEM loss takes fewer than 2^31 pixels a call, got {B} x {S} x {S}")
        scratch = self._ce_cached("hard scratch", (B, S, dev), lambda: torch.empty(nbytes, dtype=torch.uint8, device=dev))
        opts = _ext.CHardOptions(checked[0], checked[1], checked[2], checked[3], 0, scratch.data_ptr(), scratch.numel())
        opts._tensors = (scratch,)   # the struct holds a raw address: an eviction must not free it under the struct
        return opts

    def ce_loss(self, x: torch.Tensor, target: torch.Tensor, grad_scale: Optional[float] = None,
                interpolate_pos_encoding: bool = False, ignore_index: Optional[int] = None, class_weight=None,
                label_smoothing: float = 0.0, focal_gamma: float = 0.0, ohem_thresh: Optional[float] = None,
                ohem_min_kept: int = 0, ohem_keep_fraction: float = 0.0, return_stats: bool = False):
        """`nn.CrossEntropyLoss(weight=class_weight, ignore_index=ignore_index, label_smoothing=label_smoothing)(self(x),
        target)` (model/CE/classes.py:268,280 with the defaults) as a device scalar, without materialising the
        [B, C, S, S] logits: forward to the low-res map, then the fused upsample+CE kernel.
        `target`: class indices [B, S, S], torch.long (reference) or torch.uint8, on the model's device.  Labels must lie
        in [0, C) or equal `ignore_index`; any other label (255, -100, C without a matching `ignore_index`) makes the loss
        NaN.
        `ignore_index` (None = no label is ignored; 255 for void / border pixels of uint8 masks, -100 for torch's default):
        such pixels add nothing to the loss, get a zero gradient, and leave the mean's denominator.  `class_weight`: one
        weight >= 0 per class (sequence or tensor); the mean divides by the summed weights of the kept pixels, as torch
        does.  The weights are checked on the host on every call and their device copy is found again by value, so a
        new or edited tensor is honoured; a tensor that lives on the device is read back for that (one small
        synchronising copy per call): in a training loop pass a sequence or a CPU tensor.  `label_smoothing` in [0, 1].  When every pixel is ignored (or every kept pixel has weight 0) the loss is
        NaN, torch's 0 / 0.  Invalid options raise ValueError on the host.  With all three at their defaults the call is
        the plain one (the same kernels, the same bits).
        `focal_gamma` > 0: the focal loss (Lin et al. 2017), each pixel's term times (1 - p_y)^gamma.  `ohem_thresh`,
        `ohem_min_kept`, `ohem_keep_fraction`: online hard example mining as in HRNet's / mmsegmentation's OhemCrossEntropy --
        the mean runs over the hard pixels alone, those whose true-class probability lies under `ohem_thresh` (a probability
        in (0, 1], None = no threshold) and never fewer than max(ohem_min_kept, ceil(ohem_keep_fraction * valid pixels)), the
        hardest of the call's batch (per rank under data parallelism); pixels tied with the last one kept are kept too.
        Ranking is by the plain per-pixel CE; the denominator is the summed class weights of the hard pixels.  The selection
        runs on the device (include/vitseg_hardloss.h).  These four cannot be combined with `label_smoothing`.  With them at
        their defaults the call launches what it launched before.  `return_stats=True` returns (loss, stats), stats a device
        int64[4] {valid pixels, k, hard pixels, the fp32 bits of the CE threshold tau}.
        `grad_scale` (optional): the gradient `loss.backward()` deposits is grad_scale * d loss / d params, folded into
        the CE gradient inside the kernel (e.g. 1 / accumulate_grad_batches); call `.backward()` on the returned loss
        itself then -- an upstream factor is ignored in this mode.  `interpolate_pos_encoding`: as in `forward`; the
        target then has the input's size."""
        interp = bool(interpolate_pos_encoding)
        if interp:
            self._check_input(x, True)
        S, B = self._size_in(x, interp), x.shape[0]
        if tuple(target.shape) != (B, S, S) or target.dtype not in (torch.int64, torch.uint8):
            raise ValueError(f"target must be int64/uint8 [B, {S}, {S}], got {target.dtype} {tuple(target.shape)}")
        opts = self._ce_options(B, S, ignore_index, class_weight, label_smoothing)
        hard = self._hard_options(B, S, focal_gamma, ohem_thresh, ohem_min_kept, ohem_keep_fraction, force=bool(return_stats))
        if hard is not None:
            if label_smoothing != 0:
                raise ValueError("label_smoothing cannot be combined with focal_gamma / ohem_* / return_stats")
            return self._hard_ce_loss(x, target.to(self.arena.device).contiguous(), grad_scale, interp, opts, hard,
                                      bool(return_stats))
        if self._needs_grad():
            return _CELossFn.apply(self.arena, self, x, target.to(self.arena.device).contiguous(), grad_scale, interp, opts)
        with torch.no_grad():
            _, _ = self._run(x, False, True, interp=interp)  # fills the low-res logits (mask output is a by-product)
            low = self.debug_buffer(B, _lib.BUF_LOWRES, S)
            target = target.to(self.arena.device).contiguous()
            scratch = torch.empty(_lib.lib().vitseg_ce_scratch_bytes(B, S), dtype=torch.uint8, device=low.device)
            loss = torch.empty((), dtype=torch.float32, device=low.device)
            args = (low.data_ptr(), target.data_ptr(), int(target.dtype == torch.uint8), None, scratch.data_ptr(),
                    loss.data_ptr(), B, self.cfg.num_classes, S // self.cfg.patch_size, S)
            stream = torch.cuda.current_stream().cuda_stream
            if opts is None:
                _lib.check(_lib.lib().vitseg_ce_loss(*args, stream))
            else:
                _lib.check(_lib.symbol("vitseg_ce_loss_opts")(*args, C.byref(opts), 1.0, stream))
        return loss

    def _hard_ce_loss(self, x, target, grad_scale, interp, opts, hard, return_stats):
        """`ce_loss` with the focal / OHEM options: vitseg_backward_hard under autograd, else vitseg_hard_ce_loss on the
        inference forward's low-res logits."""
        B, S = x.shape[0], self._size_in(x, interp)
        if self._needs_grad():
            loss, stats = _HardCELossFn.apply(self.arena, self, x, target, grad_scale, interp, opts, hard)
        else:
            with torch.no_grad():
                _, _ = self._run(x, False, True, interp=interp)  # fills the low-res logits (mask output is a by-product)
                low = self.debug_buffer(B, _lib.BUF_LOWRES, S)
                scratch = torch.empty(_lib.lib().vitseg_ce_scratch_bytes(B, S), dtype=torch.uint8, device=low.device)
                loss = torch.empty((), dtype=torch.float32, device=low.device)
                stats = torch.zeros(4, dtype=torch.int64, device=low.device)
                _lib.check(_ext.ext_symbol("hardloss", "vitseg_hard_ce_loss")(
                    low.data_ptr(), target.data_ptr(), int(target.dtype == torch.uint8), None, scratch.data_ptr(), loss.data_ptr(),
                    B, self.cfg.num_classes, S // self.cfg.patch_size, S, C.byref(opts) if opts is not None else None,
                    C.byref(hard), 1.0, None, stats.data_ptr(), torch.cuda.current_stream().cuda_stream))
        return (loss, stats) if return_stats else loss

    def _dice_options(self, B: int, S: int, dice_weight, ce_weight, smooth, include_background):
        """The `_lib.CDiceOptions` of a `ce_dice_loss` call (validated on the host); its scratch is cached per (batch, size)."""
        dw, cw, sm, bg = check_dice_options(self.cfg.num_classes, dice_weight, ce_weight, smooth, include_background)
        dev = self.arena.device
        nbytes = int(_lib.symbol("vitseg_dice_options_scratch_bytes")(B, self.cfg.num_classes, S))
        scratch = self._ce_cached("dice scratch", (B, S, dev), lambda: torch.empty(nbytes, dtype=torch.uint8, device=dev))
        opts = _lib.CDiceOptions(cw, dw, sm, int(bg), scratch.data_ptr(), scratch.numel())
        opts._tensors = (scratch,)   # the struct holds a raw address: an eviction must not free it under the struct
        return opts

    def ce_dice_loss(self, x: torch.Tensor, target: torch.Tensor, *, dice_weight: float = 1.0, ce_weight: float = 1.0,
                     smooth: float = 1e-6, include_background: bool = True, ignore_index: Optional[int] = None,
                     class_weight=None, label_smoothing: float = 0.0, grad_scale: Optional[float] = None,
                     interpolate_pos_encoding: bool = False, return_terms: bool = False):
        """`ce_weight * CE + dice_weight * dice` on `self(x)` as a device scalar, without materialising the [B, C, S, S]
        logits or their gradient: CE is `ce_loss` with the same `ignore_index`, `class_weight` and `label_smoothing`; dice
        is the soft Dice loss of the softmax probabilities, `mean_c [1 - (2 I_c + smooth) / (P_c + T_c + smooth)]` with
        I_c = sum p_c t_c, P_c = sum p_c, T_c = sum t_c over the kept pixels of the whole batch (the binary trainer's
        `dice_loss`, model/PAED/classes.py:608-620, per class).  `include_background=False` leaves class 0 out of the
        mean.  `ignore_index` acts on both terms, the class weights and the smoothing on CE only.  A weight of 0 leaves
        its term out altogether (an exact 0; with `dice_weight=0` the value and the gradient are `ce_loss`'s).  A class
        no target pixel carries is still counted; when every pixel is ignored dice is 0 and CE is NaN.  A label outside
        [0, C) that is not `ignore_index` makes the loss NaN.  Invalid options raise ValueError on the host.
        `return_terms=True` returns (loss, ce, dice), the last two detached device scalars.  `target`, `grad_scale` and
        `interpolate_pos_encoding`: as in `ce_loss`."""
        interp = bool(interpolate_pos_encoding)
        if interp:
            self._check_input(x, True)
        S, B = self._size_in(x, interp), x.shape[0]
        if tuple(target.shape) != (B, S, S) or target.dtype not in (torch.int64, torch.uint8):
            raise ValueError(f"target must be int64/uint8 [B, {S}, {S}], got {target.dtype} {tuple(target.shape)}")
        dopts = self._dice_options(B, S, dice_weight, ce_weight, smooth, include_background)
        opts = self._ce_options(B, S, ignore_index, class_weight, label_smoothing)
        target = target.to(self.arena.device).contiguous()
        if self._needs_grad():
            terms = _CEDiceLossFn.apply(self.arena, self, x, target, grad_scale, interp, opts, dopts)
        else:
            with torch.no_grad():
                _, _ = self._run(x, False, True, interp=interp)  # fills the low-res logits (mask output is a by-product)
                low = self.debug_buffer(B, _lib.BUF_LOWRES, S)
                scratch = torch.empty(_lib.lib().vitseg_ce_scratch_bytes(B, S), dtype=torch.uint8, device=low.device)
                terms = torch.empty(3, dtype=torch.float32, device=low.device)
                _lib.check(_lib.symbol("vitseg_ce_dice_loss")(
                    low.data_ptr(), target.data_ptr(), int(target.dtype == torch.uint8), None, scratch.data_ptr(),
                    terms.data_ptr(), B, self.cfg.num_classes, S // self.cfg.patch_size, S,
                    C.byref(opts) if opts is not None else None, C.byref(dopts), 1.0, torch.cuda.current_stream().cuda_stream))
        if return_terms:
            return terms[0], terms[1].detach(), terms[2].detach()
        return terms[0]

    def _cldice_options(self, B: int, S: int, weight, classes, iters, smooth):
        """The `_ext.CClDiceOptions` of a `ce_cldice_loss` call (validated on the host); its scratch is cached per (batch,
        size, classes, iters)."""
        from .cldice import check_options
        w, cls, it, sm = check_options(self.cfg.num_classes, weight, classes, iters, smooth)
        dev = self.arena.device
        nbytes = int(_ext.ext_symbol("cldice", "vitseg_cldice_scratch_bytes")(B, len(cls), S, it))
        if nbytes == 0:
            raise ValueError(f"clDice planes of {len(cls)} x {B} x {S} x {S} pixels are beyond one call (2^31 - 1)")
        scratch = self._ce_cached("cldice scratch", (B, S, len(cls), it, dev), lambda: torch.empty(nbytes, dtype=torch.uint8, device=dev))
        arr = (C.c_int32 * len(cls))(*cls)
        opts = _ext.CClDiceOptions(w, sm, it, len(cls), arr, scratch.data_ptr(), scratch.numel(), None, None)
        opts._tensors = (scratch, arr)   # the struct holds raw addresses
        return opts

    def ce_cldice_loss(self, x: torch.Tensor, target: torch.Tensor, *, cldice_weight: float = 0.5, cldice_classes=None,
                       cldice_iters: int = 3, cldice_smooth: float = 1.0, dice_weight: float = 0.0, ce_weight: float = 1.0,
                       smooth: float = 1e-6, include_background: bool = True, ignore_index: Optional[int] = None,
                       class_weight=None, label_smoothing: float = 0.0, grad_scale: Optional[float] = None,
                       interpolate_pos_encoding: bool = False, return_terms: bool = False):
        """`ce_weight * CE + dice_weight * dice + cldice_weight * cldice` on `self(x)` as a device scalar, without
        materialising the logits or their gradient.  CE and dice are `ce_dice_loss`'s.  cldice is the soft-clDice loss of
        Shit et al. (CVPR 2021): per listed class the soft skeletons (`cldice_iters` rounds of min / max pooling) of the
        softmax plane and of the 0/1 target plane give a centre-line precision and sensitivity over the call's batch, smoothed
        by `cldice_smooth`, and cl = 1 - their harmonic mean; cldice is the mean of cl over `cldice_classes` (None: every
        class but 0).  It is per class, as the Dice term is (the published code pools the foreground channels).  Pixels of
        `ignore_index` take no part and get gradient 0.  The gradient is autograd's, ties included
        (include/vitseg_cldice.h).  A weight of 0 leaves its term out (an exact 0).  The focal / OHEM options of `ce_loss`
        cannot be combined with it.  `return_terms=True` returns (loss, ce, dice, cldice), the last three detached."""
        interp = bool(interpolate_pos_encoding)
        if interp:
            self._check_input(x, True)
        S, B = self._size_in(x, interp), x.shape[0]
        if tuple(target.shape) != (B, S, S) or target.dtype not in (torch.int64, torch.uint8):
            raise ValueError(f"target must be int64/uint8 [B, {S}, {S}], got {target.dtype} {tuple(target.shape)}")
        cld = self._cldice_options(B, S, cldice_weight, cldice_classes, cldice_iters, cldice_smooth)
        if cld.weight != 0.0 and float(dice_weight) == 0.0 and float(ce_weight) == 0.0:
            # the term alone: both weights 0, which `check_dice_options` refuses for `ce_dice_loss` and the C entry takes here
            dopts = self._dice_options(B, S, 0.0, 1.0, smooth, include_background)
            dopts.ce_weight = 0.0
        elif float(dice_weight) == 0.0 and float(ce_weight) == 1.0:
            dopts = None
        else:
            dopts = self._dice_options(B, S, dice_weight, ce_weight, smooth, include_background)
        opts = self._ce_options(B, S, ignore_index, class_weight, label_smoothing)
        target = target.to(self.arena.device).contiguous()
        if self._needs_grad():
            terms = _CEClDiceLossFn.apply(self.arena, self, x, target, grad_scale, interp, opts, dopts, cld)
        else:
            with torch.no_grad():
                _, _ = self._run(x, False, True, interp=interp)  # fills the low-res logits (mask output is a by-product)
                low = self.debug_buffer(B, _lib.BUF_LOWRES, S)
                scratch = torch.empty(_lib.lib().vitseg_ce_scratch_bytes(B, S), dtype=torch.uint8, device=low.device)
                terms = torch.empty(4, dtype=torch.float32, device=low.device)
                _lib.check(_ext.ext_symbol("cldice", "vitseg_ce_cldice_loss")(
                    low.data_ptr(), target.data_ptr(), int(target.dtype == torch.uint8), None, scratch.data_ptr(),
                    terms.data_ptr(), B, self.cfg.num_classes, S // self.cfg.patch_size, S,
                    C.byref(opts) if opts is not None else None, C.byref(dopts) if dopts is not None else None, C.byref(cld), 1.0,
                    torch.cuda.current_stream().cuda_stream))
        if return_terms:
            return terms[0], terms[1].detach(), terms[2].detach(), terms[3].detach()
        return terms[0]

    def _lovasz_options(self, B: int, S: int, weight, classes, per_image, present):
        """The `_ext.CLovaszOptions` of a `ce_lovasz_loss` call (validated on the host); its scratch is cached per (batch,
        size, number of classes)."""
        from .lovasz import check_options
        w, cls, pi, po = check_options(self.cfg.num_classes, weight, classes, per_image, present)
        dev = self.arena.device
        nbytes = int(_ext.ext_symbol("lovasz", "vitseg_lovasz_scratch_bytes")(B, len(cls), S))
        if nbytes == 0:
            raise ValueError(f"Lovasz planes of {len(cls)} x {B} x {S} x {S} pixels are beyond one call (2^31 - 1 pixels, 2^20 "
                             "segments)")
        scratch = self._ce_cached("lovasz scratch", (B, S, len(cls), dev), lambda: torch.empty(nbytes, dtype=torch.uint8, device=dev))
        arr = (C.c_int32 * len(cls))(*cls)
        opts = _ext.CLovaszOptions(w, len(cls), arr, pi, po, scratch.data_ptr(), scratch.numel(), None, None, None)
        opts._tensors = (scratch, arr)   # the struct holds raw addresses
        return opts

    def ce_lovasz_loss(self, x: torch.Tensor, target: torch.Tensor, *, lovasz_weight: float = 0.5, lovasz_classes=None,
                       lovasz_per_image: bool = False, lovasz_present: bool = True, dice_weight: float = 0.0,
                       ce_weight: float = 1.0, smooth: float = 1e-6, include_background: bool = True,
                       ignore_index: Optional[int] = None, class_weight=None, label_smoothing: float = 0.0,
                       grad_scale: Optional[float] = None, interpolate_pos_encoding: bool = False, return_terms: bool = False):
        """`ce_weight * CE + dice_weight * dice + lovasz_weight * lovasz` on `self(x)` as a device scalar, without
        materialising the logits or their gradient.  CE and dice are `ce_dice_loss`'s.  lovasz is the Lovasz-Softmax loss of
        Berman et al. (CVPR 2018), the convex surrogate of the Jaccard index: per listed class (`lovasz_classes`, None: every
        class) the errors |y - p| of a segment are sorted descending (equal errors by pixel index) and weighted by the
        Lovasz extension's gradient of the Jaccard loss; a segment is the call's batch, or each image with
        `lovasz_per_image` (the term is then the mean over the images).  `lovasz_present` (the published
        classes='present'): a class absent from a segment is left out of its mean.  Pixels of `ignore_index` take no rank
        and get gradient 0.  A weight of 0 leaves its term out (an exact 0).  The clDice term and the focal / OHEM options of
        `ce_loss` cannot be combined with it.  `return_terms=True` returns (loss, ce, dice, lovasz), the last three
        detached.  Semantics in full: include/vitseg_lovasz.h."""
        interp = bool(interpolate_pos_encoding)
        if interp:
            self._check_input(x, True)
        S, B = self._size_in(x, interp), x.shape[0]
        if tuple(target.shape) != (B, S, S) or target.dtype not in (torch.int64, torch.uint8):
            raise ValueError(f"target must be int64/uint8 [B, {S}, {S}], got {target.dtype} {tuple(target.shape)}")
        lov = self._lovasz_options(B, S, lovasz_weight, lovasz_classes, lovasz_per_image, lovasz_present)
        if lov.weight != 0.0 and float(dice_weight) == 0.0 and float(ce_weight) == 0.0:
            # the term alone: both weights 0, which `check_dice_options` refuses for `ce_dice_loss` and the C entry takes here
            dopts = self._dice_options(B, S, 0.0, 1.0, smooth, include_background)
            dopts.ce_weight = 0.0
        elif float(dice_weight) == 0.0 and float(ce_weight) == 1.0:
            dopts = None
        else:
            dopts = self._dice_options(B, S, dice_weight, ce_weight, smooth, include_background)
        opts = self._ce_options(B, S, ignore_index, class_weight, label_smoothing)
        target = target.to(self.arena.device).contiguous()
        if self._needs_grad():
            terms = _CEClDiceLossFn.apply(self.arena, self, x, target, grad_scale, interp, opts, dopts, lov)
        else:
            with torch.no_grad():
                _, _ = self._run(x, False, True, interp=interp)  # fills the low-res logits (mask output is a by-product)
                low = self.debug_buffer(B, _lib.BUF_LOWRES, S)
                scratch = torch.empty(_lib.lib().vitseg_ce_scratch_bytes(B, S), dtype=torch.uint8, device=low.device)
                terms = torch.empty(4, dtype=torch.float32, device=low.device)
                _lib.check(_ext.ext_symbol("lovasz", "vitseg_ce_lovasz_loss")(
                    low.data_ptr(), target.data_ptr(), int(target.dtype == torch.uint8), None, scratch.data_ptr(),
                    terms.data_ptr(), B, self.cfg.num_classes, S // self.cfg.patch_size, S,
                    C.byref(opts) if opts is not None else None, C.byref(dopts) if dopts is not None else None, C.byref(lov), 1.0,
                    torch.cuda.current_stream().cuda_stream))
        if return_terms:
            return terms[0], terms[1].detach(), terms[2].detach(), terms[3].detach()
        return terms[0]

    @torch.no_grad()
    def debug_buffer(self, batch: int, which: int, image_size: Optional[int] = None) -> torch.Tensor:
        """fp32 view of a workspace buffer defined after forward (parity tests); `image_size`: the input's side of that
        forward (interpolate_pos_encoding), default the model's."""
        off, n = _lib.workspace_offset(self.cfg, batch, self.precision, which, image_size)
        return self.workspace(batch, image_size)[off:off + n].view(torch.float32)
