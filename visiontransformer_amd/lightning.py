"""`LightningViTModel` -- the CE training/eval module of the reference without the `lightning`
dependency (/root/reference/model/CE/classes.py:264-297).

Same constructor, `forward`, `_resize_target`, `training_step`, `validation_step`,
`configure_optimizers` (Adam lr=1e-5), and the same checkpoint layout: `state_dict()` keys carry the
`model.` prefix of the reference's attribute name (classes.py:267) and `load_state_dict` accepts
`torch.load(ckpt)['state_dict']` as written by Lightning (model/CE/testViTModel.py:117-118).
Logging (`self.log`) is replaced by a plain `logged` dict; a minimal trainer loop lives in
`visiontransformer_amd.trainer`.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .model import ViTSegmentationModel, check_ce_options, check_dice_options, check_hard_options


class LightningViTModel(nn.Module):
    def __init__(self, num_classes, patch_size, hidden_size, num_hidden_layers, num_attention_heads, *,
                 interpolate_pos_encoding: bool = False, ignore_index=None, class_weight=None,
                 label_smoothing: float = 0.0, dice_weight: float = 0.0, dice_smooth: float = 1e-6,
                 dice_include_background: bool = True, augment=None, focal_gamma: float = 0.0, ohem_thresh=None,
                 ohem_min_kept: int = 0, ohem_keep_fraction: float = 0.0, cldice_weight: float = 0.0, cldice_classes=None,
                 cldice_iters: int = 3, cldice_smooth: float = 1.0, lovasz_weight: float = 0.0, lovasz_classes=None,
                 lovasz_per_image: bool = False, **kw):
        """`interpolate_pos_encoding`: inputs of other (square, multiple-of-P) sizes than `image_size` run with the
        position table resampled to their grid (ViTSegmentationModel.forward); targets are resized to the input's size.
        `ignore_index`, `class_weight`, `label_smoothing`: the arguments of the reference's `nn.CrossEntropyLoss()`
        (classes.py:268) it leaves at their defaults -- a void label whose pixels do not count, one weight per class,
        smoothed targets (ViTSegmentationModel.ce_loss); used by the training and the validation step alike.
        `dice_weight` > 0 adds that many times the soft Dice loss of the softmax probabilities to the CE
        (ViTSegmentationModel.ce_dice_loss with `dice_smooth`, `dice_include_background`); both steps then log `*_ce` and
        `*_dice` beside `*_loss`.  With 0 the steps call exactly what they call without the argument.
        `focal_gamma`, `ohem_thresh`, `ohem_min_kept`, `ohem_keep_fraction`: the focal factor and the online hard example
        mining of ViTSegmentationModel.ce_loss.  The training step then logs `train_kept`, the device scalar hard pixels /
        valid pixels; the validation step forms the same loss with OHEM off (the focal factor stays), so that `valid_loss` and
        early stopping do not follow the hardest pixels alone.  Not with `dice_weight` or `label_smoothing` (ValueError).  With
        all four at their defaults the steps call exactly what they call without the arguments.
        `cldice_weight` > 0 adds that many times the soft-clDice loss (ViTSegmentationModel.ce_cldice_loss with
        `cldice_classes`, `cldice_iters`, `cldice_smooth`; `dice_weight` goes along); both steps then log `*_ce`, `*_dice` and
        `*_cldice` beside `*_loss`, and validation forms the term too.  Not with `focal_gamma` / `ohem_*` (ValueError).  With 0
        the steps call exactly what they call without the argument.
        `lovasz_weight` > 0 adds that many times the Lovasz-Softmax loss (ViTSegmentationModel.ce_lovasz_loss with
        `lovasz_classes`, `lovasz_per_image`; `dice_weight` goes along); both steps then log `*_ce`, `*_dice` and `*_lovasz`
        beside `*_loss`, and validation forms the term too.  Not with `cldice_weight`, `focal_gamma` / `ohem_*` (ValueError).
        With 0 the steps call exactly what they call without the argument.
        `augment`: an `augment.Augmenter`; the training step (alone) warps and colour-jitters the batch with it, the mask
        going straight to the input's size as the class bytes the fused loss reads (one launch, in place of `_resize_target`).
        With None the steps launch exactly what they launch without the argument.
        `layer_decay`, `no_decay`, `freeze`, `head_lr_mult` (optim.arena_groups), `max_grad_norm`, `skip_nonfinite`, `ema_decay`
        (optim.FusedAdam), `weight_decay` (FusedAdamW in place of FusedAdam), `warmup_steps` with `total_steps`
        (optim.warmup_cosine, stepped per optimiser step): what `configure_optimizers` builds.  Without them it returns exactly
        what it returns without the arguments."""
        super().__init__()
        from .optim import pop_options
        self.optim_options = pop_options(kw)
        self.model = ViTSegmentationModel(num_classes, patch_size, hidden_size, num_hidden_layers,
                                          num_attention_heads, **kw)
        self.interpolate_pos_encoding = bool(interpolate_pos_encoding)
        check_ce_options(num_classes, ignore_index, class_weight, label_smoothing)   # ValueError here, not at the first step
        self.ignore_index, self.label_smoothing = ignore_index, label_smoothing
        # a tuple: one device copy, found again by value on every step
        self.class_weight = None if class_weight is None else tuple(float(v) for v in class_weight)
        self.dice_weight = float(dice_weight)
        if self.dice_weight != 0.0:
            check_dice_options(num_classes, dice_weight, 1.0, dice_smooth, dice_include_background)
        self.dice_smooth, self.dice_include_background = dice_smooth, bool(dice_include_background)
        self.hard = check_hard_options(focal_gamma, ohem_thresh, ohem_min_kept, ohem_keep_fraction) is not None
        self.focal_gamma, self.ohem_thresh = focal_gamma, ohem_thresh
        self.ohem_min_kept, self.ohem_keep_fraction = ohem_min_kept, ohem_keep_fraction
        if self.hard and self.dice_weight != 0.0:
            raise ValueError("focal_gamma / ohem_* cannot be combined with dice_weight: composing them with the Dice term needs "
                             "a variant of the fused CE + Dice kernel and is out of scope")
        if self.hard and label_smoothing != 0:
            raise ValueError("focal_gamma / ohem_* cannot be combined with label_smoothing")
        self.cldice_weight = float(cldice_weight)
        self.cldice_classes = None if cldice_classes is None else tuple(int(c) for c in cldice_classes)
        self.cldice_iters, self.cldice_smooth = cldice_iters, cldice_smooth
        from .cldice import check_options as check_cldice_options
        if self.cldice_weight != 0.0 or cldice_classes is not None:   # ValueError here, not at the first step
            check_cldice_options(num_classes, cldice_weight, cldice_classes, cldice_iters, cldice_smooth)
        if self.hard and self.cldice_weight != 0.0:
            raise ValueError("focal_gamma / ohem_* cannot be combined with cldice_weight: focal and OHEM with the clDice term are "
                             "not built")
        self.lovasz_weight = float(lovasz_weight)
        self.lovasz_classes = None if lovasz_classes is None else tuple(int(c) for c in lovasz_classes)
        self.lovasz_per_image = bool(lovasz_per_image)
        from .lovasz import check_options as check_lovasz_options
        if self.lovasz_weight != 0.0 or lovasz_classes is not None:   # ValueError here, not at the first step
            check_lovasz_options(num_classes, lovasz_weight, lovasz_classes, lovasz_per_image)
        if self.lovasz_weight != 0.0 and self.cldice_weight != 0.0:
            raise ValueError("lovasz_weight cannot be combined with cldice_weight: the two terms in one call are not built")
        if self.hard and self.lovasz_weight != 0.0:
            raise ValueError("focal_gamma / ohem_* cannot be combined with lovasz_weight: focal and OHEM with the Lovasz term are "
                             "not built")
        self.augment = augment
        self.logged = {}

    def forward(self, x):
        if self.interpolate_pos_encoding:
            return self.model(x, interpolate_pos_encoding=True)
        return self.model(x)

    def _resize_target(self, y, size, dtype=torch.long):
        """classes.py:273-274: F.interpolate(y[:, None].float(), size, mode='nearest') -> long (idx = min(floor(dst*in/out),
        in-1)).  Targets on the GPU go through one gather kernel (preprocess.Preprocessor.targets: no float round trip, no
        ATen kernels in the training step); a CPU tensor is host-side label preprocessing as in the reference."""
        if y.is_cuda and y.dim() == 3 and y.dtype in (torch.long, torch.uint8):
            from .preprocess import Preprocessor
            if getattr(self, "_prep", None) is None or self._prep.device != y.device:
                self._prep = Preprocessor(self.model.cfg.image_size, device=y.device)
            return self._prep.targets(y, tuple(size), dtype=dtype)
        return F.interpolate(y.unsqueeze(1).float(), size=size, mode="nearest").squeeze(1).to(dtype)

    def _loss(self, batch, grad_scale=None, stage=None, augment=None):
        """`stage` ("train" / "valid"): where the CE and Dice terms are logged when the Dice term is on.  `augment`: the
        Augmenter that produces the step's input and targets from the batch."""
        x, y = batch
        S = self.model.cfg.image_size  # the reference hard-codes (224, 224) = its image_size (classes.py:278)
        if self.interpolate_pos_encoding:
            S = int(x.shape[-1])       # ... which is also its input size: with other input sizes, the input's
        # uint8 class indices: what the fused CE kernels read (a quarter of the int64 bytes); C <= 32 in training.  An
        # ignored label that a byte cannot hold (torch's -100) keeps the targets int64
        wide = self.ignore_index is not None and not 0 <= self.ignore_index <= 255
        if augment is not None:   # image and mask warped by one draw; the mask lands at the augmenter's output size
            x, y = augment.apply(x, y, mask_size=augment.S, mask_dtype=torch.long if wide else torch.uint8)
        else:
            y = self._resize_target(y.to(x.device, non_blocking=True), size=(S, S), dtype=torch.long if wide else torch.uint8)
        opts = {}
        if self.ignore_index is not None or self.class_weight is not None or self.label_smoothing != 0:
            opts = dict(ignore_index=self.ignore_index, class_weight=self.class_weight, label_smoothing=self.label_smoothing)
        if self.lovasz_weight != 0.0:
            loss, ce, dice, lov = self.model.ce_lovasz_loss(
                x, y, lovasz_weight=self.lovasz_weight, lovasz_classes=self.lovasz_classes,
                lovasz_per_image=self.lovasz_per_image, dice_weight=self.dice_weight, smooth=self.dice_smooth,
                include_background=self.dice_include_background, grad_scale=grad_scale,
                interpolate_pos_encoding=self.interpolate_pos_encoding, return_terms=True, **opts)
            if stage is not None:
                self.logged[f"{stage}_ce"], self.logged[f"{stage}_dice"], self.logged[f"{stage}_lovasz"] = ce, dice, lov
            return loss
        if self.cldice_weight != 0.0:
            loss, ce, dice, cld = self.model.ce_cldice_loss(
                x, y, cldice_weight=self.cldice_weight, cldice_classes=self.cldice_classes, cldice_iters=self.cldice_iters,
                cldice_smooth=self.cldice_smooth, dice_weight=self.dice_weight, smooth=self.dice_smooth,
                include_background=self.dice_include_background, grad_scale=grad_scale,
                interpolate_pos_encoding=self.interpolate_pos_encoding, return_terms=True, **opts)
            if stage is not None:
                self.logged[f"{stage}_ce"], self.logged[f"{stage}_dice"], self.logged[f"{stage}_cldice"] = ce, dice, cld
            return loss
        if self.dice_weight != 0.0:
            loss, ce, dice = self.model.ce_dice_loss(
                x, y, dice_weight=self.dice_weight, smooth=self.dice_smooth, include_background=self.dice_include_background,
                grad_scale=grad_scale, interpolate_pos_encoding=self.interpolate_pos_encoding, return_terms=True, **opts)
            if stage is not None:
                self.logged[f"{stage}_ce"], self.logged[f"{stage}_dice"] = ce, dice
            return loss
        if self.hard:
            if stage == "train":
                loss, stats = self.model.ce_loss(
                    x, y, grad_scale=grad_scale, interpolate_pos_encoding=self.interpolate_pos_encoding,
                    focal_gamma=self.focal_gamma, ohem_thresh=self.ohem_thresh, ohem_min_kept=self.ohem_min_kept,
                    ohem_keep_fraction=self.ohem_keep_fraction, return_stats=True, **opts)
                self.logged["train_kept"] = stats[2].double() / stats[0].double()
                return loss
            return self.model.ce_loss(x, y, grad_scale=grad_scale, interpolate_pos_encoding=self.interpolate_pos_encoding,
                                      focal_gamma=self.focal_gamma, **opts)   # OHEM off
        if self.interpolate_pos_encoding:
            return self.model.ce_loss(x, y, grad_scale=grad_scale, interpolate_pos_encoding=True, **opts)
        return self.model.ce_loss(x, y, grad_scale=grad_scale, **opts)

    # `logged` holds DEVICE scalars: reading one (float(...)) is the only host sync, and only the caller decides when
    def training_step(self, batch, batch_idx, grad_scale=None):
        loss = self._loss(batch, grad_scale, stage="train", augment=self.augment)
        self.logged["train_loss"] = loss.detach()
        return loss

    def validation_step(self, batch, batch_idx):
        with torch.no_grad():
            loss = self._loss(batch, stage="valid")
        self.logged["valid_loss"] = loss
        return loss

    def configure_optimizers(self):
        from .optim import FusedAdam, configure
        if self.optim_options:
            opt, sched = configure(self.model, 1e-5, self.optim_options)
            return opt if sched is None else {"optimizer": opt, "lr_scheduler": sched}
        return FusedAdam(self.parameters(), lr=1e-5)  # Adam(lr=1e-5), classes.py:296-297

    # checkpoint schema: every key prefixed with "model." like the reference module tree
    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):
        return self.model.state_dict(destination=destination, prefix=prefix + "model.", keep_vars=keep_vars)

    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        return self.model.load_state_dict(state_dict, strict=strict)
