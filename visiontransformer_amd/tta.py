"""Test-time augmentation: the view list of `ViTSegmentationModel.predict_mask_tta` (include/vitseg.h "test-time
augmentation").

A view is (op, size, weight).  op = 0..7: f = op >> 2 is a horizontal flip applied FIRST, r = op & 3 the number of
counter-clockwise quarter turns,

    view(X, op)   = torch.rot90(torch.flip(X, [-1]) if f else X, r, dims=(-2, -1))
    unview(Y, op) = Z if not f else torch.flip(Z, [-1]),   Z = torch.rot90(Y, -r, dims=(-2, -1))

so op 4 is the horizontal flip, op 6 the vertical flip and op 2 the half turn.  `size` is the side the image is resampled
to before the forward (a multiple of the patch size, not necessarily the model's own); `weight` the view's share of the mean.
The views of a call are sizes x ops, size-major in the order given, ops increasing within a size.

The reference's scripts look at every image once (model/CE/testViTModel.py:92-126); its training side has no augmentation
either.  Here the trainer draws exactly these transforms (augment.Augmenter), and this module lets inference average over
them: the "multi-scale + flip" protocol segmentation results are usually reported under.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

PRESETS = {"none": (0,), "hflip": (0, 4), "flip": (0, 2, 4, 6), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}
MERGES = {"logits": 0, "probs": 1}   # the `mode` argument of vitseg_tta_blend
MAX_VIEWS = 16                       # what one vitseg_tta_blend launch takes


def parse_ops(tta) -> Tuple[int, ...]:
    """The ops of a preset name ("none", "hflip", "flip", "d4"), of one op or of a sequence of ops: distinct, increasing.
    ValueError for an unknown preset or an op outside 0..7."""
    if isinstance(tta, str):
        if tta not in PRESETS:
            raise ValueError(f"unknown TTA preset {tta!r}: one of {sorted(PRESETS)} or a sequence of ops 0..7")
        return PRESETS[tta]
    if isinstance(tta, (int,)) and not isinstance(tta, bool):
        tta = (tta,)
    try:
        ops = [op for op in tta]
    except TypeError:
        raise ValueError(f"tta must be a preset name or a sequence of ops 0..7, got {tta!r}") from None
    for op in ops:
        if isinstance(op, bool) or not isinstance(op, int) or not 0 <= op <= 7:
            raise ValueError(f"unknown TTA op {op!r}: ops are 0..7 (flip = op >> 2, quarter turns = op & 3)")
    if not ops:
        raise ValueError("tta names no view")
    return tuple(sorted(set(ops)))


def parse_sizes(spec) -> Optional[Tuple[int, ...]]:
    """Command-line form of `sizes`: "160,224" -> (160, 224); None or "" -> None (the image's own size)."""
    if spec is None or spec == "":
        return None
    if isinstance(spec, str):
        return tuple(int(v) for v in spec.split(",") if v.strip())
    return tuple(int(v) for v in spec)


def view_list(tta, sizes: Optional[Sequence[int]], weights: Optional[Sequence[float]], S: int, patch_size: int) -> List[tuple]:
    """[(op, size, weight)] of one call: sizes x ops, size-major in the order given, ops increasing within a size.
    `sizes` defaults to (S,); `weights` is one per size, default 1.  ValueError for an unknown preset or op, a size that is
    not a positive multiple of the patch size, a weight that is not finite and > 0, a weight count that differs from the
    size count, or more than 16 views."""
    ops = parse_ops(tta)
    sizes = (int(S),) if sizes is None else tuple(sizes)
    if not sizes:
        raise ValueError("sizes names no size")
    P = int(patch_size)
    for s in sizes:
        if isinstance(s, bool) or int(s) != s or int(s) < P or int(s) % P:
            raise ValueError(f"TTA size {s!r} is not a positive multiple of the patch size {P}.")
    weights = (1.0,) * len(sizes) if weights is None else tuple(weights)
    if len(weights) != len(sizes):
        raise ValueError(f"{len(weights)} weights for {len(sizes)} sizes (one weight per size)")
    for w in weights:
        if not (math.isfinite(float(w)) and float(w) > 0.0):
            raise ValueError(f"TTA weight {w!r} must be finite and > 0")
    views = [(op, int(s), float(w)) for s, w in zip(sizes, weights) for op in ops]
    if len(views) > MAX_VIEWS:
        raise ValueError(f"{len(views)} views ({len(sizes)} sizes x {len(ops)} ops): at most {MAX_VIEWS} merge in one launch")
    return views


def merge_mode(merge: str) -> int:
    if merge not in MERGES:
        raise ValueError(f'merge must be "logits" or "probs", got {merge!r}')
    return MERGES[merge]
