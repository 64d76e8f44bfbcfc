"""Mask clean-up on the device: regions below a minimum area become background, enclosed holes are filled.

The masks `predict_mask` returns are decided pixel by pixel, so they carry islands of a few pixels and pinholes inside solid
regions; every consumer of the mask (the boxes panel, the crack and distance metrics, the worker's PNG) takes them at face
value.  The reference has the same speckle and no answer to it (its get_bounding_boxes labels the raw argmax,
model/CE/testViTModel.py:34-42); the usual host answer is remove_small_objects + scipy.ndimage.binary_fill_holes per class
and image.  Here one call of `vitseg_clean_mask` (csrc/clean.hip) does both for a whole batch, on the labelling launches of
csrc/regions.hip:

1. `min_area`: every region (regions.region_boxes' regions: maximal `connectivity`-connected sets of equal non-background
   pixels) of fewer than `min_area` pixels becomes `background`.
2. `fill_holes`, on the result of step 1: a hole is a 4-connected component of background pixels that does not touch the
   image frame (4-connected whatever `connectivity` is: binary_fill_holes' default structure).  A hole of at most
   `max_hole_area` pixels (0: no limit) whose non-background 4-neighbours all carry one class takes that class; a hole
   bordered by two or more classes stays background.
"""
from __future__ import annotations

import argparse

import numpy as np
import torch

from . import _common, _lib
from .regions import _checked

STATS = _lib.CLEAN_STATS


def _count(name: str, v) -> int:
    return _common.integer(name, v, 0, (1 << 31) - 1, "0..2^31 - 1")


def check_options(min_area=0, fill_holes=False, max_hole_area=0, connectivity: int = 4, background: int = 0):
    """Validates the clean-up options without a mask (what `worker.gpu_slot` refuses when the slot is built); returns
    (min_area, fill_holes, max_hole_area) as (int, bool, int).  ValueError otherwise."""
    min_area, max_hole_area = _count("min_area", min_area), _count("max_hole_area", max_hole_area)
    if not isinstance(fill_holes, (bool, np.bool_)):
        raise ValueError(f"fill_holes must be a bool, got {fill_holes!r}")
    _common.connectivity(connectivity)
    _common.integer("background", background, 0, 255, "0..255 (clean-up needs a background)")
    return min_area, bool(fill_holes), max_hole_area


def active(min_area=0, fill_holes=False) -> bool:
    """Whether these options change anything: min_area 0 and 1 remove nothing."""
    return int(min_area) > 1 or bool(fill_holes)


@torch.no_grad()
def clean_mask(mask, *, min_area: int = 0, fill_holes: bool = False, max_hole_area: int = 0, connectivity: int = 4,
               background: int = 0, return_stats: bool = False, device="cuda:0"):
    """The cleaned label map of a class mask uint8 / long [n, H, W] or [H, W] (torch or numpy; values 0..255): a device
    tensor of the input's dtype and rank.  `min_area` (default 0 = off; 0 and 1 change nothing): regions of fewer pixels
    become `background`, a region of exactly `min_area` pixels stays.  `fill_holes`: then the enclosed holes of at most
    `max_hole_area` pixels (0 = no limit) with one bordering class take that class.  `connectivity` 4 or 8 is that of the
    regions of step 1; holes are 4-connected always.  `background` 0..255 (there is no "none").
    `return_stats`: also a list of one dict per image (the dict itself for a [H, W] mask) with the keys of STATS --
    regions_removed, pixels_removed, holes_filled, pixels_filled, holes_mixed (left: two or more bordering classes),
    holes_over_area (left: above max_hole_area, mixed or not); reading them is the only host sync, without it there is none.
    With both steps off the input itself is returned (zero statistics) and nothing is launched.  A host tensor is copied to
    `device`.  Exact and reproducible to the bit; an image gets the same result alone as in a batch."""
    min_area, fill_holes, max_hole_area = check_options(min_area, fill_holes, max_hole_area, connectivity, background)
    m, single = _checked(mask, background, connectivity)
    background = int(background)
    n, H, W = (int(d) for d in m.shape)
    if not active(min_area, fill_holes):
        if not return_stats:
            return mask
        zero = [dict.fromkeys(STATS, 0) for _ in range(n)]
        return mask, (zero[0] if single else zero)
    dtype = m.dtype
    if not m.is_cuda:
        m = m.to(device)
    m = m.to(torch.uint8).contiguous()
    dev = m.device
    out = torch.empty_like(m)
    stats = torch.empty((n, 8), dtype=torch.int32, device=dev) if return_stats else None
    scratch = torch.empty(_lib.symbol("vitseg_clean_scratch_bytes")(n, H, W), dtype=torch.uint8, device=dev)
    _lib.check(_lib.symbol("vitseg_clean_mask")(
        m.data_ptr(), out.data_ptr(), n, H, W, connectivity, background, min_area, int(fill_holes), max_hole_area,
        stats.data_ptr() if stats is not None else None, scratch.data_ptr(), scratch.numel(),
        torch.cuda.current_stream(dev).cuda_stream))
    out = out.to(dtype)
    if single:
        out = out[0]
    if not return_stats:
        return out
    st = [dict(zip(STATS, (int(v) for v in row[:len(STATS)]))) for row in stats.cpu().numpy()]
    return out, (st[0] if single else st)


def _nonneg(text: str) -> int:
    try:
        v = int(text)
    except ValueError:
        v = -1
    if v < 0:
        raise argparse.ArgumentTypeError(f"a non-negative integer is expected, got {text!r}")
    return v


def add_arguments(ap: argparse.ArgumentParser) -> None:
    """--min-area / --fill-holes / --max-hole-area of the worker and the evaluation scripts."""
    ap.add_argument("--min-area", type=_nonneg, default=0,
                    help="mask clean-up: predicted regions of fewer pixels become background (default 0: off)")
    ap.add_argument("--fill-holes", action="store_true",
                    help="mask clean-up: enclosed background holes bordered by one class take that class")
    ap.add_argument("--max-hole-area", type=_nonneg, default=0,
                    help="with --fill-holes: only holes of at most this many pixels are filled (default 0: no limit)")


def arguments(a: argparse.Namespace) -> dict:
    """The keywords min_area / fill_holes / max_hole_area from a namespace parsed after `add_arguments`."""
    return dict(min_area=a.min_area, fill_holes=a.fill_holes, max_hole_area=a.max_hole_area)
