"""Connected regions of class masks and their boxes, on the device: the arithmetic of the reference's "Predicted Regions
with Boxes" panel.

The reference's three inference scripts (model/CE/testViTModel.py:34-42,171-185, model/CE/datasetTestViTmodel.py:27,315-318,
model/PAED/ViTscriptTest.py:27,318-321) run `get_bounding_boxes` -- scipy.ndimage.label on `pred == c`, then np.argwhere
per label -- for every class present in the prediction except 0, in ascending class order.  Here one call of
`vitseg_regions` (csrc/regions.hip) labels every class of a whole batch at once and returns, per image, one record per
region: (class, y_min, x_min, y_max, x_max, area, first), box inclusive, `first` = raster index of the region's first
pixel, in (class, first) order -- exactly the order in which the reference's loop emits its boxes.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _lib

FIELDS = ("class", "y_min", "x_min", "y_max", "x_max", "area", "first")
DEFAULT_MAX_REGIONS = 1024   # records per image on the first call; an image with more triggers one call at its count


def _checked(mask, background: int, connectivity: int) -> Tuple[torch.Tensor, bool]:
    """Validates the arguments before anything reaches the library; returns the mask as [n, H, W] and whether it was 2-D."""
    if isinstance(mask, np.ndarray):
        mask = torch.from_numpy(mask)
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"mask must be a torch.Tensor or numpy array, got {type(mask).__name__}")
    if mask.dtype not in (torch.uint8, torch.int64):
        raise ValueError(f"mask must be uint8 or int64 (long), got {mask.dtype}")
    if mask.dim() not in (2, 3):
        raise ValueError(f"mask must be [n, H, W] or [H, W], got shape {tuple(mask.shape)}")
    if mask.numel() == 0:
        raise ValueError(f"mask must not be empty, got shape {tuple(mask.shape)}")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity}")
    if isinstance(background, bool) or not isinstance(background, (int, np.integer)) or not -1 <= int(background) <= 255:
        raise ValueError(f"background must be an integer in 0..255 or -1 (none), got {background!r}")
    single = mask.dim() == 2
    if single:
        mask = mask[None]
    H, W = int(mask.shape[1]), int(mask.shape[2])
    if H * W >= 1 << 31:
        raise ValueError(f"an image of {H} x {W} pixels exceeds the 2^31 - 1 pixels of one image")
    if mask.dtype == torch.int64:
        lo, hi = int(mask.min()), int(mask.max())
        if lo < 0 or hi > 255:
            raise ValueError(f"mask values must lie in 0..255, got {lo}..{hi}")
    return mask, single


def _launch(m: torch.Tensor, background: int, connectivity: int, max_regions: int, want_labels: bool):
    """Enqueues one vitseg_regions call on the current stream (no host sync): (counts, regions, labels or None)."""
    n, H, W = (int(d) for d in m.shape)
    dev = m.device
    scratch = torch.empty(_lib.region_symbol("vitseg_regions_scratch_bytes")(n, H, W), dtype=torch.uint8, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    regions = torch.empty((n, max_regions, 8), dtype=torch.int32, device=dev)
    labels = torch.empty((n, H, W), dtype=torch.int32, device=dev) if want_labels else None
    _lib.check(_lib.region_symbol("vitseg_regions")(
        m.data_ptr(), n, H, W, connectivity, background, counts.data_ptr(),
        regions.data_ptr() if max_regions > 0 else None, max_regions,
        labels.data_ptr() if labels is not None else None, scratch.data_ptr(), scratch.numel(),
        torch.cuda.current_stream(dev).cuda_stream))
    return counts, regions, labels


@torch.no_grad()
def region_boxes(mask, *, background: int = 0, connectivity: int = 4, return_labels: bool = False,
                 device="cuda:0"):
    """Regions of a class mask uint8 / long [n, H, W] or [H, W] (what `predict_mask` returns, or any label map with
    values 0..255): a list of one int32 [k, 7] numpy array per image (the array itself for a [H, W] mask), rows (class, y_min, x_min, y_max, x_max, area, first) in
    (class, first) order.  `background` (default 0, as the reference's `if class_idx == 0: continue`; -1 = none) forms
    no region; `connectivity` 4 (scipy's default structure, the reference's) or 8.  `return_labels`: also the int32
    [n, H, W] (or [H, W]) device tensor of region indices, -1 on background.  A host tensor is copied to `device`.
    The records of a batch come from one launch sequence; the only host sync is the read of the counts (an image with
    more than DEFAULT_MAX_REGIONS regions makes one more call sized to the largest count: the same bits)."""
    m, single = _checked(mask, background, connectivity)
    if not m.is_cuda:
        m = m.to(device)
    m = m.to(torch.uint8).contiguous()
    background = int(background)
    counts, regions, labels = _launch(m, background, connectivity, DEFAULT_MAX_REGIONS, return_labels)
    cnt = counts.cpu().numpy()
    if int(cnt.max()) > DEFAULT_MAX_REGIONS:
        counts, regions, labels = _launch(m, background, connectivity, int(cnt.max()), return_labels)
    rec = regions[:, :int(cnt.max()), :7].cpu().numpy()
    out = [np.ascontiguousarray(rec[i, :int(cnt[i])]) for i in range(len(cnt))]
    if single:
        out, labels = out[0], (labels[0] if labels is not None else None)
    return (out, labels) if return_labels else out


def boxes_by_class(records) -> Dict[int, List[Tuple[int, int, int, int]]]:
    """{class: [(y_min, x_min, y_max, x_max), ...]} from one image's records: exactly what the reference's loop builds
    from get_bounding_boxes, class by class in ascending order (testViTModel.py:171-185)."""
    out: Dict[int, List[Tuple[int, int, int, int]]] = {}
    for r in np.asarray(records):
        out.setdefault(int(r[0]), []).append((int(r[1]), int(r[2]), int(r[3]), int(r[4])))
    return out
