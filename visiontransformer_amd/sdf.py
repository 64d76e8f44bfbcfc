"""Exact Euclidean distance transforms and the signed-distance targets of binary masks, on the device: the arithmetic of
the reference's `segmentation.compute_sdf` (model/PAED/segmentation.py:6-34), which the binary PAED dataset runs for every
item (model/PAED/classes.py:51-85):

    m = mask.astype(bool)
    sdf_ext = distance_transform_edt(~m).astype(float32)    # non-mask pixels: distance to the nearest mask pixel
    sdf_int = distance_transform_edt(m).astype(float32)     # mask pixels: distance to the nearest non-mask pixel
    each divided by its maximum when that is > 0

One call of `vitseg_sdf` (csrc/sdf.hip) computes both fields of a whole uint8 batch with an exact separable EDT (Meijster,
Roerdink & Hesselink 2000) in integer arithmetic, then takes the root in float64 and casts, as scipy does: the results are
bitwise scipy's, including its result for a field without any feature pixel (the distance to the virtual point (-1, 0)).
"""
from __future__ import annotations

from typing import Tuple

import numpy as np
import torch

from . import _lib

MAX_SIDE = 16384     # H and W: 1 .. MAX_SIDE
MAX_BATCH = 65535


def _checked(mask) -> Tuple[torch.Tensor, bool]:
    """Validates the mask before anything reaches the library; returns it as uint8 [n, H, W] (non-zero = mask pixel) and
    whether it was 2-D."""
    if isinstance(mask, np.ndarray):
        mask = torch.from_numpy(np.ascontiguousarray(mask))
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"mask must be a torch.Tensor or numpy array, got {type(mask).__name__}")
    if mask.dim() not in (2, 3):
        raise ValueError(f"mask must be [n, H, W] or [H, W], got shape {tuple(mask.shape)}")
    if mask.numel() == 0:
        raise ValueError(f"mask must not be empty, got shape {tuple(mask.shape)}")
    single = mask.dim() == 2
    if single:
        mask = mask[None]
    n, H, W = (int(d) for d in mask.shape)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"H and W must lie in 1..{MAX_SIDE}, got {H} x {W}")
    if n > MAX_BATCH:
        raise ValueError(f"at most {MAX_BATCH} masks per call, got {n}")
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    elif mask.dtype != torch.uint8:
        mask = (mask != 0).to(torch.uint8)
    return mask, single


def _launch(m: torch.Tensor, normalize: bool):
    """Enqueues one vitseg_sdf call on the current stream for a contiguous device uint8 [n, H, W] mask: (sdf_ext, sdf_int),
    float32 [n, H, W] each."""
    n, H, W = (int(d) for d in m.shape)
    dev = m.device
    scratch = torch.empty(_lib.symbol("vitseg_sdf_scratch_bytes")(n, H, W), dtype=torch.uint8, device=dev)
    e = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    i = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.symbol("vitseg_sdf")(m.data_ptr(), n, H, W, int(bool(normalize)), e.data_ptr(), i.data_ptr(),
                                             scratch.data_ptr(), scratch.numel(), torch.cuda.current_stream(dev).cuda_stream))
    return e, i


@torch.no_grad()
def compute_sdf(mask, normalize: bool = True, device=None):
    """(sdf_ext, sdf_int) of a binary mask [H, W] or a batch [n, H, W], bitwise what the reference's
    `segmentation.compute_sdf` returns for each image alone; `normalize=False` gives the raw `distance_transform_edt(~m)`
    and `distance_transform_edt(m)` as float32.  uint8 and bool masks are read as they are (non-zero = mask pixel); any
    other dtype is taken as `mask != 0`.  numpy in: numpy float32 out, computed on `device` (default cuda:0).  torch in:
    float32 tensors on the device; a CUDA tensor stays on its own, a host tensor goes to `device` (default cuda:0).
    Raises ValueError for an empty mask, a rank other than 2 or 3, H or W outside 1..16384 or more than 65535 masks."""
    as_numpy = isinstance(mask, np.ndarray)
    m, single = _checked(mask)
    if not m.is_cuda:
        m = m.to(device or "cuda:0")
    e, i = _launch(m.contiguous(), normalize)
    if single:
        e, i = e[0], i[0]
    if as_numpy:
        return e.cpu().numpy(), i.cpu().numpy()
    return e, i
