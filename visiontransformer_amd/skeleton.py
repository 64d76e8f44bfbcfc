"""Skeletons of binary masks on the device: what the reference's `CrackSeg.skeletonize` (model/PAED/segmentation.py:89-111)
gets from `skimage.morphology.skeletonize`, one image at a time on the host.  One call of `vitseg_skeleton`
(csrc/skeleton.hip) thins a whole uint8 batch by the algorithm that function cites, exactly as published (T. Y. Zhang and
C. Y. Suen, "A Fast Parallel Algorithm for Thinning Digital Patterns", CACM 1984; the rules are in include/vitseg.h).  Its
known quirks come with it: an isolated 2 x 2 square vanishes, and a full rectangle thins to a short segment or a single pixel.

While the bit-packed plane fits one workgroup's LDS (1024 x 1024 on the MI355X) the call is a single launch without any
host synchronisation; larger planes (`predict_mask_windowed` produces them) take the global route, which reads a convergence
word on the host every 16 passes and therefore synchronises the stream.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .sdf import MAX_SIDE, _checked

MAX_BATCH = 32767
ROUTES = {"auto": _lib.SKELETON_AUTO, "resident": _lib.SKELETON_RESIDENT, "global": _lib.SKELETON_GLOBAL}


def _launch(m: torch.Tensor, route: int, want_passes: bool):
    """Enqueues one vitseg_skeleton call on the current stream for a contiguous device uint8 [n, H, W] mask."""
    n, H, W = (int(d) for d in m.shape)
    dev = m.device
    with torch.cuda.device(dev):
        nbytes = _lib.symbol("vitseg_skeleton_scratch_bytes")(n, H, W, route)
        if nbytes == 0:
            raise ValueError(f"skeletonize: a {H} x {W} plane does not fit the resident route (or n = {n} is outside "
                             f"1..{MAX_BATCH})")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
        passes = torch.empty(n, dtype=torch.int32, device=dev) if want_passes else None
        _lib.check(_lib.symbol("vitseg_skeleton")(m.data_ptr(), n, H, W, route, out.data_ptr(),
                                                  None if passes is None else passes.data_ptr(),
                                                  scratch.data_ptr(), nbytes,
                                                  torch.cuda.current_stream(dev).cuda_stream))
    return out, passes


@torch.no_grad()
def skeletonize(mask, device=None, route: str = "auto", return_passes: bool = False):
    """The Zhang-Suen skeleton of a binary mask [H, W] or of each mask of a batch [n, H, W]: a uint8 array of 0 / 1 of the same
    kind (numpy in, numpy out; torch in, a tensor on the device) and shape.  uint8 and bool masks are read as they are
    (non-zero = mask pixel), any other dtype as `mask != 0`.  A CUDA tensor stays on its device, anything else goes to
    `device` (default cuda:0).  route: "auto", "resident" (ValueError when the plane does not fit) or "global".
    return_passes: also the int32 [n] passes each mask took, the final pass that deleted nothing included.
    Raises ValueError for an empty mask, a rank other than 2 or 3, H or W outside 1..16384 or more than 32767 masks."""
    if route not in ROUTES:
        raise ValueError(f"route must be one of {sorted(ROUTES)}, got {route!r}")
    as_numpy = isinstance(mask, np.ndarray)
    m, single = _checked(mask)
    if m.shape[0] > MAX_BATCH:
        raise ValueError(f"at most {MAX_BATCH} masks per call, got {m.shape[0]}")
    if not m.is_cuda:
        m = m.to(device or "cuda:0")
    out, passes = _launch(m.contiguous(), ROUTES[route], return_passes)
    if single:
        out = out[0]
    if as_numpy:
        out = out.cpu().numpy()
        passes = None if passes is None else passes.cpu().numpy()
    return (out, passes) if return_passes else out


class CrackSeg:
    """The reference's call surface (model/PAED/segmentation.py:89-111)."""

    @staticmethod
    def skeletonize(mask: torch.Tensor) -> torch.Tensor:
        """A 2-D tensor with values in [0, 1] or binary -> the float 0 / 1 skeleton of `mask > 0.5`, on the mask's device.
        The thinning runs on the GPU (a host tensor goes to cuda:0 and comes back)."""
        if not isinstance(mask, torch.Tensor) or mask.dim() != 2:
            raise ValueError("mask must be a 2-D torch.Tensor")
        m = (mask.detach() > 0.5).to(torch.uint8)
        return skeletonize(m).float().to(mask.device)


__all__ = ["skeletonize", "CrackSeg", "MAX_SIDE", "MAX_BATCH"]
