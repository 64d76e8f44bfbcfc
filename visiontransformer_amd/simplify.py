"""Line simplification on the device: Douglas-Peucker over the rings of `polygons.region_polygons`, the polylines of
`centerlines.trace` and a caller's own geometry, between the tracing call and the copy to the host.

The rule is stated in include/vitseg_simplify.h and is exact integer geometry: the distance of a point is to the segment
between its kept neighbours (a thin hook past the end of the base is not lost), the point of largest distance wins a base
(the smallest index among equals), the ends of open lines are always kept, a closed line is anchored at its first point and
the point farthest from it and each of its two halves is split at least once, so a ring never degenerates to two points.  Two
limits: lines are simplified independently of each other, so neighbouring regions may gap or overlap by up to the tolerance
along a shared border, and a simplified ring may come to touch or cross itself (a ring whose kept points would have no area
or one of the other sign is returned as it is, so outer rings stay positive and holes negative).  One call of `vitseg_simplify_lines`
(csrc/simplify.hip) simplifies every line of a whole batch.  The usual host answer is cv2.approxPolyDP per contour, shapely's
simplify(preserve_topology=False) or skimage.measure.approximate_polygon per line.
"""
from __future__ import annotations

import math
from typing import List, Sequence

import numpy as np
import torch

from . import _ext, _lib

SHORT = 64        # include/vitseg_simplify.h VITSEG_SIMPLIFY_SHORT: the longest line handled by one wave
RESIDENT = 2048   # VITSEG_SIMPLIFY_RESIDENT: the longest line handled inside LDS
MAX_TOLERANCE = 32768.0   # pixels: tol2_q8 at most 2^38
MAX_COORD = 16384
MAX_BATCH, MAX_LINES, MAX_POINTS = 65535, 1 << 24, 1 << 30
RING_COLS = (1, 2, -1)     # (offset_col, count_col, closed_col) of vitseg_region_polygons' ring rows: every line is closed
BRANCH_COLS = (2, 3, 4)    # of vitseg_centerlines' branch rows: kind 1 is closed
OUT_FIELDS = ("offset", "points", "points_full", "area2", "ymin", "xmin", "ymax", "xmax")


class Simplified(list):
    """The list `region_polygons` / `trace` return in place of a plain one when they simplified: the same items, plus
    `tolerance` (pixels) and `full`, the number of points of every item before the simplification (per region: all its
    rings).  The GeoJSON writers read both."""

    def __init__(self, items, tolerance, full):
        super().__init__(items)
        self.tolerance = float(tolerance)
        self.full = [int(v) for v in full]


def _symbol(name: str):
    return _ext.ext_symbol("simplify", name)


def tol2_q8(tolerance) -> int:
    """The tolerance (pixels) squared in 1/256 px^2, round(tolerance^2 * 256), as the library takes it.  Raises ValueError for
    anything but a finite real number in 0..32768."""
    if isinstance(tolerance, (bool, np.bool_)) or not isinstance(tolerance, (int, float, np.integer, np.floating)):
        raise ValueError(f"the simplification tolerance must be a number of pixels, got {tolerance!r}")
    t = float(tolerance)
    if not math.isfinite(t) or t < 0.0 or t > MAX_TOLERANCE:
        raise ValueError(f"the simplification tolerance must be finite and in 0..{MAX_TOLERANCE:g} pixels, got {tolerance!r}")
    return int(round(t * t * 256.0))


def _check_cols(cols, row_stride: int):
    try:
        oc, cc, kc = (int(c) for c in cols)
    except (TypeError, ValueError):
        raise ValueError(f"cols must be (offset_col, count_col, closed_col), got {cols!r}") from None
    if not (0 <= oc < row_stride and 0 <= cc < row_stride and oc != cc and -1 <= kc < row_stride):
        raise ValueError(f"cols {cols!r} do not fit rows of {row_stride} words")
    return oc, cc, kc


@torch.no_grad()
def simplify_device(points: torch.Tensor, lines: torch.Tensor, line_counts: torch.Tensor, cols, tolerance, max_out_points=None):
    """Enqueues one vitseg_simplify_lines call on the current stream (no host sync) for contiguous device tensors: points int32
    [n, max_points, 2..4] of (y, x, extra ...), lines int64 [n, max_lines, row_stride], line_counts int32 [n]; cols =
    (offset_col, count_col, closed_col) names the columns of a row, closed_col -1 for lines that are all closed (RING_COLS,
    BRANCH_COLS).  Returns (out_counts int64 [n]: the kept points of each image; out_lines int64 [n, max_lines, 8]: OUT_FIELDS;
    out_points int32 [n, max_out_points, stride]: the kept points, line after line).  max_out_points defaults to max_points, 0
    is a count query.  Arguments are validated before the library is asked for anything."""
    q = tol2_q8(tolerance)
    for name, t, dtype, dims in (("points", points, torch.int32, 3), ("lines", lines, torch.int64, 3),
                                 ("line_counts", line_counts, torch.int32, 1)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or t.dim() != dims:
            raise ValueError(f"{name} must be a {dims}-d {dtype} tensor, got "
                             f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
        if not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous device tensor")
    n, max_points, stride = (int(d) for d in points.shape)
    if int(lines.shape[0]) != n or int(line_counts.shape[0]) != n or lines.device != points.device or line_counts.device != points.device:
        raise ValueError(f"points, lines and line_counts must hold the same {n} images on one device")
    max_lines, row_stride = int(lines.shape[1]), int(lines.shape[2])
    if not 2 <= stride <= 4 or not 1 <= row_stride <= 64:
        raise ValueError(f"points must have 2..4 columns and lines 1..64, got {stride} and {row_stride}")
    oc, cc, kc = _check_cols(cols, row_stride)
    if not 1 <= n <= MAX_BATCH or max_lines > MAX_LINES or max_points > MAX_POINTS:
        raise ValueError(f"simplify takes at most {MAX_BATCH} images of at most 2^24 lines and 2^30 points, got {n} x {max_lines} "
                         f"lines, {max_points} points")
    cap = max_points if max_out_points is None else int(max_out_points)
    if cap < 0:
        raise ValueError(f"max_out_points must not be negative, got {max_out_points!r}")
    dev = points.device
    with torch.cuda.device(dev):
        out_counts = torch.empty(n, dtype=torch.int64, device=dev)
        out_lines = torch.empty((n, max_lines, 8), dtype=torch.int64, device=dev)
        out_points = torch.empty((n, cap, stride), dtype=torch.int32, device=dev)
        if max_lines == 0 or max_points == 0:   # nothing to hand over: no line can hold a point
            return out_counts.zero_(), out_lines.zero_(), out_points.zero_()
        nbytes = _symbol("vitseg_simplify_scratch_bytes")(n, max_lines, max_points)
        scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _lib.check(_symbol("vitseg_simplify_lines")(
            points.data_ptr(), max_points, stride, lines.data_ptr(), max_lines, row_stride, oc, cc, kc, line_counts.data_ptr(), n, q,
            out_counts.data_ptr(), out_lines.data_ptr(), out_points.data_ptr() if cap > 0 else None, cap, scratch.data_ptr(),
            nbytes, torch.cuda.current_stream(dev).cuda_stream))
    return out_counts, out_lines, out_points


def kept_to_host(out_counts: torch.Tensor, out_lines: torch.Tensor, out_points: torch.Tensor):
    """The host copies of `simplify_device`'s outputs: (counts [n], line rows [n, max_lines, 8], the kept slice of the points
    [n, largest count, stride]).  The read of the counts is the only wait before the slice is known."""
    counts = out_counts.cpu().numpy()
    top = min(int(counts.max()) if len(counts) else 0, int(out_points.shape[1]))
    return counts, out_lines.cpu().numpy(), out_points[:, :top].cpu().numpy()


def simplify(polylines: Sequence, tolerance, closed: bool = False, device="cuda:0") -> List[np.ndarray]:
    """Simplifies a caller's own geometry: `polylines` is a sequence of integer [v, 2..4] arrays of (y, x, extra ...) with the
    same number of columns and 0 <= y, x <= 16384, all open (closed=False: the two ends are kept) or all closed (closed=True:
    the last point joins the first and is not repeated).  Returns the list of int32 arrays of the kept points, in order, with
    their extra columns.  One call simplifies them all.  Raises ValueError before the library is asked for anything."""
    q = tol2_q8(tolerance)
    del q
    if not isinstance(closed, (bool, np.bool_)):
        raise ValueError(f"closed must be True or False, got {closed!r}")
    arrays = []
    for i, p in enumerate(polylines):
        a = np.asarray(p)
        if a.ndim != 2 or not 2 <= a.shape[1] <= 4 or a.shape[0] < 1 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"polyline {i} must be an integer [v, 2..4] array with at least one point, got {a.dtype} {a.shape}")
        if arrays and a.shape[1] != arrays[0].shape[1]:
            raise ValueError(f"polyline {i} has {a.shape[1]} columns, the first has {arrays[0].shape[1]}")
        if int(a[:, :2].min()) < 0 or int(a[:, :2].max()) > MAX_COORD:
            raise ValueError(f"polyline {i} has coordinates outside 0..{MAX_COORD}")
        if int(np.abs(a).max()) > np.iinfo(np.int32).max:
            raise ValueError(f"polyline {i} has a column outside int32")
        arrays.append(a.astype(np.int32))
    if not arrays:
        return []
    counts = np.array([len(a) for a in arrays], np.int64)
    rows = np.stack([np.cumsum(counts) - counts, counts, np.full(len(arrays), int(closed), np.int64)], axis=1)
    out_counts, out_lines, out_points = simplify_device(
        torch.from_numpy(np.concatenate(arrays)[None]).to(device), torch.from_numpy(rows[None]).to(device),
        torch.tensor([len(arrays)], dtype=torch.int32, device=device), (0, 1, 2), tolerance)
    _, lines, pts = kept_to_host(out_counts, out_lines, out_points)
    return [np.ascontiguousarray(pts[0, int(o):int(o + c)]) for o, c in zip(lines[0, :, 0], lines[0, :, 1])]


__all__ = ["tol2_q8", "simplify_device", "simplify", "kept_to_host", "Simplified", "SHORT", "RESIDENT", "RING_COLS", "BRANCH_COLS", "OUT_FIELDS"]
