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
import math
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _common, _lib

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
    _common.connectivity(connectivity)
    _common.integer("background", background, -1, 255, "0..255 or -1 (none)")
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
    scratch = torch.empty(_lib.symbol("vitseg_regions_scratch_bytes")(n, H, W), dtype=torch.uint8, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    regions = torch.empty((n, max_regions, 8), dtype=torch.int32, device=dev)
    labels = torch.empty((n, H, W), dtype=torch.int32, device=dev) if want_labels else None
    _lib.check(_lib.symbol("vitseg_regions")(
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


# ---- per-region measurements (vitseg_region_props, csrc/props.hip) ----

PROPS_FIELDS = ("class", "first", "area", "y_min", "x_min", "y_max", "x_max", "sum_y", "sum_x", "sum_yy", "sum_xx", "sum_xy",
                "perimeter", "frame_pixels", "max_d2", "skel_len", "end_points", "skel_max_d2", "skel_width_q16", "reserved")
PROPS_ROUTES = {"auto": _lib.SKELETON_AUTO, "resident": _lib.SKELETON_RESIDENT, "global": _lib.SKELETON_GLOBAL}
PROPS_MAX_SIDE, PROPS_MAX_BATCH = 16384, 32767
PROPS_KEYS = ("class", "box", "area", "centroid", "major_axis", "minor_axis", "orientation", "eccentricity", "extent",
              "perimeter", "compactness", "touches_frame", "thickness_max", "length", "width_mean", "width_max", "end_points")


def _checked_props(mask, skeleton_classes, background: int, connectivity: int, route: str):
    """`_checked` plus the arguments of `region_props` alone: (mask [n, H, W], single, the classes or "all")."""
    m, single = _checked(mask, background, connectivity)
    if route not in PROPS_ROUTES:
        raise ValueError(f"route must be one of {sorted(PROPS_ROUTES)}, got {route!r}")
    n, H, W = (int(d) for d in m.shape)
    if H > PROPS_MAX_SIDE or W > PROPS_MAX_SIDE or n > PROPS_MAX_BATCH:
        raise ValueError(f"region_props takes at most {PROPS_MAX_BATCH} images of at most {PROPS_MAX_SIDE} x {PROPS_MAX_SIDE} "
                         f"pixels, got {n} x {H} x {W}")
    if skeleton_classes is None:
        return m, single, []
    if isinstance(skeleton_classes, str):
        if skeleton_classes != "all":
            raise ValueError(f'skeleton_classes must be None, "all" or a sequence of label values, got {skeleton_classes!r}')
        return m, single, "all"
    return m, single, _common.label_values("skeleton_classes", skeleton_classes, empty_ok=True, background=int(background))


def _launch_props(m: torch.Tensor, classes, background: int, connectivity: int, route: int, max_regions: int,
                  want_labels: bool):
    """Enqueues one vitseg_region_props call on the current stream (no host sync unless the skeleton's global route
    runs): (counts, props, labels or None)."""
    n, H, W = (int(d) for d in m.shape)
    dev = m.device
    K = len(classes)
    cls = (C.c_int32 * K)(*classes) if K else None
    with torch.cuda.device(dev):
        nbytes = _lib.symbol("vitseg_region_props_scratch_bytes")(n, H, W, K, route)
        if nbytes == 0:
            raise ValueError(f"region_props: a {H} x {W} plane does not fit the resident route of the skeleton (or the shape "
                             f"{n} x {H} x {W} is out of range)")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(n, dtype=torch.int32, device=dev)
        props = torch.empty((n, max_regions, _lib.PROPS_FIELDS), dtype=torch.int64, device=dev)
        labels = torch.empty((n, H, W), dtype=torch.int32, device=dev) if want_labels else None
        _lib.check(_lib.symbol("vitseg_region_props")(
            m.data_ptr(), n, H, W, connectivity, background, cls, K, route, counts.data_ptr(),
            props.data_ptr() if max_regions > 0 else None, max_regions,
            labels.data_ptr() if labels is not None else None, scratch.data_ptr(), nbytes,
            torch.cuda.current_stream(dev).cuda_stream))
    return counts, props, labels


@torch.no_grad()
def region_props(mask, *, skeleton_classes=None, background: int = 0, connectivity: int = 4, route: str = "auto",
                 return_labels: bool = False, device="cuda:0"):
    """Per-region measurements of a class mask uint8 / long [n, H, W] or [H, W]: a list of one int64 [k, 20] numpy array per
    image (the array itself for a [H, W] mask), one row per region in `region_boxes`' (class, first) order, columns
    PROPS_FIELDS: the record, the raw moments sum_y .. sum_xy, the perimeter in pixel sides, the pixels on the image frame and,
    for the classes in `skeleton_classes` (None: none; "all": every non-background value present; else label values), the
    region's maximal squared inscribed radius, its skeleton length, end points, maximal squared half-width on the skeleton and
    the fixed-point sum of the half-widths (include/vitseg.h); -1 in those five columns for every other class.
    `props_from_records` turns the rows into centroids, axes, orientation, lengths and widths.
    Under connectivity 4 two diagonally touching regions of one class are thinned and measured as the one plane they share.
    `background`, `connectivity`, `return_labels`, `device`: as `region_boxes`, and validated the same way.  `route`: the
    skeleton's ("auto", "resident", "global"; the global route synchronises the stream).  Otherwise the only host sync is
    the read of the counts ("all" reads the values present first); an image with more than DEFAULT_MAX_REGIONS regions
    makes one more call sized to the largest count: the same bits."""
    m, single, classes = _checked_props(mask, skeleton_classes, background, connectivity, route)
    if not m.is_cuda:
        m = m.to(device)
    m = m.to(torch.uint8).contiguous()
    background = int(background)
    if classes == "all":
        classes = [int(c) for c in torch.unique(m).cpu().tolist() if int(c) != background]
    args = (m, classes, background, connectivity, PROPS_ROUTES[route])
    counts, props, labels = _launch_props(*args, DEFAULT_MAX_REGIONS, return_labels)
    cnt = counts.cpu().numpy()
    if int(cnt.max()) > DEFAULT_MAX_REGIONS:
        counts, props, labels = _launch_props(*args, int(cnt.max()), return_labels)
    rec = props[:, :int(cnt.max())].cpu().numpy()
    out = [np.ascontiguousarray(rec[i, :int(cnt[i])]) for i in range(len(cnt))]
    if single:
        out, labels = out[0], (labels[0] if labels is not None else None)
    return (out, labels) if return_labels else out


def props_from_records(records, pixel_size: float = 1.0) -> List[dict]:
    """One dict per row of one image's `region_props` array (int64 [k, 20]): host arithmetic on the integers.  The central
    moments are formed exactly, with Python integers (area * sum_yy - sum_y^2 and so on), before the first division.
    Lengths are multiplied by `pixel_size`, areas by its square:
      class, box (y_min, x_min, y_max, x_max; pixels, inclusive), area, centroid (y, x);
      major_axis, minor_axis   4 sqrt(l1), 4 sqrt(l2) of the eigenvalues l1 >= l2 of the covariance matrix of the pixel
                               centres (the axes of the ellipse with the same second moments);
      orientation              atan2(2 v_xy, v_xx - v_yy) / 2: the major axis' angle from the column axis towards the row axis;
      eccentricity             sqrt(1 - l2 / l1) (0 for a single pixel);   extent  area / box area;
      perimeter                the outline in pixel sides, holes included;
      compactness              4 pi area / perimeter^2 -- the pixel-side perimeter overstates a slanted or curved outline, so
                               this is a digital estimate (a disc gets about pi / 4, a square 1 at any size);
      touches_frame            the image frame cuts the region off: its measurements are lower bounds;
      thickness_max            2 sqrt(max_d2) - 1;   length  the skeleton pixels;   end_points;
      width_mean, width_max    2 (skel_width_q16 / 65536) / skel_len - 1 and 2 sqrt(skel_max_d2) - 1, the width convention of
                               metrics.crack_from_stats.
    A quantity that was not measured (the class was not in skeleton_classes) or is empty (no skeleton pixel) is nan."""
    rec = np.asarray(records)
    if rec.ndim != 2 or rec.shape[1] != len(PROPS_FIELDS):
        raise ValueError(f"records must be [k, {len(PROPS_FIELDS)}], got {rec.shape}")
    ps = _common.pixel_size(pixel_size)
    nan = float("nan")
    out = []
    for row in rec:
        (cls, _, a, y0, x0, y1, x1, sy, sx, syy, sxx, sxy, per, frame, max_d2, slen, ends, smax, q16, _) = (int(v) for v in row)
        a2 = a * a
        vyy, vxx, vxy = (a * syy - sy * sy) / a2, (a * sxx - sx * sx) / a2, (a * sxy - sx * sy) / a2
        half, diff = (vxx + vyy) / 2, math.hypot((vxx - vyy) / 2, vxy)
        l1, l2 = half + diff, max(half - diff, 0.0)
        measured = max_d2 >= 0
        out.append({
            "class": cls, "box": (y0, x0, y1, x1), "area": a * ps * ps, "centroid": (sy / a * ps, sx / a * ps),
            "major_axis": 4 * math.sqrt(l1) * ps, "minor_axis": 4 * math.sqrt(l2) * ps,
            "orientation": 0.5 * math.atan2(2 * vxy, vxx - vyy),
            "eccentricity": math.sqrt(max(1 - l2 / l1, 0.0)) if l1 > 0 else 0.0,
            "extent": a / ((y1 - y0 + 1) * (x1 - x0 + 1)), "perimeter": per * ps,
            "compactness": 4 * math.pi * a / (per * per), "touches_frame": frame > 0,
            "thickness_max": (2 * math.sqrt(max_d2) - 1) * ps if measured else nan,
            "length": slen * ps if measured else nan,
            "width_mean": (2 * (q16 / 65536) / slen - 1) * ps if measured and slen else nan,
            "width_max": (2 * math.sqrt(smax) - 1) * ps if measured and slen else nan,
            "end_points": ends if measured else nan,
        })
    return out


# header of <model>_region_props.csv (--region-props of the evaluation scripts): one row per region of either map
PROPS_CSV_COLUMNS = ["Source", "Model_ID", "Model_Name", "Batch_Num", "Image_Idx", "Region", "Class", "Y_Min", "X_Min", "Y_Max",
                     "X_Max", "Area", "Centroid_Y", "Centroid_X", "Major_Axis", "Minor_Axis", "Orientation", "Eccentricity",
                     "Extent", "Perimeter", "Compactness", "Touches_Frame", "Thickness_Max", "Length", "Width_Mean", "Width_Max",
                     "End_Points"]


def props_csv_row(source: str, model_info, batch_num, image_idx, region: int, d: dict) -> list:
    """One row of <model>_region_props.csv from one dict of `props_from_records`; source "pred" or "gt"."""
    return [source, model_info[0], model_info[1], batch_num, image_idx, region, d["class"], *d["box"], d["area"],
            d["centroid"][0], d["centroid"][1], d["major_axis"], d["minor_axis"], d["orientation"], d["eccentricity"],
            d["extent"], d["perimeter"], d["compactness"], int(d["touches_frame"]), d["thickness_max"], d["length"],
            d["width_mean"], d["width_max"], d["end_points"]]


def write_props_csv(path: str, rows) -> None:
    _common.write_csv(path, PROPS_CSV_COLUMNS, rows)
