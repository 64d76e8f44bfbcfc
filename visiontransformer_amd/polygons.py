"""Region outlines on the device: every connected region of a class mask as polygon rings with holes, and their GeoJSON.

The regions are `regions.region_boxes`' (same connectivity, background, order); the outline is exact integer geometry on the
pixel-corner lattice, stated in include/vitseg_polygons.h: each region has one outer ring (positive area, starting at the top
left corner of its `first` pixel, the region on the right of the walk) and one ring of negative area per hole; collinear
corners are dropped.  One call of `vitseg_region_polygons` (csrc/polygons.hip) outlines every class of a whole batch.  The
usual host answer is cv2.findContours or skimage.measure.find_contours per class and image.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _common, _ext, _lib
from . import simplify as _simplify
from .regions import _checked

DEFAULT_MAX_RINGS = 1024       # ring rows per image on the first call
DEFAULT_MAX_VERTICES = 65536   # vertices per image on the first call; an image above either makes one call at the true sizes
MAX_SIDE, MAX_PIXELS = 16384, 1 << 29


def _symbol(name: str):
    return _ext.ext_symbol("polygons", name)


def _launch(m: torch.Tensor, background: int, connectivity: int, max_rings: int, max_vertices: int, want_labels: bool):
    """Enqueues one vitseg_region_polygons call on the current stream (no host sync): (counts int32 [4 n]: the region counts,
    the ring counts and, as int64, the vertex counts; rings; vertices; the class at every ring's start; labels or None)."""
    n, H, W = (int(d) for d in m.shape)
    dev = m.device
    with torch.cuda.device(dev):
        nbytes = _symbol("vitseg_region_polygons_scratch_bytes")(n, H, W)
        scratch = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        counts = torch.empty(4 * n, dtype=torch.int32, device=dev)
        rings = torch.empty((n, max_rings, 4), dtype=torch.int64, device=dev)
        vertices = torch.empty((n, max_vertices, 2), dtype=torch.int32, device=dev)
        labels = torch.empty((n, H, W), dtype=torch.int32, device=dev) if want_labels else None
        _lib.check(_symbol("vitseg_region_polygons")(
            m.data_ptr(), n, H, W, connectivity, background, counts.data_ptr(), counts[n:].data_ptr(), counts[2 * n:].data_ptr(),
            rings.data_ptr() if max_rings > 0 else None, max_rings, vertices.data_ptr() if max_vertices > 0 else None,
            max_vertices, labels.data_ptr() if labels is not None else None, scratch.data_ptr(), nbytes,
            torch.cuda.current_stream(dev).cuda_stream))
        # the class of a region is the mask's value under its outer ring's start; read for every ring row, used for those
        start = vertices.to(torch.int64).gather(1, rings[:, :, 1:2].clamp(0, max_vertices - 1).expand(-1, -1, 2))
        cls = m.view(n, -1).gather(1, (start[:, :, 0] * W + start[:, :, 1]).clamp(0, H * W - 1))
    return counts, rings, vertices, cls, labels


def _records(rings: np.ndarray, vertices: np.ndarray, cls: np.ndarray, k: int, W: int):
    """One image: (`region_boxes`' int32 [k, 7] records, polygons) from its ring rows, vertices and ring-start classes."""
    region, off, area = rings[:, 0], rings[:, 1], rings[:, 3]
    outer = np.nonzero(area > 0)[0]
    if len(outer) != k or not np.array_equal(np.sort(region[outer]), np.arange(k)):
        raise RuntimeError(f"region_polygons: {len(outer)} outer rings for {k} regions")
    rec = np.zeros((k, 7), np.int32)
    polygons: List[List[np.ndarray]] = [[] for _ in range(k)]
    if k == 0:
        return rec, polygons
    lo = np.minimum.reduceat(vertices, off, axis=0)[outer]
    hi = np.maximum.reduceat(vertices, off, axis=0)[outer]
    start = vertices[off[outer]].astype(np.int64)
    r = region[outer]
    rec[r, 0] = cls[outer]
    rec[r, 1], rec[r, 2], rec[r, 3], rec[r, 4] = lo[:, 0], lo[:, 1], hi[:, 0] - 1, hi[:, 1] - 1
    np.add.at(rec[:, 5], region, area.astype(np.int32))   # the outline's pixels minus the holes'
    rec[r, 6] = start[:, 0] * W + start[:, 1]
    for i in np.argsort(region, kind="stable"):   # ring order within a region: the outer ring, then its holes
        polygons[int(region[i])].append(np.ascontiguousarray(vertices[int(off[i]):int(off[i] + rings[i, 2])]))
    return rec, polygons


def _records_simplified(rings: np.ndarray, lines: np.ndarray, kept: np.ndarray, cls: np.ndarray, k: int, W: int, tolerance):
    """`_records` for simplified rings: the region and the TRUE area from the ring rows, offset, count and the box of the full
    ring from `simplify_device`'s line rows; a ring's first vertex stays first, so `first` is read from the kept vertices."""
    region, area, off = rings[:, 0], rings[:, 3], lines[:, 0]
    outer = np.nonzero(area > 0)[0]
    if len(outer) != k or not np.array_equal(np.sort(region[outer]), np.arange(k)):
        raise RuntimeError(f"region_polygons: {len(outer)} outer rings for {k} regions")
    rec = np.zeros((k, 7), np.int32)
    polygons = _simplify.Simplified([[] for _ in range(k)], tolerance, np.bincount(region, weights=lines[:, 2], minlength=k))
    if k == 0:
        return rec, polygons
    start = kept[off[outer]].astype(np.int64)
    r = region[outer]
    rec[r, 0] = cls[outer]
    rec[r, 1], rec[r, 2], rec[r, 3], rec[r, 4] = lines[outer, 4], lines[outer, 5], lines[outer, 6] - 1, lines[outer, 7] - 1
    np.add.at(rec[:, 5], region, area.astype(np.int32))
    rec[r, 6] = start[:, 0] * W + start[:, 1]
    for i in np.argsort(region, kind="stable"):
        polygons[int(region[i])].append(np.ascontiguousarray(kept[int(off[i]):int(off[i] + lines[i, 1])]))
    return rec, polygons


@torch.no_grad()
def region_polygons(mask, *, background: int = 0, connectivity: int = 4, return_labels: bool = False, device="cuda:0",
                    simplify=None):
    """Outlines of the regions of a class mask uint8 / long [n, H, W] or [H, W]: per image a pair (records, polygons) -- a list of
    pairs for a batch, the pair itself for a [H, W] mask.  `records` is `region_boxes`' int32 [k, 7] array; `polygons[i]` is the
    list of region i's rings, int32 [v, 2] arrays of (y, x) lattice corners: the outer ring first, then one ring per hole (walked
    the other way: `ring_area` is negative).  Rings are open -- the last vertex joins the first.
    `background`, `connectivity`, `return_labels`, `device`: as `region_boxes`, and validated the same way, before the library is
    asked for anything.  One call is enqueued; the only host wait is the read of the counts (an image with more than
    DEFAULT_MAX_RINGS rings or DEFAULT_MAX_VERTICES vertices makes one more call at the true sizes: the same bits).
    `simplify`: a tolerance in pixels (None: off, nothing else is launched).  Every ring is thinned on the device by
    `simplify.simplify_device` (Douglas-Peucker with the segment distance; include/vitseg_simplify.h) before anything but the
    counts, the ring rows and the kept vertices is copied back.  A ring keeps its first vertex first and at least three
    vertices; the records keep the true area, class, `first` and box of the full outline; `polygons` is a
    `simplify.Simplified` list, which also holds the tolerance and every region's full vertex count.  Rings are simplified one by one:
    neighbouring regions may gap or overlap by up to the tolerance, and a ring may come to touch itself; the outer ring keeps a
    positive and a hole a negative area (a ring that would turn over is returned as it is)."""
    m, single = _checked(mask, background, connectivity)
    if simplify is not None:
        _simplify.tol2_q8(simplify)
    n, H, W = (int(d) for d in m.shape)
    if H > MAX_SIDE or W > MAX_SIDE or H * W >= MAX_PIXELS or n > 65535:
        raise ValueError(f"region_polygons takes at most 65535 images of at most {MAX_SIDE} x {MAX_SIDE} and fewer than 2^29 "
                         f"pixels, got {n} x {H} x {W}")
    if not m.is_cuda:
        m = m.to(device)
    m = m.to(torch.uint8).contiguous()
    background = int(background)
    out = _launch(m, background, connectivity, DEFAULT_MAX_RINGS, DEFAULT_MAX_VERTICES, return_labels)
    cnt = out[0].cpu().numpy()
    regions_n, rings_n, verts_n = cnt[:n], cnt[n:2 * n], cnt[2 * n:].view(np.int64)
    if int(rings_n.max()) > DEFAULT_MAX_RINGS or int(verts_n.max()) > DEFAULT_MAX_VERTICES:
        out = _launch(m, background, connectivity, max(int(rings_n.max()), 1), max(int(verts_n.max()), 1), return_labels)
    _, rings, vertices, cls, labels = out
    if simplify is not None:
        thin = _simplify.simplify_device(vertices, rings, out[0][n:2 * n], _simplify.RING_COLS, simplify)
        _, lines, kept = _simplify.kept_to_host(*thin)
        rings = rings[:, :int(rings_n.max())].cpu().numpy()
        cls = cls[:, :int(rings_n.max())].cpu().numpy()
        res = [_records_simplified(rings[i, :int(rings_n[i])], lines[i, :int(rings_n[i])], kept[i], cls[i, :int(rings_n[i])],
                                   int(regions_n[i]), W, simplify) for i in range(n)]
        if single:
            res, labels = res[0], (labels[0] if labels is not None else None)
        return (res, labels) if return_labels else res
    rings = rings[:, :int(rings_n.max())].cpu().numpy()
    vertices = vertices[:, :int(verts_n.max())].cpu().numpy()
    cls = cls[:, :int(rings_n.max())].cpu().numpy()
    res = [_records(rings[i, :int(rings_n[i])], vertices[i, :int(verts_n[i])], cls[i, :int(rings_n[i])], int(regions_n[i]), W)
           for i in range(n)]
    if single:
        res, labels = res[0], (labels[0] if labels is not None else None)
    return (res, labels) if return_labels else res


def ring_area(ring) -> int:
    """The signed area of a ring of (y, x) vertices, the shoelace sum 1/2 sum (x_i y_{i+1} - x_{i+1} y_i): the pixels an outer
    ring encloses, minus the pixels of a hole."""
    v = np.asarray(ring, dtype=np.int64).reshape(-1, 2)
    y, x = v[:, 0], v[:, 1]
    return int(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)) // 2


def ring_length(ring) -> int:
    """The length of a ring of (y, x) vertices in pixel sides (the sum over a region's rings is `region_props`' perimeter)."""
    v = np.asarray(ring, dtype=np.int64).reshape(-1, 2)
    return int(np.abs(v - np.roll(v, -1, axis=0)).sum())


def polygons_to_geojson(records, polygons, *, pixel_size: float = 1.0, image_id=None,
                        class_names: Optional[Sequence[str]] = None) -> dict:
    """A GeoJSON FeatureCollection (a dict for json.dump) of one image's `region_polygons` pair: one Feature per region, its
    geometry a Polygon whose first ring is the outline and whose others are the holes, each closed by repeating its first
    point, coordinates [x * pixel_size, y * pixel_size] (x to the right, y down, the image's top left corner at the origin).
    Properties: class, first, area (pixels times pixel_size squared), holes, image_id and, with `class_names`, class_name.
    The polygons of `region_polygons(..., simplify=tol)` (a `simplify.Simplified` list) add simplify_tolerance and
    vertices_full, the number of vertices of the region's full outline, all its rings together; nothing else changes."""
    ps = _common.pixel_size(pixel_size)
    thinned = isinstance(polygons, _simplify.Simplified)
    rec = np.asarray(records).reshape(-1, 7)
    if len(rec) != len(polygons):
        raise ValueError(f"{len(rec)} records for {len(polygons)} polygons")
    features = []
    for r, (row, rings) in enumerate(zip(rec, polygons)):
        coords = []
        for ring in rings:
            v = np.asarray(ring).reshape(-1, 2)
            pts = [[float(x) * ps, float(y) * ps] for y, x in v.tolist()]
            coords.append(pts + [pts[0]])
        props = {"class": int(row[0]), "first": int(row[6]), "area": int(row[5]) * ps * ps, "holes": len(rings) - 1,
                 "image_id": image_id}
        if class_names is not None:
            props["class_name"] = str(class_names[int(row[0])])
        if thinned:
            props.update(simplify_tolerance=polygons.tolerance, vertices_full=int(polygons.full[r]))
        features.append({"type": "Feature", "geometry": {"type": "Polygon", "coordinates": coords}, "properties": props})
    return {"type": "FeatureCollection", "features": features}
