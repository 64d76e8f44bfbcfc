"""Crack centre-lines as a graph on the device: the pixel graph of a skeleton traced into nodes (end points, junctions,
isolated pixels), branches and ordered polylines, and their GeoJSON -- the line counterpart of `polygons.region_polygons`.

The contract is stated in include/vitseg_centerlines.h: two skeleton pixels are linked when they are 4-neighbours, or diagonal
neighbours with neither pixel between them set; nodes are the pixels whose number of links is not 2; a branch is the walk from
one node to the next, reported once, from its smaller end; a curve without a node is a closed branch that starts at its
smallest pixel.  One call of `vitseg_centerlines` (csrc/centerlines.hip) thins a whole batch with `vitseg_skeleton`'s kernels,
measures it with the exact distance field and traces it; everything it returns is an integer.  The usual host answer is skan
or a hand-written walk over the skeleton, one image at a time.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _common, _ext, _lib
from . import simplify as _simplify
from .skeleton import MAX_BATCH, MAX_SIDE, ROUTES

MAX_PIXELS = 1 << 29
NODE_FIELDS = ("y", "x", "degree", "d2")
BRANCH_FIELDS = ("start", "end", "offset", "points", "kind", "orthogonal", "diagonal", "width_q16", "max_d2")


def _symbol(name: str):
    return _ext.ext_symbol("centerlines", name)


def check_options(classes, thin=True, route: str = "auto"):
    """Validates what does not depend on the mask; returns the class values as a list of ints, or None."""
    if not isinstance(thin, (bool, np.bool_)):
        raise ValueError(f"thin must be True or False, got {thin!r}")
    if route not in ROUTES:
        raise ValueError(f"route must be one of {sorted(ROUTES)}, got {route!r}")
    if classes is None:
        return None
    if isinstance(classes, (str, bytes)):
        raise ValueError(f"classes must be None or a sequence of label values, got {classes!r}")
    return _common.label_values("classes", classes)


def _checked(mask, classes, thin, route):
    """Validates the arguments before anything reaches the library: (mask [n, H, W], whether it was 2-D, the class values or
    None)."""
    if isinstance(mask, np.ndarray):
        mask = torch.from_numpy(np.ascontiguousarray(mask))
    if not isinstance(mask, torch.Tensor):
        raise ValueError(f"mask must be a torch.Tensor or numpy array, got {type(mask).__name__}")
    if mask.dtype not in (torch.uint8, torch.bool, torch.int64):
        raise ValueError(f"mask must be uint8, bool or int64 (long), got {mask.dtype}")
    if mask.dim() not in (2, 3):
        raise ValueError(f"mask must be [n, H, W] or [H, W], got shape {tuple(mask.shape)}")
    if mask.numel() == 0:
        raise ValueError(f"mask must not be empty, got shape {tuple(mask.shape)}")
    classes = check_options(classes, thin, route)
    single = mask.dim() == 2
    if single:
        mask = mask[None]
    n, H, W = (int(d) for d in mask.shape)
    if H > MAX_SIDE or W > MAX_SIDE or H * W >= MAX_PIXELS or n > MAX_BATCH:
        raise ValueError(f"trace takes at most {MAX_BATCH} images of at most {MAX_SIDE} x {MAX_SIDE} and fewer than 2^29 pixels, "
                         f"got {n} x {H} x {W}")
    if mask.dtype == torch.int64:
        lo, hi = int(mask.min()), int(mask.max())
        if lo < 0 or hi > 255:
            raise ValueError(f"mask values must lie in 0..255, got {lo}..{hi}")
    return mask, single, classes


def _launch(m: torch.Tensor, value: int, thin: bool, route: int, max_nodes: int, max_branches: int, max_points: int):
    """Enqueues one vitseg_centerlines call on the current stream for a contiguous device uint8 [n, H, W] mask: (counts int32
    [4 n]: the node counts, the branch counts and, as int64, the point counts; nodes; branches; points)."""
    n, H, W = (int(d) for d in m.shape)
    dev = m.device
    with torch.cuda.device(dev):
        nbytes = _symbol("vitseg_centerlines_scratch_bytes")(n, H, W, route)
        if nbytes == 0:
            raise ValueError(f"trace: a {H} x {W} plane does not fit the resident route of the skeleton (or the shape "
                             f"{n} x {H} x {W} is out of range)")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        counts = torch.empty(4 * n, dtype=torch.int32, device=dev)
        nodes = torch.empty((n, max_nodes, 4), dtype=torch.int32, device=dev)
        branches = torch.empty((n, max_branches, 9), dtype=torch.int64, device=dev)
        points = torch.empty((n, max_points, 3), dtype=torch.int32, device=dev)
        _lib.check(_symbol("vitseg_centerlines")(
            m.data_ptr(), n, H, W, value, int(thin), route, counts.data_ptr(), counts[n:].data_ptr(), counts[2 * n:].data_ptr(),
            nodes.data_ptr() if max_nodes > 0 else None, max_nodes, branches.data_ptr() if max_branches > 0 else None,
            max_branches, points.data_ptr() if max_points > 0 else None, max_points, scratch.data_ptr(), nbytes,
            torch.cuda.current_stream(dev).cuda_stream))
    return counts, nodes, branches, points


def _trace_value(m: torch.Tensor, value: int, thin: bool, route: int, simplify=None):
    """One plane selection of a batch: a count query, then the call at the true sizes; [(nodes, branches, points)] per image.
    With `simplify` the points are thinned on the device and only the kept ones are copied back."""
    n = int(m.shape[0])
    cnt = _launch(m, value, thin, route, 0, 0, 0)[0].cpu().numpy()
    nodes_n, branches_n, points_n = cnt[:n], cnt[n:2 * n], cnt[2 * n:].view(np.int64)
    counts, nodes, branches, points = _launch(m, value, thin, route, int(nodes_n.max()), int(branches_n.max()),
                                              int(points_n.max()))
    if simplify is not None:
        thinned = _simplify.simplify_device(points, branches, counts[n:2 * n], _simplify.BRANCH_COLS, simplify)
        kept_n, lines, points = _simplify.kept_to_host(*thinned)
        nodes, branches = nodes.cpu().numpy(), branches.cpu().numpy()
        full = branches[:, :, 3].copy()
        branches[:, :, 2:4] = lines[:, :, 0:2]   # offset and count alone change: lengths and widths stay the full branch's
        points_n = kept_n
    else:
        nodes, branches, points = nodes.cpu().numpy(), branches.cpu().numpy(), points.cpu().numpy()
    out = []
    for i in range(n):
        b = branches[i, :int(branches_n[i])]
        pts = points[i, :int(points_n[i])]
        lists = [np.ascontiguousarray(pts[int(o):int(o + c)]) for o, c in zip(b[:, 2], b[:, 3])]
        if simplify is not None:
            lists = _simplify.Simplified(lists, simplify, full[i, :int(branches_n[i])])
        out.append((nodes[i, :int(nodes_n[i])].copy(), b.copy(), lists))
    return out


@torch.no_grad()
def trace(mask, classes=None, thin: bool = True, route: str = "auto", device=None, simplify=None):
    """The centre-line graph of a mask uint8 / bool / long [n, H, W] or [H, W], numpy or torch.
    classes=None reads the mask as binary (non-zero = set) and returns, per image, a triple (nodes, branches, points); with a
    sequence of label values (0..255, distinct) it returns, per image, a dict class -> triple, each class traced on its own plane
    {mask == class}.  A [H, W] mask gives the triple or the dict itself, a batch a list of them.
      nodes     int32 [k, 4]: (y, x, degree, d2) in raster order; degree 0 an isolated pixel, 1 an end point, 3 or 4 a junction;
      branches  int64 [b, 9]: BRANCH_FIELDS -- start and end raster index, offset and count of its points, kind (0 open,
                1 closed), orthogonal and diagonal links walked, the q16 sum of its points' distances to the edge, their
                largest d2;
      points    a list of b int32 [v, 3] arrays of (y, x, d2) in walking order.
    thin=True traces `skeleton.skeletonize`'s skeleton of the plane (`route` as there; "global", and "auto" above 1024 x 1024,
    synchronise the stream); thin=False takes the plane as a centre-line set as it is.  d2 is the exact squared distance to the
    nearest pixel outside the plane's set.  Each plane selection makes a count query and one call at the true sizes; the
    counts are the only host read.  A CUDA tensor stays on its device, anything else goes to `device` (default cuda:0).
    `simplify`: a tolerance in pixels (None: off, nothing else is launched).  Every branch's polyline is thinned on the device
    by `simplify.simplify_device` (Douglas-Peucker with the segment distance; include/vitseg_simplify.h) and only the kept
    points are copied back.  Both ends of a branch are kept, so branches still meet at their node pixels; a closed branch
    keeps its start and at least three points.  The rows of `branches` change in offset and count alone -- links, width sum
    and max_d2 stay the full branch's -- and `points` is a `simplify.Simplified` list that also holds the tolerance and
    every branch's full point count, which `branch_table` and `centerlines_to_geojson` read.
    Raises ValueError, before the library is asked for anything, for a bad mask, `classes`, `thin`, `route` or `simplify`."""
    m, single, classes = _checked(mask, classes, thin, route)
    if simplify is not None:
        _simplify.tol2_q8(simplify)
    if not m.is_cuda:
        m = m.to(device or "cuda:0")
    m = m.to(torch.uint8).contiguous()
    n = int(m.shape[0])
    if classes is None:
        res = _trace_value(m, -1, bool(thin), ROUTES[route], simplify)
    else:
        per_class = {c: _trace_value(m, c, bool(thin), ROUTES[route], simplify) for c in classes}
        res = [{c: per_class[c][i] for c in classes} for i in range(n)]
    return res[0] if single else res


def _rows(branches) -> np.ndarray:
    rec = np.asarray(branches)
    if rec.ndim != 2 or rec.shape[1] != len(BRANCH_FIELDS):
        raise ValueError(f"branches must be [b, {len(BRANCH_FIELDS)}], got {rec.shape}")
    return rec


def branch_table(branches, pixel_size: float = 1.0, points=None) -> List[dict]:
    """One dict per row of one image's `branches` (int64 [b, 9]): host arithmetic on the integers.  Lengths are multiplied by
    `pixel_size`:
      length                  (orthogonal + diagonal * sqrt(2)) links: a diagonal step counts sqrt(2), not one pixel;
      chord, tortuosity       the distance between the first and the last point and length / chord (inf for a loop) -- from
                              `points`, the list `trace` returns with the rows; nan without it; a closed branch has chord 0;
      width_mean, width_max   2 (width_q16 / 65536) / points - 1 and 2 sqrt(max_d2) - 1, the width convention of
                              regions.props_from_records;
      closed, start, end, points   kind == 1, the raster indices of the two ends, the number of points.
    With the `points` of `trace(..., simplify=tol)` the mean width divides by the branch's full point count, the chord is that
    of the kept ends (the same two points) and `points` is the kept count."""
    rec = _rows(branches)
    full = points.full if isinstance(points, _simplify.Simplified) else None
    ps = _common.pixel_size(pixel_size)
    if points is not None and len(points) != len(rec):
        raise ValueError(f"{len(rec)} branches for {len(points)} point lists")
    nan = float("nan")
    out = []
    for i, row in enumerate(rec):
        start, end, _, count, kind, orth, diag, q16, max_d2 = (int(v) for v in row)
        length = orth + diag * math.sqrt(2.0)
        chord = nan
        if kind == 1:
            chord = 0.0
        elif points is not None:
            p = np.asarray(points[i]).reshape(-1, 3)
            chord = math.hypot(int(p[-1, 0]) - int(p[0, 0]), int(p[-1, 1]) - int(p[0, 1]))
        out.append({
            "start": start, "end": end, "closed": kind == 1, "points": count, "length": length * ps, "chord": chord * ps,
            "tortuosity": nan if math.isnan(chord) else (length / chord if chord > 0 else float("inf")),
            "width_mean": (2 * (q16 / 65536) / (count if full is None else full[i]) - 1) * ps, "width_max": (2 * math.sqrt(max_d2) - 1) * ps,
        })
    return out


def summary(nodes, branches, pixel_size: float = 1.0) -> dict:
    """One image's graph in five numbers: end_points (degree 1), junctions (degree 3 or 4), isolated (degree 0), branches and
    total_length (every link once, diagonal links as sqrt(2), times `pixel_size`)."""
    nd = np.asarray(nodes)
    if nd.ndim != 2 or nd.shape[1] != len(NODE_FIELDS):
        raise ValueError(f"nodes must be [k, {len(NODE_FIELDS)}], got {nd.shape}")
    rec = _rows(branches)
    ps = _common.pixel_size(pixel_size)
    deg = nd[:, 2]
    return {"end_points": int((deg == 1).sum()), "junctions": int((deg >= 3).sum()), "isolated": int((deg == 0).sum()),
            "branches": len(rec), "total_length": (int(rec[:, 5].sum()) + int(rec[:, 6].sum()) * math.sqrt(2.0)) * ps}


def _without_collinear(p: np.ndarray) -> np.ndarray:
    """The interior points at which the walk does not turn, dropped."""
    if len(p) < 3:
        return p
    step = np.diff(p[:, :2].astype(np.int64), axis=0)
    keep = np.ones(len(p), bool)
    keep[1:-1] = np.any(step[1:] != step[:-1], axis=1)
    return p[keep]


def centerlines_to_geojson(branches, points, *, pixel_size: float = 1.0, image_id=None, class_id=None,
                           class_names: Optional[Sequence[str]] = None, drop_collinear: bool = True) -> dict:
    """A GeoJSON FeatureCollection (a dict for json.dump) of one image's `trace` rows: one Feature per branch, its geometry a
    LineString through the branch's pixel centres, coordinates [(x + 0.5) * pixel_size, (y + 0.5) * pixel_size] -- the corner
    lattice of `polygons.polygons_to_geojson`, so lines and outlines overlay.  A closed branch repeats its first coordinate at
    the end; an open branch of one link has two coordinates.  `drop_collinear` leaves out the points at which the line does not
    turn (the properties are those of the full branch).  Properties: class (`class_id`), start, end (raster indices), closed,
    length, width_mean, width_max (`branch_table`, in units of pixel_size), points, image_id and, with `class_names` and a
    `class_id`, class_name.  The `points` of `trace(..., simplify=tol)` (a `simplify.Simplified` list) add simplify_tolerance
    and vertices_full, the branch's full point count; nothing else changes."""
    table = branch_table(branches, pixel_size, points)
    thinned = isinstance(points, _simplify.Simplified)
    ps = _common.pixel_size(pixel_size)
    features = []
    for i, (d, pts) in enumerate(zip(table, points)):
        p = np.asarray(pts).reshape(-1, 3)
        if d["closed"]:
            p = np.concatenate([p, p[:1]])
        if drop_collinear:
            p = _without_collinear(p)
        coords = [[(float(x) + 0.5) * ps, (float(y) + 0.5) * ps] for y, x, _ in p.tolist()]
        props = {"class": None if class_id is None else int(class_id), "start": d["start"], "end": d["end"], "closed": d["closed"],
                 "length": d["length"], "width_mean": d["width_mean"], "width_max": d["width_max"], "points": d["points"],
                 "image_id": image_id}
        if class_names is not None and class_id is not None:
            props["class_name"] = str(class_names[int(class_id)])
        if thinned:
            props.update(simplify_tolerance=points.tolerance, vertices_full=points.full[i])
        features.append({"type": "Feature", "geometry": {"type": "LineString", "coordinates": coords}, "properties": props})
    return {"type": "FeatureCollection", "features": features}


# header of <model>_crack_branches.csv (--crack-graph of the evaluation scripts): one row per branch, then one summary row per
# image and class (Branch "summary", the branch columns empty)
CSV_COLUMNS = ["Model_ID", "Model_Name", "Batch_Num", "Image_Idx", "Class", "Branch", "Start", "End", "Closed", "Points", "Length",
               "Chord", "Tortuosity", "Width_Mean", "Width_Max", "End_Points", "Junctions", "Isolated", "Branches", "Total_Length"]


def csv_rows(model_info, batch_num, image_idx, class_id, table, summ) -> List[list]:
    """The rows of <model>_crack_branches.csv for one image and class from `branch_table`'s dicts and `summary`'s dict."""
    head = [model_info[0], model_info[1], batch_num, image_idx, class_id]
    rows = [head + [i, d["start"], d["end"], int(d["closed"]), d["points"], d["length"], d["chord"], d["tortuosity"],
                    d["width_mean"], d["width_max"], "", "", "", "", ""] for i, d in enumerate(table)]
    rows.append(head + ["summary"] + [""] * 9 + [summ["end_points"], summ["junctions"], summ["isolated"], summ["branches"],
                                                summ["total_length"]])
    return rows


__all__ = ["trace", "branch_table", "summary", "centerlines_to_geojson", "NODE_FIELDS", "BRANCH_FIELDS"]
