"""numpy restatement of vitseg_regions (include/vitseg.h): connected regions of a class mask, their boxes, areas and first
pixels, in the order the reference's "Predicted Regions with Boxes" loop emits them (model/CE/testViTModel.py:34-42,
171-185: np.unique classes, then scipy.ndimage.label numbering, which follows the raster order of each component's
first pixel).  No scipy: union-find by minimum index with vectorised hooking and pointer jumping, so it runs where scipy
is not installed.  Also the test masks (blobs, checkerboard, serpentine, ...).  A plain helper module, imported like
dropout_ref.py."""
import numpy as np

FIELDS = ("class", "y_min", "x_min", "y_max", "x_max", "area", "first")


def _offsets(connectivity):
    if connectivity == 4:
        return [(0, -1), (-1, 0)]
    if connectivity == 8:
        return [(0, -1), (-1, 0), (-1, -1), (-1, 1)]
    raise ValueError(f"connectivity must be 4 or 8, got {connectivity}")


def _roots(m, background, connectivity):
    """parent[p] = minimum raster index of p's region (p itself for a root); -1 on background."""
    H, W = m.shape
    P = H * W
    flat = m.reshape(-1).astype(np.int32)
    valid = flat != background
    idx = np.arange(P, dtype=np.int64).reshape(H, W)
    a_list, b_list = [], []
    for dy, dx in _offsets(connectivity):   # neighbour (y + dy, x + dx) precedes (y, x) in raster order
        y0, y1 = max(0, -dy), H
        x0, x1 = max(0, -dx), min(W, W - dx)
        if y0 >= y1 or x0 >= x1:
            continue
        p = idx[y0:y1, x0:x1].reshape(-1)
        q = idx[y0 + dy:y1 + dy, x0 + dx:x1 + dx].reshape(-1)
        keep = valid[p] & (flat[p] == flat[q])
        a_list.append(q[keep])
        b_list.append(p[keep])
    lo_e = np.concatenate(a_list) if a_list else np.zeros(0, np.int64)
    hi_e = np.concatenate(b_list) if b_list else np.zeros(0, np.int64)
    parent = np.arange(P, dtype=np.int64)
    while True:
        ra, rb = parent[lo_e], parent[hi_e]
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        ch = lo != hi
        if not ch.any():
            break
        np.minimum.at(parent, hi[ch], lo[ch])   # hook roots onto the smaller root
        while True:                              # pointer jumping to full compression
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    parent[~valid] = -1
    return parent


def regions_one(m, background=0, connectivity=4):
    """(records int32 [k, 7] in (class, first) order, labels int32 [H, W]: region index, -1 on background)."""
    m = np.asarray(m)
    assert m.ndim == 2
    H, W = m.shape
    flat = m.reshape(-1).astype(np.int64)
    parent = _roots(m, background, connectivity)
    roots = np.nonzero(parent == np.arange(H * W))[0]
    cls = flat[roots]
    order = np.lexsort((roots, cls))
    roots, cls = roots[order], cls[order]
    k = roots.size
    index_of = np.full(H * W, -1, np.int64)
    index_of[roots] = np.arange(k)
    valid = parent >= 0
    lab = np.full(H * W, -1, np.int64)
    lab[valid] = index_of[parent[valid]]
    ys, xs = np.divmod(np.arange(H * W, dtype=np.int64), W)
    li, yv, xv = lab[valid], ys[valid], xs[valid]
    area = np.bincount(li, minlength=k)
    ymax = np.full(k, -1, np.int64)
    xmin = np.full(k, W, np.int64)
    xmax = np.full(k, -1, np.int64)
    np.maximum.at(ymax, li, yv)
    np.minimum.at(xmin, li, xv)
    np.maximum.at(xmax, li, xv)
    rec = np.stack([cls, roots // W, xmin, ymax, xmax, area, roots], axis=1).astype(np.int32).reshape(k, 7)
    return rec, lab.reshape(H, W).astype(np.int32)


def region_boxes_ref(mask, background=0, connectivity=4, return_labels=False):
    """The restatement of visiontransformer_amd.regions.region_boxes on a [n, H, W] or [H, W] array."""
    m = np.asarray(mask)
    single = m.ndim == 2
    if single:
        m = m[None]
    out = [regions_one(mi, background, connectivity) for mi in m]
    recs = [r for r, _ in out]
    if not return_labels:
        return recs
    labels = np.stack([l for _, l in out])
    return recs, (labels[0] if single else labels)


def boxes_by_class(records):
    """{class: [(y_min, x_min, y_max, x_max), ...]} -- what the reference's loop collects from get_bounding_boxes."""
    out = {}
    for r in np.asarray(records):
        out.setdefault(int(r[0]), []).append((int(r[1]), int(r[2]), int(r[3]), int(r[4])))
    return out


def scipy_records(m, background=0, connectivity=4):
    """The reference's own rule: scipy.ndimage.label per class present (ascending, background skipped) + np.argwhere per
    label (testViTModel.py:34-42), extended by area and first pixel; and the labels map (offset_c + k - 1).  Needs scipy."""
    from scipy import ndimage
    m = np.asarray(m)
    W = m.shape[1]
    structure = None if connectivity == 4 else np.ones((3, 3), dtype=bool)
    rows = []
    labels = np.full(m.shape, -1, np.int64)
    for c in np.unique(m):
        if int(c) == background:
            continue
        lab, nf = ndimage.label(m == c, structure=structure)
        off = len(rows)
        labels[lab > 0] = lab[lab > 0] - 1 + off
        for k in range(1, nf + 1):
            coords = np.argwhere(lab == k)
            y_min, x_min = coords.min(axis=0)
            y_max, x_max = coords.max(axis=0)
            first = int(coords[0, 0]) * W + int(coords[0, 1])   # argwhere is in raster order
            rows.append((int(c), int(y_min), int(x_min), int(y_max), int(x_max), len(coords), first))
    return np.asarray(rows, dtype=np.int32).reshape(-1, 7), labels.astype(np.int32)


# ---- test masks ----

def _box_blur(a, r, axis):
    c = np.cumsum(np.pad(a, [(r + 1, r) if ax == axis else (0, 0) for ax in range(a.ndim)], mode="wrap"), axis=axis)
    n = a.shape[axis]
    hi = np.take(c, np.arange(2 * r + 1, 2 * r + 1 + n), axis=axis)
    lo = np.take(c, np.arange(0, n), axis=axis)
    return hi - lo


def blobs(seed, H, W, C, n=None, radius=6):
    """A smoothed random field thresholded into C classes at its quantiles: uint8 [H, W] (or [n, H, W])."""
    rs = np.random.RandomState(seed)
    shape = (H, W) if n is None else (n, H, W)
    f = rs.standard_normal(shape)
    for _ in range(3):
        f = _box_blur(_box_blur(f, radius, f.ndim - 1), radius, f.ndim - 2)
    q = np.quantile(f, np.linspace(0, 1, C + 1)[1:-1])
    return np.searchsorted(q, f).astype(np.uint8)


def checkerboard(H, W):
    y, x = np.mgrid[:H, :W]
    return ((y + x) % 2).astype(np.uint8)


def serpentine(H, W, cls=1):
    """One-pixel-wide path of class `cls` through the whole image on class 0: every even row, joined at alternating
    ends through the odd rows (the longest chain a labelling can meet)."""
    m = np.zeros((H, W), np.uint8)
    m[0::2] = cls
    for y in range(1, H, 2):
        m[y, W - 1 if (y // 2) % 2 == 0 else 0] = cls
    return m


def u_shape(H, W):
    """Two arms of class 1 that meet only in the last row."""
    m = np.zeros((H, W), np.uint8)
    m[:, 2] = 1
    m[:, W - 3] = 1
    m[H - 1, 2:W - 2] = 1
    return m


def rings(H, W, k=3):
    y, x = np.mgrid[:H, :W]
    r = np.sqrt((y - H / 2.0 + 0.5) ** 2 + (x - W / 2.0 + 0.5) ** 2)
    return ((r // 4).astype(np.int64) % k).astype(np.uint8)


def all_values(seed, H, W):
    rs = np.random.RandomState(seed)
    return (rs.permutation(H * W) % 256).astype(np.uint8).reshape(H, W)


def golden_cases():
    """name -> uint8 mask: the cases of tests/golden/regions/regions.npz."""
    rs = np.random.RandomState(7)
    return {
        "blobs2_224": blobs(1, 224, 224, 2),
        "blobs17_224": blobs(2, 224, 224, 17),
        "checker_64": checkerboard(64, 64),
        "serpentine_96": serpentine(96, 96),
        "u_70x45": u_shape(70, 45),
        "rings_96": rings(96, 96),
        "strip_1x300": rs.randint(0, 3, size=(1, 300)).astype(np.uint8),
        "strip_257x1": rs.randint(0, 3, size=(257, 1)).astype(np.uint8),
        "blobs5_333x500": blobs(3, 333, 500, 5, radius=4),
        "all256_48": all_values(4, 48, 48),
    }


GOLDEN_VARIANTS = [(4, 0), (4, -1), (8, 0), (8, -1)]   # (connectivity, background)
