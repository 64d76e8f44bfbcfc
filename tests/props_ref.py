"""numpy restatement of vitseg_region_props (include/vitseg.h): one int64 row of 20 fields per connected region, composed
from regions_ref.region_boxes_ref (the regions, their order and the labels), skeleton_ref.skeleton_one / end_points /
inner_d2 (the skeleton and the distance field of each class plane) and plain loops over the labels.  `props_naive` is a
second form, per region from np.argwhere, to hold the first against.  Also the test masks.  A plain helper module, imported
like regions_ref.py."""
import numpy as np

import regions_ref as RR
import skeleton_ref as SK

NF = 20
FIELDS = ("class", "first", "area", "y_min", "x_min", "y_max", "x_max", "sum_y", "sum_x", "sum_yy", "sum_xx", "sum_xy",
          "perimeter", "frame_pixels", "max_d2", "skel_len", "end_points", "skel_max_d2", "skel_width_q16", "reserved")


def q16(d2):
    """llrint(sqrt((double) d2) * 65536.0) of an integer array, as int64."""
    return np.rint(np.sqrt(np.asarray(d2, np.float64)) * 65536.0).astype(np.int64)


def sides(m):
    """Per pixel, the number of its four sides whose neighbour lies outside the image or has another value."""
    m = np.asarray(m).astype(np.int32)
    p = np.full((m.shape[0] + 2, m.shape[1] + 2), -1, np.int32)
    p[1:-1, 1:-1] = m
    return sum((p[1 + dy:p.shape[0] - 1 + dy, 1 + dx:p.shape[1] - 1 + dx] != m).astype(np.int64)
               for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)))


def class_planes(m, classes):
    """{c: (skeleton 0 / 1, d2 int64)} of the planes {m == c}."""
    return {int(c): (SK.skeleton_one(m == c)[0], SK.inner_d2(m == c)) for c in classes}


def props_one(m, classes=(), background=0, connectivity=4):
    """(props int64 [k, 20], labels int32 [H, W]) of one class map."""
    m = np.asarray(m)
    H, W = m.shape
    rec, lab = RR.regions_one(m, background, connectivity)
    k = len(rec)
    out = np.zeros((k, NF), np.int64)
    out[:, 0], out[:, 1], out[:, 2] = rec[:, 0], rec[:, 6], rec[:, 5]
    out[:, 3:7] = rec[:, 1:5]
    planes = class_planes(m, classes)
    for c in planes:
        assert 0 <= c <= 255 and c != background
    measured = np.isin(out[:, 0], list(planes))
    out[~measured, 14:19] = -1
    out[measured, 17] = -1
    side = sides(m)
    for y in range(H):
        for x in range(W):
            r = lab[y, x]
            if r < 0:
                continue
            o = out[r]
            o[7] += y
            o[8] += x
            o[9] += y * y
            o[10] += x * x
            o[11] += x * y
            o[12] += side[y, x]
            o[13] += y in (0, H - 1) or x in (0, W - 1)
            if measured[r]:
                skel, d2 = planes[int(m[y, x])]
                o[14] = max(o[14], d2[y, x])
                if skel[y, x]:
                    o[15] += 1
                    o[17] = max(o[17], d2[y, x])
                    o[18] += q16(d2[y, x])
    for c, (skel, _) in planes.items():   # end points: skeleton pixels with exactly one set 8-neighbour in the plane's skeleton
        ends = (skel == 1) & (sum(SK.neighbours(skel)) == 1)
        for y, x in np.argwhere(ends):
            out[lab[y, x], 16] += 1
    return out, lab


def props_ref(mask, classes=(), background=0, connectivity=4, return_labels=False):
    """The restatement of visiontransformer_amd.regions.region_props on a [n, H, W] or [H, W] array."""
    m = np.asarray(mask)
    single = m.ndim == 2
    if single:
        m = m[None]
    res = [props_one(mi, classes, background, connectivity) for mi in m]
    out = [p for p, _ in res]
    labels = np.stack([l for _, l in res])
    if single:
        out, labels = out[0], labels[0]
    return (out, labels) if return_labels else out


def props_naive(m, classes=(), background=0, connectivity=4, records=RR.regions_one):
    """The same rows, region by region: np.argwhere of the region's label, then sums over its coordinates.  `records`: the
    labelling, (m, background, connectivity) -> (records, labels); regions_ref.scipy_records is scipy.ndimage.label's."""
    m = np.asarray(m)
    H, W = m.shape
    rec, lab = records(m, background, connectivity)
    planes = class_planes(m, classes)
    rows = []
    for r in range(len(rec)):
        yx = np.argwhere(lab == r).astype(np.int64)
        y, x = yx[:, 0], yx[:, 1]
        c = int(m[y[0], x[0]])
        per = 0
        for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            yy, xx = y + dy, x + dx
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            same = np.zeros(len(y), bool)
            same[inside] = m[yy[inside], xx[inside]] == c
            per += int((~same).sum())
        row = [c, int(y[0] * W + x[0]), len(y), y.min(), x.min(), y.max(), x.max(), y.sum(), x.sum(), (y * y).sum(),
               (x * x).sum(), (x * y).sum(), per, int(((y == 0) | (y == H - 1) | (x == 0) | (x == W - 1)).sum())]
        if c in planes:
            skel, d2 = planes[c]
            on = skel[y, x] == 1
            nb = sum(SK.neighbours(skel))[y, x]
            dd = d2[y, x]
            row += [dd.max(), int(on.sum()), int((on & (nb == 1)).sum()), dd[on].max() if on.any() else -1, q16(dd[on]).sum()]
        else:
            row += [-1] * 5
        rows.append(row + [0])
    return np.asarray(rows, np.int64).reshape(-1, NF)


# ---- test masks ----

def staircase(H, W, cls=1):
    """A diagonal of single pixels of one class: min(H, W) regions under connectivity 4, one under 8."""
    m = np.zeros((H, W), np.uint8)
    d = np.arange(min(H, W))
    m[d, d] = cls
    return m


def square2(H, W, cls=1):
    """An isolated 2 x 2 square of one class: its skeleton is empty."""
    m = np.zeros((H, W), np.uint8)
    m[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1] = cls
    return m


def mixed_batch(H=70, W=97):
    """Three images of 5 classes: blobs; a serpentine and a U over blobs; rings with a blob overlay."""
    a = RR.blobs(11, H, W, 5, radius=3)
    b = RR.blobs(12, H, W, 3, radius=4)
    b[RR.serpentine(H, W) == 1] = 3
    b[RR.u_shape(H, W) == 1] = 4
    c = RR.rings(H, W, 3)
    c[RR.blobs(13, H, W, 4, radius=3) == 3] = 4
    c[RR.blobs(14, H, W, 6, radius=3) == 0] = 3
    return np.stack([a, b, c]).astype(np.uint8)


def golden_cases():
    """name -> (uint8 mask, classes, background, connectivity): the cases of tests/golden/props/props.npz."""
    mb = mixed_batch(40, 53)
    return {
        "blobs5_c4": (mb[0], (1, 3), 0, 4),
        "paths_c8": (mb[1], (3, 4), 0, 8),
        "rings_c4_nobg": (mb[2], (0, 2, 4), -1, 4),
        "crack_33x65_c8": (SK.crack_map(33, 65, 5), (1, 2), 0, 8),
        "stairs_24_c4": (staircase(24, 24), (1,), 0, 4),
        "stairs_24_c8": (staircase(24, 24), (1,), 0, 8),
        "square2_16": (square2(16, 16), (1,), 0, 4),
        "full_9x40": (np.full((9, 40), 2, np.uint8), (2,), 0, 4),
        "blobs5_none": (mb[0], (), 0, 8),
    }
