"""numpy restatement of vitseg_sdf (include/vitseg.h): exact squared Euclidean distances of a binary mask and of its
complement, and the float steps of the reference's compute_sdf (model/PAED/segmentation.py:6-34: scipy's
distance_transform_edt of ~mask and of mask, each divided by its maximum).  No scipy: a vectorised down / up scan per
column, then a brute-force minimum over the columns of each row, so it runs where scipy is not installed.  Also the test
masks (empty, full, single pixels and holes, thin lines, sparse points, blobs, checkerboard, strips, cracks).  A plain
helper module, imported like regions_ref.py."""
import numpy as np


def column_pass(features):
    """int64 [H, W]: distance from each pixel to the nearest feature pixel in its column, INF = H + W when the column has
    none."""
    f = np.asarray(features, dtype=bool)
    H, W = f.shape
    INF = H + W
    y = np.arange(H, dtype=np.int64)[:, None]
    last = np.maximum.accumulate(np.where(f, y, -INF), axis=0)                # last feature row at or above
    nxt = np.minimum.accumulate(np.where(f, y, H + INF)[::-1], axis=0)[::-1]   # next feature row at or below
    return np.minimum(np.minimum(y - last, nxt - y), INF)


def virtual_d2(H, W):
    """scipy's distance_transform_edt of an input without any zero, squared: the distance to the virtual feature (-1, 0)."""
    y, x = np.mgrid[:H, :W].astype(np.int64)
    return (y + 1) ** 2 + x ** 2


def edt2(features):
    """int64 [H, W]: exact squared distance of every pixel to the nearest True pixel of `features` (0 on them); with no
    True pixel, scipy's virtual feature at (-1, 0)."""
    f = np.asarray(features, dtype=bool)
    H, W = f.shape
    if not f.any():
        return virtual_d2(H, W)
    if W == 1:
        return column_pass(f) ** 2
    if H == 1:
        return column_pass(f.T).T ** 2
    g = column_pass(f)
    g2 = np.where(g < H + W, g * g, np.int64(1) << 40)   # a column without a feature pixel never wins
    dx2 = (np.arange(W, dtype=np.int64)[:, None] - np.arange(W, dtype=np.int64)[None, :]) ** 2   # [x, x']
    out = np.empty((H, W), np.int64)
    for r in range(H):
        out[r] = (dx2 + g2[r][None, :]).min(axis=1)
    return out


def dist(d2):
    """scipy's distance: the root taken in float64, then cast to float32."""
    return np.sqrt(np.asarray(d2, dtype=np.float64)).astype(np.float32)


def normalized(d2):
    """compute_sdf's normalisation of one field: float32 distance / float32 maximum, all zero when the maximum is 0."""
    d = dist(d2)
    mx = dist(np.max(d2))
    return d / mx if mx > 0 else np.zeros_like(d)


def sdf_one(mask, normalize=True):
    """(sdf_ext, sdf_int) float32 [H, W] of one mask (non-zero = mask pixel)."""
    m = np.asarray(mask) != 0
    e2, i2 = edt2(m), edt2(~m)
    if normalize:
        return normalized(e2), normalized(i2)
    return dist(e2), dist(i2)


def sdf_ref(masks, normalize=True):
    """The restatement of vitseg_sdf / sdf.compute_sdf on a [n, H, W] or [H, W] array: (sdf_ext, sdf_int) float32."""
    m = np.asarray(masks)
    single = m.ndim == 2
    if single:
        m = m[None]
    out = [sdf_one(mi, normalize) for mi in m]
    e, i = np.stack([a for a, _ in out]), np.stack([b for _, b in out])
    return (e[0], i[0]) if single else (e, i)


def scipy_d2(a):
    """scipy's distance_transform_edt(a) squared, as exact integers (d2 = round(dist^2)): the distance of each non-zero
    pixel of `a` to the nearest zero pixel.  Needs scipy."""
    from scipy.ndimage import distance_transform_edt
    d = distance_transform_edt(np.asarray(a, dtype=bool))
    return np.rint(d * d).astype(np.int64)


def scipy_compute_sdf(mask):
    """compute_sdf's few lines restated with scipy: the normalised float32 pair.  Needs scipy."""
    from scipy.ndimage import distance_transform_edt
    m = np.asarray(mask).astype(bool)
    e = distance_transform_edt(~m).astype(np.float32)
    i = distance_transform_edt(m).astype(np.float32)
    if e.max() > 0:
        e /= e.max()
    if i.max() > 0:
        i /= i.max()
    return e, i


# ---- test masks (uint8, 0 / 1) ----

def _box_blur(a, r, axis):
    c = np.cumsum(np.pad(a, [(r + 1, r) if ax == axis else (0, 0) for ax in range(a.ndim)], mode="wrap"), axis=axis)
    n = a.shape[axis]
    return np.take(c, np.arange(2 * r + 1, 2 * r + 1 + n), axis=axis) - np.take(c, np.arange(0, n), axis=axis)


def blobs(seed, H, W, density=0.3, radius=4):
    """A smoothed random field thresholded at its (1 - density) quantile."""
    f = np.random.RandomState(seed).standard_normal((H, W))
    for _ in range(2):
        f = _box_blur(_box_blur(f, radius, 1), radius, 0)
    return (f > np.quantile(f, 1 - density)).astype(np.uint8)


def checkerboard(H, W):
    y, x = np.mgrid[:H, :W]
    return ((y + x) % 2).astype(np.uint8)


def sparse_points(seed, H, W, k=5):
    m = np.zeros((H, W), np.uint8)
    rs = np.random.RandomState(seed)
    m[rs.randint(0, H, k), rs.randint(0, W, k)] = 1
    return m


def cracks(seed, H, W, k=3):
    """Thin random polylines: k random walks of one-pixel width that turn slowly, like cracks in a concrete image."""
    rs = np.random.RandomState(seed)
    m = np.zeros((H, W), np.uint8)
    for _ in range(k):
        n = 2 * max(H, W)
        a = rs.uniform(0, 2 * np.pi) + np.cumsum(rs.normal(0, 0.15, n))
        y = rs.uniform(0, H) + np.cumsum(np.sin(a))
        x = rs.uniform(0, W) + np.cumsum(np.cos(a))
        out = (y < 0) | (y >= H) | (x < 0) | (x >= W)
        stop = int(np.argmax(out)) if out.any() else n
        m[y[:stop].astype(np.int64), x[:stop].astype(np.int64)] = 1
    return m


def thin_lines(H, W):
    m = np.zeros((H, W), np.uint8)
    m[H // 3, :] = 1
    m[:, (2 * W) // 3] = 1
    d = np.arange(min(H, W))
    m[d, d] = 1
    return m


def single(H, W, y, x, hole=False):
    m = np.zeros((H, W), np.uint8)
    m[y, x] = 1
    return 1 - m if hole else m


def corners(H, W, hole=False):
    m = np.zeros((H, W), np.uint8)
    m[0, 0] = m[0, W - 1] = m[H - 1, 0] = m[H - 1, W - 1] = 1
    return 1 - m if hole else m


def random_mask(rs, H, W, density):
    return (rs.rand(H, W) < density).astype(np.uint8)


KINDS = ("empty", "cracks", "blobs", "checker", "points", "full", "lines", "sparse")


def kind_mask(kind, seed, H, W):
    if kind == "empty":
        return np.zeros((H, W), np.uint8)
    if kind == "full":
        return np.ones((H, W), np.uint8)
    if kind == "cracks":
        return cracks(seed, H, W)
    if kind == "blobs":
        return blobs(seed, H, W)
    if kind == "checker":
        return checkerboard(H, W)
    if kind == "points":
        return sparse_points(seed, H, W)
    if kind == "lines":
        return thin_lines(H, W)
    if kind == "sparse":
        return random_mask(np.random.RandomState(seed), H, W, 0.02)
    raise ValueError(kind)


def mixed_batch(seed, n, H, W):
    """n masks of every kind in turn; every other one holds 0 / 255 like a decoded 'L' mask, the rest 0 / 1."""
    out = np.stack([kind_mask(KINDS[i % len(KINDS)], seed + i, H, W) for i in range(n)])
    out[1::2] *= 255
    return out


def golden_cases():
    """name -> uint8 mask: the cases of tests/golden/sdf/sdf.npz."""
    rs = np.random.RandomState(9)
    cases = {
        "empty_1x1": np.zeros((1, 1), np.uint8),
        "full_1x1": np.ones((1, 1), np.uint8),
        "empty_1x5": np.zeros((1, 5), np.uint8),
        "empty_5x1": np.zeros((5, 1), np.uint8),
        "full_7x3": np.ones((7, 3), np.uint8),
        "empty_7x3": np.zeros((7, 3), np.uint8),
        "empty_224": np.zeros((224, 224), np.uint8),
        "full_224": np.ones((224, 224), np.uint8),
        "single_31x17": single(31, 17, 12, 5),
        "hole_31x17": single(31, 17, 12, 5, hole=True),
        "corners_40x23": corners(40, 23),
        "corner_holes_40x23": corners(40, 23, hole=True),
        "corner_tl_33x45": single(33, 45, 0, 0),
        "corner_br_33x45": single(33, 45, 32, 44),
        "lines_96x64": thin_lines(96, 64),
        "points_224": sparse_points(3, 224, 224, k=7),
        "blobs_224": blobs(4, 224, 224),
        "blobs_97x151": blobs(5, 97, 151, density=0.5, radius=3),
        "checker_64x37": checkerboard(64, 37),
        "cracks_224": cracks(6, 224, 224),
        "cracks_150x200": cracks(7, 150, 200, k=2),
        "strip_1x300": random_mask(rs, 1, 300, 0.05),
        "strip_257x1": random_mask(rs, 257, 1, 0.05),
        "strip_empty_1x300": np.zeros((1, 300), np.uint8),
        "random_61x89": random_mask(rs, 61, 89, 0.02),
        "dense_53x29": random_mask(rs, 53, 29, 0.9),
    }
    cases["values_45x45"] = (random_mask(rs, 45, 45, 0.1) * rs.randint(1, 256, size=(45, 45))).astype(np.uint8)
    return cases


# cases whose normalised pair the goldens also hold, straight from compute_sdf's lines run with scipy
NORMALIZED_CASES = ("empty_7x3", "full_7x3", "empty_224", "single_31x17", "hole_31x17", "blobs_97x151", "cracks_150x200",
                    "strip_1x300", "values_45x45")
