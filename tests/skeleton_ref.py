"""numpy restatement of vitseg_skeleton and vitseg_skeleton_stats (include/vitseg.h): Zhang-Suen thinning as published
(T. Y. Zhang and C. Y. Suen, "A Fast Parallel Algorithm for Thinning Digital Patterns", CACM 1984), written per pixel from
the paper's rules on 0 / 1 arrays -- no bit packing, no words, so it shares no trick with the kernel -- and the crack
statistics on the skeletons, with scipy's distance_transform_edt for the widths.  Also the test masks.  A plain helper
module, imported like sdf_ref.py."""
import numpy as np

# offsets (dy, dx) of P2 .. P9: clockwise from north
NEIGHBOURS = [(-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1)]


def neighbours(m):
    """The eight neighbour arrays P2 .. P9 of a 0 / 1 array; pixels outside the image are background."""
    H, W = m.shape
    p = np.zeros((H + 2, W + 2), np.int32)
    p[1:-1, 1:-1] = m
    return [p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy, dx in NEIGHBOURS]


def sub_iteration(m, sub):
    """One sub-iteration (0 or 1) decided for all pixels from `m`: the array after deletion and whether anything was deleted."""
    P2, P3, P4, P5, P6, P7, P8, P9 = n = neighbours(m)
    B = sum(n)
    A = sum((n[i] == 0) & (n[(i + 1) % 8] == 1) for i in range(8))
    if sub == 0:
        cond = (P2 * P4 * P6 == 0) & (P4 * P6 * P8 == 0)
    else:
        cond = (P2 * P4 * P8 == 0) & (P2 * P6 * P8 == 0)
    delete = (m == 1) & (B >= 2) & (B <= 6) & (A == 1) & cond
    return np.where(delete, 0, m).astype(np.uint8), bool(delete.any())


def skeleton_one(mask):
    """(skeleton uint8 0 / 1, passes) of one mask (non-zero = set); the pass that deleted nothing is counted."""
    m = (np.asarray(mask) != 0).astype(np.uint8)
    passes = 0
    while True:
        m, d1 = sub_iteration(m, 0)
        m, d2 = sub_iteration(m, 1)
        passes += 1
        if not (d1 or d2):
            return m, passes


def skeleton_ref(masks):
    """(skeleton uint8 [n, H, W], passes int32 [n]) of a batch."""
    out = [skeleton_one(m) for m in np.asarray(masks)]
    return np.stack([s for s, _ in out]), np.array([p for _, p in out], np.int32)


def end_points(skel):
    """Skeleton pixels with exactly one set 8-neighbour."""
    return int(((skel == 1) & (sum(neighbours(skel)) == 1)).sum())


def inner_d2(X):
    """Exact squared distance of each pixel of X to the nearest pixel outside X (scipy's distance_transform_edt, squared and
    rounded; its virtual point when X is the whole image), 0 outside X."""
    from scipy.ndimage import distance_transform_edt
    d = distance_transform_edt(np.asarray(X, dtype=bool))
    return np.rint(d * d).astype(np.int64)


def stats_ref(gt, pred, classes):
    """(stats_i int64 [n, K, 10], stats_f float64 [n, K, 2]) of vitseg_skeleton_stats."""
    gt, pred = np.asarray(gt), np.asarray(pred)
    n, K = gt.shape[0], len(classes)
    si, sf = np.zeros((n, K, 10), np.int64), np.zeros((n, K, 2), np.float64)
    for i in range(n):
        for k, c in enumerate(classes):
            G, P = gt[i] == c, pred[i] == c
            for side, (X, O) in enumerate([(G, P), (P, G)]):
                S = skeleton_one(X)[0] == 1
                d2 = inner_d2(X)[S]
                si[i, k, 0 + side] = X.sum()
                si[i, k, 2 + side] = S.sum()
                si[i, k, 4 + side] = (S & O).sum()
                si[i, k, 6 + side] = d2.max() if S.any() else -1
                si[i, k, 8 + side] = end_points(S.astype(np.uint8))
                sf[i, k, side] = np.sqrt(d2.astype(np.float64)).sum()
    return si, sf


def components(m):
    """Number of 8-connected components."""
    from scipy.ndimage import label
    return int(label(np.asarray(m) != 0, structure=np.ones((3, 3), int))[1])


def labelled(m):
    """(labels, count) of the 8-connected components."""
    from scipy.ndimage import label
    return label(np.asarray(m) != 0, structure=np.ones((3, 3), int))


# ---- test masks (uint8 0 / 1) ----

def crack(H, W, seed, half=1):
    """A random walk from the left edge to the right, widened to a band of 2 half + 1 pixels."""
    rs = np.random.RandomState(seed)
    m = np.zeros((H, W), np.uint8)
    y = rs.uniform(0.25 * H, 0.75 * H)
    for x in range(W):
        y = min(max(y + rs.normal(0, 0.7), 0), H - 1)
        m[max(int(y) - half, 0):int(y) + half + 1, max(x - half, 0):x + half + 1] = 1
    return m


def blobs(H, W, seed):
    """Gaussian-filtered noise thresholded at its 70 % quantile."""
    from scipy.ndimage import gaussian_filter
    f = gaussian_filter(np.random.RandomState(seed).standard_normal((H, W)), 3.0, mode="constant")
    return (f > np.quantile(f, 0.7)).astype(np.uint8)


def full(H, W):
    return np.ones((H, W), np.uint8)


def empty(H, W):
    return np.zeros((H, W), np.uint8)


def single(H, W, y=None, x=None):
    m = np.zeros((H, W), np.uint8)
    m[H // 2 if y is None else y, W // 2 if x is None else x] = 1
    return m


def square2(H, W):
    """An isolated 2 x 2 square (clipped by an image smaller than that)."""
    m = np.zeros((H, W), np.uint8)
    y, x = max(H // 2 - 1, 0), max(W // 2 - 1, 0)
    m[y:y + 2, x:x + 2] = 1
    return m


def diagonal(H, W):
    m = np.zeros((H, W), np.uint8)
    d = np.arange(min(H, W))
    m[d, d] = 1
    return m


def checkerboard(H, W):
    y, x = np.mgrid[:H, :W]
    return ((y + x) % 2).astype(np.uint8)


def noise(H, W, seed, density):
    return (np.random.RandomState(seed).rand(H, W) < density).astype(np.uint8)


GENERATORS = ("crack1", "crack2", "blobs", "full", "empty", "single", "square2", "diagonal", "checkerboard", "noise50",
              "noise80")


def generate(kind, H, W, seed=0):
    if kind == "crack1":
        return crack(H, W, seed, 1)
    if kind == "crack2":
        return crack(H, W, seed, 2)
    if kind == "blobs":
        return blobs(H, W, seed)
    if kind == "noise50":
        return noise(H, W, seed, 0.5)
    if kind == "noise80":
        return noise(H, W, seed, 0.8)
    return {"full": full, "empty": empty, "single": single, "square2": square2, "diagonal": diagonal,
            "checkerboard": checkerboard}[kind](H, W)


def all_masks(H, W, seed=0):
    """name -> mask: every generator at one size; every other mask holds 0 / 255 like a decoded 'L' image."""
    out = {k: generate(k, H, W, seed + i) for i, k in enumerate(GENERATORS)}
    for k in list(out)[1::2]:
        out[k] = out[k] * 255
    return out


def crack_map(H, W, seed):
    """A class map of thin structures: class 1 a band of half-width 2, class 2 one of half-width 1 drawn over it, the rest 0."""
    m = crack(H, W, seed, 2)
    m[crack(H, W, seed + 100, 1) == 1] = 2
    return m
