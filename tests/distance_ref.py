"""numpy restatement of vitseg_distance_stats (include/vitseg.h), written from its definitions: per image and class c the
sets A = {gt == c} and P = {pred == c} (mode 0) or their 4-neighbour borders S ^ binary_erosion(S) (mode 1), the counts, the
fp64 sums of every pixel's distance to the nearest pixel of the other set, the maximal squared distances and the two order
statistics of the pooled squared distances around a rational percentile.  Two routes: "brute" over all pixel pairs in float64
(no scipy), and "scipy" (distance_transform_edt, binary_erosion); a third, "edt", reads sdf_ref's numpy distance transform
and serves the larger device cases where all pairs would take too long.  Also the test cases.  A plain helper module, imported like
sdf_ref.py."""
import numpy as np

MODES = {"sets": 0, "borders": 1}


def border_numpy(S):
    """S ^ erosion of S by the cross, border_value 0: the pixels of S with a 4-neighbour outside S or outside the image."""
    S = np.asarray(S, dtype=bool)
    p = np.pad(S, 1, constant_values=False)
    inner = p[1:-1, 1:-1] & p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:]
    return S & ~inner


def border_scipy(S):
    from scipy.ndimage import binary_erosion
    S = np.asarray(S, dtype=bool)
    return S ^ binary_erosion(S)   # scipy's defaults: the cross structure, border_value = 0


def sets_of(gt, pred, c, mode, route="brute"):
    A, P = np.asarray(gt) == c, np.asarray(pred) == c
    if mode == 1:
        b = border_scipy if route == "scipy" else border_numpy
        A, P = b(A), b(P)
    return A, P


def d2_to_set_brute(src, dst):
    """int64 [|src|]: squared distance of every pixel of `src` to the nearest pixel of `dst` (both non-empty), the minimum over
    all pairs taken in float64 (the squares are integers below 2^53: exact)."""
    s = np.argwhere(src).astype(np.float64)
    d = np.argwhere(dst).astype(np.float64)
    out = np.empty(len(s), np.int64)
    for lo in range(0, len(s), 512):   # chunks keep the pair matrix small
        blk = s[lo:lo + 512]
        dd = (blk[:, None, 0] - d[None, :, 0]) ** 2 + (blk[:, None, 1] - d[None, :, 1]) ** 2
        out[lo:lo + 512] = dd.min(axis=1).astype(np.int64)
    return out


def d2_to_set_scipy(src, dst):
    from scipy.ndimage import distance_transform_edt
    d = distance_transform_edt(~dst)   # distance of every pixel to the nearest pixel of dst
    return np.rint(d[src] * d[src]).astype(np.int64)


def ranks(N, pct_num, pct_den):
    lo = pct_num * (N - 1) // pct_den
    return lo, min(lo + 1, N - 1)


def d2_to_set_edt(src, dst):
    """The same from sdf_ref.edt2, the numpy distance transform that needs no scipy: for the larger device cases."""
    import sdf_ref
    return sdf_ref.edt2(dst)[src].astype(np.int64)


ROUTES = {"brute": d2_to_set_brute, "scipy": d2_to_set_scipy, "edt": d2_to_set_edt}


def fields_one(gt, pred, c, mode, route="brute"):
    """(n, m, d2 of A's pixels to P, d2 of P's pixels to A, float64 [2] sums) of one image and class; the d2 arrays are None
    when either set is empty."""
    A, P = sets_of(gt, pred, c, mode, route)
    n, m = int(A.sum()), int(P.sum())
    sf = np.zeros(2, np.float64)
    if n == 0 or m == 0:
        if mode == 0:   # the reference's rule: the non-empty set's distances to the index origin
            for k, S in enumerate((A, P)):
                yx = np.argwhere(S).astype(np.float64)
                sf[k] = np.sqrt(yx[:, 0] ** 2 + yx[:, 1] ** 2).sum()
        return n, m, None, None, sf
    ap, pa = ROUTES[route](A, P), ROUTES[route](P, A)
    sf[0], sf[1] = np.sqrt(ap.astype(np.float64)).sum(), np.sqrt(pa.astype(np.float64)).sum()
    return n, m, ap, pa, sf


def stats_of_fields(fields, pct_num, pct_den):
    """(int64 [6], float64 [2]): n, m, max_d2_AP, max_d2_PA, d2_lo, d2_hi and sumAP, sumPA."""
    n, m, ap, pa, sf = fields
    si = np.array([n, m, -1, -1, -1, -1], np.int64)
    if ap is not None:
        pooled = np.sort(np.concatenate([ap, pa]))
        lo, hi = ranks(n + m, pct_num, pct_den)
        si[2:] = ap.max(), pa.max(), pooled[lo], pooled[hi]
    return si, sf.copy()


def stats_one(gt, pred, c, mode, pct_num, pct_den, route="brute"):
    return stats_of_fields(fields_one(gt, pred, c, mode, route), pct_num, pct_den)


def stats_ref_multi(gt, pred, classes, mode, percentiles, route="brute"):
    """The restatement of vitseg_distance_stats on uint8 [n, H, W] maps for several percentiles (num, den) at once:
    {(num, den): (stats_i int64 [n, K, 6], stats_f float64 [n, K, 2])}; the distances are computed once."""
    gt, pred = np.asarray(gt), np.asarray(pred)
    n, K = gt.shape[0], len(classes)
    out = {tuple(p): (np.zeros((n, K, 6), np.int64), np.zeros((n, K, 2), np.float64)) for p in percentiles}
    for i in range(n):
        for k, c in enumerate(classes):
            f = fields_one(gt[i], pred[i], c, mode, route)
            for p, (si, sf) in out.items():
                si[i, k], sf[i, k] = stats_of_fields(f, *p)
    return out


def stats_ref(gt, pred, classes, mode, pct_num, pct_den, route="brute"):
    return stats_ref_multi(gt, pred, classes, mode, [(pct_num, pct_den)], route)[(pct_num, pct_den)]


def pooled_distances(gt, pred, c, mode):
    """float64 distances of the pooled multiset of one image and class (both sets non-empty), for np.percentile."""
    A, P = sets_of(gt, pred, c, mode)
    return np.sqrt(np.concatenate([d2_to_set_brute(A, P), d2_to_set_brute(P, A)]).astype(np.float64))


def sum_bound(N):
    """Relative bound on an fp64 sum of N non-negative correctly rounded roots against another such sum taken in any order:
    (N - 1) roundings of the additions and half an ulp of each root, 2^-53 each, on both sides."""
    return 2.0 * (N + 1) * 2.0 ** -53


# ---- test maps (uint8 class maps) ----

def random_map(seed, H, W, density, c=1):
    return (np.random.RandomState(seed).rand(H, W) < density).astype(np.uint8) * c


def shifted(m, dy, dx):
    """m moved by (dy, dx), zeros shifted in."""
    H, W = m.shape
    out = np.zeros_like(m)
    ys, yd = (slice(0, H - dy), slice(dy, H)) if dy >= 0 else (slice(-dy, H), slice(0, H + dy))
    xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
    out[yd, xd] = m[ys, xs]
    return out


def class_map(seed, H, W, num_classes):
    """Blocky random regions of num_classes labels, like a segmentation map."""
    rs = np.random.RandomState(seed)
    small = rs.randint(0, num_classes, ((H + 7) // 8, (W + 7) // 8)).astype(np.uint8)
    m = np.kron(small, np.ones((8, 8), np.uint8))[:H, :W]
    noise = rs.rand(H, W) < 0.03
    m[noise] = rs.randint(0, num_classes, int(noise.sum()))
    return np.ascontiguousarray(m)


def bucket_straddle_case(a, b):
    """A 1 x (b + 1) strip, class 1: gt = the pixel at column 0, pred = the pixels at columns a < b.  The pooled squared
    distances are [a^2, a^2, b^2], so at the median lo = 1 and hi = 2 pick a^2 and b^2.  (31, 33) puts 961 and 1089 on the two
    sides of 2^10, (1023, 1025) puts 1046529 and 1050625 on the two sides of 2^20: the boundaries of a 10-bit radix select's
    second and first digit, after which the two ranks follow different prefixes."""
    gt = np.zeros((1, b + 1), np.uint8)
    pred = np.zeros((1, b + 1), np.uint8)
    gt[0, 0] = 1
    pred[0, a] = pred[0, b] = 1
    return gt, pred


def plateau_case():
    """A long plateau of ties at the rank: gt a full row, pred the row 5 below it and one far pixel; all but a few of the 141
    pooled keys are 25."""
    gt = np.zeros((12, 70), np.uint8)
    pred = np.zeros((12, 70), np.uint8)
    gt[2, :] = 1
    pred[7, :] = 1
    pred[0, 0] = 1
    return gt, pred


def single_pixels(H, W):
    gt = np.zeros((H, W), np.uint8)
    pred = np.zeros((H, W), np.uint8)
    gt[0, 0] = 1
    pred[H - 1, W - 1] = 1
    return gt, pred


SIZES = [(1, 1), (1, 9), (7, 1), (13, 21), (61, 77), (64, 300)]


def mask_cases(H, W, seed=0):
    """name -> (gt, pred) uint8 maps with labels 0 / 1 at one size: the kinds the device tests run at every size."""
    g3 = random_map(seed + 1, H, W, 0.3)
    z = np.zeros((H, W), np.uint8)
    one = np.ones((H, W), np.uint8)
    cases = {
        "sparse": (random_map(seed + 2, H, W, 0.02), random_map(seed + 3, H, W, 0.02)),
        "medium": (g3, random_map(seed + 4, H, W, 0.3)),
        "dense": (random_map(seed + 5, H, W, 0.7), random_map(seed + 6, H, W, 0.7)),
        "shifted": (g3, shifted(g3, min(2, H - 1), -min(3, W - 1))),
        "identical_zero": (z, z.copy()),
        "single": single_pixels(H, W),
        "gt_empty": (z, g3),
        "pred_empty": (g3, z.copy()),
        "full": (one, one.copy()),
        "full_vs_medium": (one, g3),
    }
    return cases


def golden_cases():
    """name -> (gt, pred, classes): the cases of tests/golden/distance/distance.npz."""
    out = {}
    for H, W in [(1, 9), (13, 21), (61, 77)]:
        for name, (g, p) in mask_cases(H, W, seed=H).items():
            if name in ("medium", "shifted", "single", "gt_empty", "full_vs_medium"):
                out[f"{name}_{H}x{W}"] = (g, p, [0, 1, 7])
    out["straddle_2p10"] = bucket_straddle_case(31, 33) + ([1],)
    out["straddle_2p20"] = bucket_straddle_case(1023, 1025) + ([1],)
    out["plateau"] = plateau_case() + ([0, 1],)
    out["classes_40x56"] = (class_map(3, 40, 56, 4), class_map(4, 40, 56, 4), [0, 1, 2, 3])
    return out


GOLDEN_PERCENTILES = [(0, 1), (1, 2), (19, 20), (1, 1)]   # 0, 50, 95, 100
