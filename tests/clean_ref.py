"""numpy restatement of vitseg_clean_mask (include/vitseg.h): regions below a minimum area become background, then the
enclosed holes with one bordering class are filled.  No scipy: built on regions_ref._roots (union-find by minimum index), the
way regions_ref avoids it.  Also the cases and variants of tests/golden/clean/clean.npz.  A plain helper module, imported
like regions_ref.py."""
import numpy as np

import regions_ref as R

STATS = ("regions_removed", "pixels_removed", "holes_filled", "pixels_filled", "holes_mixed", "holes_over_area")


def clean_one(m, min_area=0, fill_holes=False, max_hole_area=0, connectivity=4, background=0):
    """(cleaned uint8 [H, W], int32 [6] in the order of STATS) of one uint8 [H, W] label map."""
    m = np.array(m, dtype=np.uint8)
    assert m.ndim == 2 and 0 <= background <= 255
    H, W = m.shape
    P = H * W
    flat = m.reshape(-1)
    st = dict.fromkeys(STATS, 0)
    if min_area > 1:   # step 1: regions of fewer than min_area pixels
        parent = R._roots(m, background, connectivity)
        valid = parent >= 0
        area = np.bincount(parent[valid], minlength=P)
        small = (area > 0) & (area < min_area)            # indexed by root
        gone = np.zeros(P, bool)
        gone[valid] = small[parent[valid]]
        st["regions_removed"], st["pixels_removed"] = int(small.sum()), int(gone.sum())
        flat[gone] = background
    if fill_holes:     # step 2: 4-connected background components off the frame, on the result of step 1
        parent = R._roots(m, -1, 4)                       # no background: every pixel has a root
        bg = flat == background
        ys, xs = np.divmod(np.arange(P), W)
        frame = (ys == 0) | (ys == H - 1) | (xs == 0) | (xs == W - 1)
        touches = np.zeros(P, bool)
        touches[parent[bg & frame]] = True
        area = np.bincount(parent[bg], minlength=P)
        cmin, cmax = np.full(P, 256), np.full(P, -1)
        idx = np.arange(P).reshape(H, W)
        for dy, dx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
            p = idx[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)].reshape(-1)
            q = p + dy * W + dx
            keep = bg[p] & ~bg[q]
            np.minimum.at(cmin, parent[p[keep]], flat[q[keep]])
            np.maximum.at(cmax, parent[p[keep]], flat[q[keep]])
        hole = (area > 0) & ~touches                      # indexed by root
        over = hole & (area > max_hole_area) if max_hole_area > 0 else np.zeros(P, bool)
        one = hole & ~over & (cmin == cmax)
        st["holes_over_area"] = int(over.sum())
        st["holes_mixed"] = int((hole & ~over & (cmin != cmax)).sum())
        st["holes_filled"], st["pixels_filled"] = int(one.sum()), int(area[one].sum())
        px = np.nonzero(bg)[0]
        px = px[one[parent[px]]]
        flat[px] = cmin[parent[px]]
    return m, np.array([st[k] for k in STATS], np.int32)


def clean_ref(mask, **kw):
    """The restatement of visiontransformer_amd.clean.clean_mask(..., return_stats=True) on a [n, H, W] or [H, W] array:
    (cleaned array, list of dicts; the dict itself for [H, W])."""
    m = np.asarray(mask)
    single = m.ndim == 2
    outs = [clean_one(mi, **kw) for mi in (m[None] if single else m)]
    out = np.stack([o for o, _ in outs]).astype(m.dtype)
    st = [dict(zip(STATS, (int(v) for v in s))) for _, s in outs]
    return (out[0], st[0]) if single else (out, st)


# ---- test masks ----

def speckle(seed, H, W, C, n=None, fraction=0.025, radius=5):
    """regions_ref.blobs with `fraction` of the pixels re-drawn uniformly over the C classes: islands of a few pixels and
    pinholes, as a per-pixel argmax leaves them."""
    m = R.blobs(seed, H, W, C, n=n, radius=radius)
    rs = np.random.RandomState(1000 + seed)
    hit = rs.rand(*m.shape) < fraction
    m[hit] = rs.randint(0, C, size=int(hit.sum())).astype(np.uint8)
    return m


def nested(H=96, W=120):
    """A 3-thick class-2 frame around a hole 74 wide that crosses tile seams, holding a 6-pixel class-5 island and a
    40-pixel class-2 island."""
    m = np.zeros((H, W), np.uint8)
    m[8:88, 10:110] = 2
    m[11:85, 13:107] = 0
    m[30:32, 40:43] = 5
    m[50:55, 60:68] = 2
    return m


def no_background(H=40, W=50):
    """Classes 1, 2 and 3 and no pixel of class 0; every region has 100 pixels or more."""
    m = np.ones((H, W), np.uint8)
    m[:, W // 2:] = 2
    m[10:20, 10:20] = 3
    return m


def clean_cases():
    """name -> (uint8 mask, background): the cases of tests/golden/clean/clean.npz."""
    g = R.golden_cases()
    s5 = speckle(12, 97, 131, 5)
    cases = {
        "speckle2_96x130": (speckle(11, 96, 130, 2), 0),
        "speckle5_97x131": (s5, 0),
        "speckle5_97x131_bg3": (s5, 3),
        "speckle17_224": (speckle(13, 224, 224, 17), 0),
        "nested_96x120": (nested(), 0),
        "allbg_40x50": (np.zeros((40, 50), np.uint8), 0),
        "nobg_40x50": (no_background(), 0),
    }
    for name in ("rings_96", "checker_64", "u_70x45", "serpentine_96", "strip_1x300", "strip_257x1"):
        cases[name] = (g[name], 0)
    return cases


# (min_area, fill_holes, max_hole_area, connectivity)
VARIANTS = [(8, 0, 0, 4), (8, 0, 0, 8), (0, 1, 0, 4), (8, 1, 0, 4), (8, 1, 0, 8), (8, 1, 20, 4)]
EXTRA_VARIANTS = {"nested_96x120": [(7, 1, 0, 4), (6, 1, 0, 4), (8, 1, 6916, 4), (8, 1, 6915, 4)]}
NO_HOLES = ("u_70x45", "serpentine_96", "strip_1x300", "strip_257x1")   # no enclosed background: fill_holes changes nothing
UNCHANGED = ("allbg_40x50", "nobg_40x50")                               # nothing to remove either: no variant changes them
TWO_CLASS = ("speckle2_96x130", "checker_64", "u_70x45", "serpentine_96")   # fill_holes there is binary_fill_holes


def variants(name):
    return VARIANTS + EXTRA_VARIANTS.get(name, [])


def key(name, variant):
    a, f, h, c = variant
    return f"{name}.a{a}.f{f}.h{h}.c{c}"
