"""numpy restatement of vitseg_augment (include/vitseg.h "training augmentation"): int64 coordinates, fp32 operations one
at a time.  A plain helper module, imported like util.py; the kernel is expected to match it bit for bit."""
import numpy as np

CONSTANT, EDGE = 0, 1
LIN_MAX, OFF_MAX = 1 << 26, 1 << 40
IDENTITY = (65536, 0, 0, 0, 65536, 0)
f32 = np.float32


def clamp_matrix(M):
    """The kernel's clamp on load: m00, m01, m10, m11 to +-2^26 and m02, m12 to +-2^40."""
    M = np.asarray(M, np.int64).reshape(6).copy()
    for i in range(6):
        lim = OFF_MAX if i % 3 == 2 else LIN_MAX
        M[i] = min(max(int(M[i]), -lim), lim)
    return M


def coords(M, oh, ow):
    """(U, V) int64 [oh, ow]: Q16 source coordinates of every output pixel centre."""
    m = clamp_matrix(M)
    tx = (2 * np.arange(ow, dtype=np.int64) + 1)[None, :]
    ty = (2 * np.arange(oh, dtype=np.int64) + 1)[:, None]
    U = (m[0] * tx + m[1] * ty + 2 * m[2] - 65536) >> 1
    V = (m[3] * tx + m[4] * ty + 2 * m[5] - 65536) >> 1
    return U, V


def matrix(a, src_hw, dst_hw):
    """vitseg_augment_matrix's formula: rint(65536 [[Ws a00/Wd, Ws a01/Hd, Ws a02], [Hs a10/Wd, Hs a11/Hd, Hs a12]])."""
    a = [float(v) for v in a]
    Hs, Ws = (float(v) for v in src_hw)
    Hd, Wd = (float(v) for v in dst_hw)
    e = [Ws * a[0] / Wd, Ws * a[1] / Hd, Ws * a[2], Hs * a[3] / Wd, Hs * a[4] / Hd, Hs * a[5]]
    return np.array([int(np.rint(65536.0 * v)) for v in e], np.int64)


def _taps(U, V, H, W, border):
    ix, iy = U >> 16, V >> 16
    fx, fy = (U & 0xFFFF) >> 8, (V & 0xFFFF) >> 8
    w = [(256 - fy) * (256 - fx), (256 - fy) * fx, fy * (256 - fx), fy * fx]
    taps = []
    for dy, dx in ((0, 0), (0, 1), (1, 0), (1, 1)):
        x, y = ix + dx, iy + dy
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
        if border == EDGE:
            inside = np.ones_like(inside)
        taps.append((np.clip(y, 0, H - 1), np.clip(x, 0, W - 1), inside))
    return w, taps


def coverage(M, H, W, oh, ow):
    """Fractions of the output pixels whose four image taps are (all in frame, none in frame, some in frame)."""
    U, V = coords(M, oh, ow)
    _, taps = _taps(U, V, H, W, CONSTANT)
    cnt = sum(t[2].astype(np.int64) for t in taps)
    return float((cnt == 4).mean()), float((cnt == 0).mean()), float(((cnt > 0) & (cnt < 4)).mean())


def warp_image_one(src, M, oh, ow, border, fill):
    """One sample: src uint8 [H, W, 3] or float32 [3, H, W] -> float32 [3, oh, ow] before the colour step."""
    u8 = src.dtype == np.uint8
    H, W = (src.shape[0], src.shape[1]) if u8 else (src.shape[1], src.shape[2])
    U, V = coords(M, oh, ow)
    w, taps = _taps(U, V, H, W, border)
    out = np.empty((3, oh, ow), f32)
    for c in range(3):
        if u8:
            r = np.rint(f32(fill[c]))
            fc = 0 if not r >= 0 else int(min(r, 255))
            S = np.zeros((oh, ow), np.int64)
            for wk, (ty, tx, inside) in zip(w, taps):
                S += wk * np.where(inside, src[ty, tx, c].astype(np.int64), fc)
            out[c] = S.astype(f32) / f32(16711680.0)
        else:
            p = [np.where(inside, src[c][ty, tx], f32(fill[c])).astype(f32) for ty, tx, inside in taps]
            wf = [wk.astype(f32) for wk in w]
            s = (wf[0] * p[0] + wf[1] * p[1]).astype(f32)
            s = (s + wf[2] * p[2]).astype(f32)
            s = (s + wf[3] * p[3]).astype(f32)
            out[c] = s * f32(2.0 ** -16)
    return out


def colour_one(v, cm):
    """v float32 [3, oh, ow], cm float32 [12]: clamp(((c0 r + c1 g) + c2 b) + c3, 0, 1), each operation rounded on its own."""
    cm = np.asarray(cm, f32).reshape(3, 4)
    out = np.empty_like(v)
    for c in range(3):
        s = (cm[c, 0] * v[0] + cm[c, 1] * v[1]).astype(f32)
        s = (s + cm[c, 2] * v[2]).astype(f32)
        s = (s + cm[c, 3]).astype(f32)
        out[c] = np.fmin(np.fmax(s, f32(0)), f32(1))
    return out


def warp_mask_one(src, M, oh, ow, border, fill_label, out_dtype):
    """One sample: src uint8 / int64 [H, W] -> out_dtype [oh, ow] by nearest tap."""
    H, W = src.shape
    U, V = coords(M, oh, ow)
    jx, jy = (U + 32768) >> 16, (V + 32768) >> 16
    lab = src[np.clip(jy, 0, H - 1), np.clip(jx, 0, W - 1)].astype(np.int64)
    if border == CONSTANT:
        inside = (jx >= 0) & (jx < W) & (jy >= 0) & (jy < H)
        lab = np.where(inside, lab, np.int64(fill_label))
    return lab.astype(out_dtype)   # (int64 -> uint8 keeps the low byte, as the kernel's store does)


def augment(images, matrices, oh, ow, colour=None, border=EDGE, fill=(0, 0, 0), masks=(), fill_label=0):
    """The whole call.  images: uint8 [n, H, W, 3] or float32 [n, 3, H, W]; matrices int64 [n, 6]; colour float32 [n, 12] or
    None; masks: a sequence of (src [n, h, w], matrices [n, 6], oh, ow, out_dtype).  Returns (x float32 [n, 3, oh, ow],
    [warped mask, ...])."""
    n = images.shape[0]
    x = np.empty((n, 3, oh, ow), f32)
    for b in range(n):
        v = warp_image_one(images[b], matrices[b], oh, ow, border, fill)
        x[b] = v if colour is None else colour_one(v, colour[b])
    ys = []
    for src, Mm, mh, mw, dt in masks:
        ys.append(np.stack([warp_mask_one(src[b], Mm[b], mh, mw, border, fill_label, dt) for b in range(n)]))
    return x, ys
