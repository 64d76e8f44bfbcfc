"""Two restatements of the soft-clDice loss (include/vitseg_cldice.h) for the tests (a plain helper module, imported like
util.py):

(a) the published composition in torch -- soft_erode = min(-max_pool2d(-x, (3,1)), -max_pool2d(-x, (1,3))), soft_dilate =
    max_pool2d(x, (3,3)), soft_skel, the loss of Shit et al. (CVPR 2021) per class -- differentiated by autograd, usable in
    fp32 and fp64;
(b) an explicit gather-form adjoint in numpy (fp64) that implements the tie rules by hand and takes no help from autograd:
    relu'(0) = 0, a pooling window hands its gradient to the first extremal tap in row-major window order, min(m_col, m_row)
    gives all to the smaller and half to each when equal.  `pool_rule="last"` and `min_rule="col"` switch a rule to a wrong
    one, for the sensitivity tests.

Also the planes and targets the CPU and the GPU tests share.
"""
import numpy as np
import torch
import torch.nn.functional as F


# ---- (a) the published composition ----

def soft_erode(x):
    p1 = -F.max_pool2d(-x, (3, 1), (1, 1), (1, 0))
    p2 = -F.max_pool2d(-x, (1, 3), (1, 1), (0, 1))
    return torch.min(p1, p2)


def soft_dilate(x):
    return F.max_pool2d(x, (3, 3), (1, 1), (1, 1))


def soft_open(x):
    return soft_dilate(soft_erode(x))


def soft_skel(img, iters):
    """img: [n, H, W] (any float dtype); the published soft_skel."""
    img = img.unsqueeze(1)
    skel = F.relu(img - soft_open(img))
    for _ in range(iters):
        img = soft_erode(img)
        delta = F.relu(img - soft_open(img))
        skel = skel + F.relu(delta - skel * delta)
    return skel.squeeze(1)


def cldice_terms(p, y, void, iters, smooth):
    """(cl, tprec, tsens) of one class: p, y [n, H, W] of one dtype, void a bool mask; differentiable w.r.t. p."""
    keep = (~void).to(p.dtype)
    p, y = p * keep, y * keep
    sp, st = soft_skel(p, iters), soft_skel(y, iters)
    tprec = ((sp * y).sum() + smooth) / (sp.sum() + smooth)
    tsens = ((st * p).sum() + smooth) / (st.sum() + smooth)
    return 1.0 - 2.0 * tprec * tsens / (tprec + tsens), tprec, tsens


def cldice_autograd(p, y, void, iters, smooth, dtype):
    """Terms and d cl / d p of restatement (a) in `dtype`, from the same fp32 planes: ((cl, tprec, tsens) floats, grad)."""
    q = p.detach().to(dtype).clone().requires_grad_(True)
    cl, tp, ts = cldice_terms(q, y.to(dtype), void, iters, smooth)
    cl.backward()
    return (cl.item(), tp.item(), ts.item()), q.grad.detach()


# ---- (b) the explicit adjoint ----

def _shift(a, dy, dx, fill):
    """out[y, x] = a[y - dy, x - dx] (fill outside): what the pixel at offset (-dy, -dx) holds, moved to (y, x)."""
    n, H, W = a.shape
    out = np.full_like(a, fill)
    ys, yd = (slice(0, H - dy), slice(dy, H)) if dy >= 0 else (slice(-dy, H), slice(0, H + dy))
    xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
    out[:, yd, xd] = a[:, ys, xs]
    return out


def _pick(stack, largest, rule):
    """Index of the extremal entry along axis 0: the first (torch) or, rule == "last", the last one."""
    f = np.argmax if largest else np.argmin
    if rule == "first":
        return f(stack, axis=0)
    assert rule == "last", rule
    return stack.shape[0] - 1 - f(stack[::-1], axis=0)


def _erode(I, pool_rule, min_rule):
    """erode(I) and its choices: (m, ct, rt, wc, wr); ct / rt in {-1, 0, 1}."""
    inf = np.inf
    col = np.stack([_shift(I, 1, 0, inf), I, _shift(I, -1, 0, inf)])    # up, centre, down
    row = np.stack([_shift(I, 0, 1, inf), I, _shift(I, 0, -1, inf)])    # left, centre, right
    ci, ri = _pick(col, False, pool_rule), _pick(row, False, pool_rule)
    mc, mr = np.take_along_axis(col, ci[None], 0)[0], np.take_along_axis(row, ri[None], 0)[0]
    if min_rule == "half":
        wc = (mc < mr) + 0.5 * (mc == mr)
    else:
        assert min_rule == "col", min_rule
        wc = (mc <= mr).astype(I.dtype)
    return np.minimum(mc, mr), ci - 1, ri - 1, wc, 1.0 - wc


_TAPS = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]   # dy-major, then dx


def _dilate(I, pool_rule):
    stack = np.stack([_shift(I, -dy, -dx, -np.inf) for dy, dx in _TAPS])
    ti = _pick(stack, True, pool_rule)
    return np.take_along_axis(stack, ti[None], 0)[0], ti


def _erode_adjoint(T, ct, rt, wc, wr):
    """Each input pixel collects T x share from the outputs whose chosen tap it is."""
    g = np.zeros_like(T)
    for d in (-1, 0, 1):
        g += _shift(T * wc * (ct == d), d, 0, 0.0)   # the output at (y - d, x) chose the tap d rows below itself
        g += _shift(T * wr * (rt == d), 0, d, 0.0)
    return g


def _dilate_adjoint(gO, ti):
    g = np.zeros_like(gO)
    for t, (dy, dx) in enumerate(_TAPS):
        g += _shift(gO * (ti == t), dy, dx, 0.0)
    return g


def skel_forward_np(I0, iters, pool_rule="first", min_rule="half"):
    """soft_skel in numpy with everything the adjoint needs."""
    I = [I0]
    er = []
    for _ in range(iters + 1):
        m, ct, rt, wc, wr = _erode(I[-1], pool_rule, min_rule)
        er.append((ct, rt, wc, wr))
        I.append(m)
    st = []
    skel = None
    for k in range(iters + 1):
        O, ti = _dilate(I[k + 1], pool_rule)
        v = I[k] - O
        D = np.maximum(v, 0.0) * (v > 0)
        prev = skel
        if k == 0:
            u = None
            skel = D
        else:
            u = D - prev * D
            skel = prev + np.maximum(u, 0.0) * (u > 0)
        st.append((ti, v, D, prev, u))
    return skel, (I, er, st)


def skel_adjoint_np(gs, saved, iters):
    """d L / d I_0 from gs = d L / d skel, by gathers."""
    I, er, st = saved
    A = None   # what I_{k+1} collected as stage k+1's own input
    for k in range(iters, -1, -1):
        ti, v, D, prev, u = st[k]
        if k > 0:
            r = gs * (u > 0)
            gD = r - r * prev
            gs = gs - r * D
        else:
            gD = gs
        gv = gD * (v > 0)
        T = _dilate_adjoint(-gv, ti)
        if A is not None:
            T = T + A
        A = gv + _erode_adjoint(T, *er[k])
    return A


def cldice_explicit(p, y, void, iters, smooth, pool_rule="first", min_rule="half"):
    """Restatement (b) in fp64: ((cl, tprec, tsens), d cl / d p) with numpy arrays [n, H, W]."""
    keep = ~np.asarray(void)
    p = np.asarray(p, dtype=np.float64) * keep
    y = np.asarray(y, dtype=np.float64) * keep
    sp, saved = skel_forward_np(p, iters, pool_rule, min_rule)
    st, _ = skel_forward_np(y, iters, pool_rule, min_rule)
    dp, ds = sp.sum() + smooth, st.sum() + smooth
    tp, ts = ((sp * y).sum() + smooth) / dp, ((st * p).sum() + smooth) / ds
    cl = 1.0 - 2.0 * tp * ts / (tp + ts)
    dtp, dts = -2.0 * ts * ts / (tp + ts) ** 2, -2.0 * tp * tp / (tp + ts) ** 2
    alpha, beta, gamma = dtp / dp, -dtp * tp / dp, dts / ds
    g = skel_adjoint_np(alpha * y + beta, saved, iters) + gamma * st
    return (cl, tp, ts), g * keep


# ---- shared cases ----

def line_target(n, H, W, seed=0):
    """0/1 planes of thin lines (1-3 px): a row band, a column band and a diagonal per image, some touching the frame; never
    a full plane."""
    rng = np.random.RandomState(seed)
    t = np.zeros((n, H, W), dtype=np.uint8)
    for i in range(n):
        w = 1 + (i + seed) % 3
        r0 = 0 if i % 2 == 0 else int(rng.randint(0, max(H - w, 1)))       # even images: the band touches the top edge
        t[i, r0:r0 + w, :] = 1
        c0 = max(W - w, 0) if i % 3 == 0 else int(rng.randint(0, max(W - w, 1)))
        if W > 3 * w:
            t[i, :, c0:c0 + w] = 1
        if H > 4 and W > 4:
            for d in range(min(H, W)):
                t[i, d, max(0, min(W - 1, d + i)):max(0, min(W, d + i + w))] = 1
        if H == 1 or W == 1:   # a line image: leave gaps, so that the plane is not full
            t[i] = 0
            t[i].reshape(-1)[1::3] = 1
    assert t.min() == 0 or t.size == 1
    return torch.from_numpy(t)


def make_plane(kind, n, H, W, target, seed=0):
    """fp32 probability planes [n, H, W]: "smooth" (a blurred target plus noise), "eighths" (round(8 p) / 8: ties everywhere),
    "binary" (0/1) and "clamped" (values in (0, 1) with exact 0 and exact 1 among them)."""
    g = torch.Generator().manual_seed(1000 + seed)
    t = target.float()
    blur = F.avg_pool2d(t.unsqueeze(1), 3, 1, 1, count_include_pad=False).squeeze(1)
    p = (0.15 + 0.6 * blur + 0.25 * torch.rand((n, H, W), generator=g)).clamp(0.0, 1.0)
    if kind == "smooth":
        return p.contiguous()
    if kind == "eighths":
        return (torch.round(p * 8) / 8).contiguous()
    if kind == "binary":
        return (p > 0.55).float().contiguous()
    assert kind == "clamped", kind
    p = ((p - 0.3) * 2.0).clamp(0.0, 1.0).contiguous()
    p.view(-1)[0], p.view(-1)[-1] = 0.0, 1.0   # both ends are there on the smallest plane too
    return p


def void_mask(n, H, W, fraction, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.rand((n, H, W), generator=g) < fraction
