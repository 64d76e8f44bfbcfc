"""Two restatements of the Lovasz-Softmax loss (Berman, Triki and Blaschko, CVPR 2018) for the tests (a plain helper module,
imported like cldice_ref.py).

(a) `lovasz_grad`, `lovasz_softmax_flat`, `lovasz_softmax`: the published composition in torch -- |fg - p| sorted descending, the
    gradient of the Jaccard loss by two cumsums and a difference, a dot product -- with a stable sort, under autograd.
(b) `closed_form`: the same in integers, in numpy, on the bit patterns of fp32 errors: what include/vitseg_lovasz.h states, rank by
    rank.  `sort_key` is the header's key; `term` joins segments into the term of a fused call with its g planes.
"""
import numpy as np
import torch

VOID_KEY = 0xFFFFFFFF


# ---------------------------------------------------------------- (a) the published composition
def lovasz_grad(gt_sorted):
    p = gt_sorted.numel()
    gts = gt_sorted.sum()
    intersection = gts - gt_sorted.cumsum(0)
    union = gts + (1 - gt_sorted).cumsum(0)
    jaccard = 1.0 - intersection / union
    if p > 1:
        jaccard = torch.cat([jaccard[:1], jaccard[1:] - jaccard[:-1]])
    return jaccard


def lovasz_softmax_flat(probas, labels, classes="present"):
    """probas [P, C], labels [P] (no void left).  classes: 'present', 'all' or a list.  Returns (the mean, {class: loss})."""
    per = {}
    if probas.numel() == 0:
        return probas.sum() * 0.0, per
    C = probas.shape[1]
    todo = list(range(C)) if classes in ("all", "present") else list(classes)
    for c in todo:
        fg = (labels == c).to(probas.dtype)
        if classes == "present" and fg.sum() == 0:
            continue
        errors = (fg - probas[:, c]).abs()
        errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
        per[c] = torch.dot(errors_sorted, lovasz_grad(fg[perm]))
    if not per:
        return probas.sum() * 0.0, per
    return sum(per.values()) / len(per), per


def lovasz_softmax(probas, labels, classes="present", per_image=False, ignore=None, present=True):
    """probas [B, C, H, W], labels [B, H, W].  `classes`: 'present' / 'all' as published, or a list, which `present` then
    filters per segment as 'present' does."""
    def flat(pr, lab):
        B, C = pr.shape[0], pr.shape[1]
        pr = pr.permute(0, 2, 3, 1).reshape(-1, C)
        lab = lab.reshape(-1)
        if ignore is not None:
            keep = lab != ignore
            pr, lab = pr[keep], lab[keep]
        cl = classes
        if not isinstance(cl, str) and present:
            cl = [c for c in cl if (lab == c).any()]
        return lovasz_softmax_flat(pr, lab, cl)[0]
    if per_image:
        return sum(flat(pr[None], lab[None]) for pr, lab in zip(probas, labels)) / probas.shape[0]
    return flat(probas, labels)


# ---------------------------------------------------------------- (b) the closed form in integers
def errors32(prob, y):
    """e = y ? 1 - p : p in fp32: one subtraction or none."""
    prob = np.asarray(prob, dtype=np.float32)
    return np.where(y, np.float32(1.0) - prob, prob).astype(np.float32)


def sort_key(e32):
    """The header's key: ascending keys = descending errors by bit pattern; a NaN is the canonical quiet NaN and ranks first."""
    e32 = np.ascontiguousarray(e32, dtype=np.float32)
    b = e32.view(np.uint32).copy()
    b[np.isnan(e32)] = 0x7FC00000
    u = np.where(b & np.uint32(0x80000000), ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)
    return ~u


def closed_form(e32, y, valid=None, coef=1.0, dtype=np.float32):
    """One segment.  e32 fp32 [L] errors, y bool [L], valid bool [L] (None: all).  Returns (L_c as a Python float from fp64,
    grad [L] = (dtype)(coef * dJ * (y ? -1 : +1)), fp32 as the device writes it, with +0 at void pixels, order int32 [L] with -1 past the valid ranks, G)."""
    e32 = np.ascontiguousarray(e32, dtype=np.float32).reshape(-1)
    y = np.asarray(y, dtype=bool).reshape(-1)
    L = e32.size
    valid = np.ones(L, dtype=bool) if valid is None else np.asarray(valid, dtype=bool).reshape(-1)
    idx = np.flatnonzero(valid)
    key = sort_key(e32[idx])
    assert not (key == VOID_KEY).any()
    rank = idx[np.argsort(key, kind="stable")]   # equal keys: ascending pixel index
    n = rank.size
    order = np.full(L, -1, dtype=np.int32)
    order[:n] = rank
    grad = np.zeros(L, dtype=dtype)
    ys = y[rank].astype(np.int64)
    G = int(ys.sum())
    if n == 0:
        return 0.0, grad, order, G
    r = np.arange(1, n + 1, dtype=np.int64)
    F = np.cumsum(ys)
    U = G + (r - F)
    with np.errstate(divide="ignore", invalid="ignore"):
        d1 = 1.0 / U.astype(np.float64)
        d0 = (G - F).astype(np.float64) / ((U - 1).astype(np.float64) * U.astype(np.float64))
    dJ = np.where(ys == 1, d1, np.where(U - 1 == 0, 1.0, d0))
    loss = float(np.sum(e32[rank].astype(np.float64) * dJ))
    grad[rank] = (np.float64(coef) * dJ * np.where(ys == 1, -1.0, 1.0)).astype(dtype)
    return loss, grad, order, G


def term(e, y, valid, per_image, present_only, weight=1.0, gscale=1.0, dtype=np.float32):
    """The term of a fused call from its planes: e fp32 [K, B, P] errors, y bool [K, B, P], valid bool [B, P].  Returns (the
    term, L_c per segment [K] or [K, B], the g planes fp32 [K, B, P]) by the header's rules: K', coef, the means."""
    K, B, P = e.shape
    groups = B if per_image else 1
    seg = (lambda a, k, q: a[k, q]) if per_image else (lambda a, k, q: a[k].reshape(-1))
    vseg = (lambda q: valid[q]) if per_image else (lambda q: valid.reshape(-1))
    Lc = np.zeros((K, groups))
    g = np.zeros((K, B, P), dtype=dtype)
    total = 0.0
    for q in range(groups):
        Gs = [int((seg(y, k, q) & vseg(q)).sum()) for k in range(K)]
        on = [not present_only or Gs[k] > 0 for k in range(K)]
        kp = sum(on)
        coef = 0.0
        if kp:
            coef = (np.float64(np.float32(weight)) * np.float64(np.float32(gscale))) / np.float64(kp)
            if per_image:
                coef = coef / np.float64(B)
        m = 0.0
        for k in range(K):
            Lc[k, q], gk, _, _ = closed_form(seg(e, k, q), seg(y, k, q), vseg(q), coef, dtype)
            if on[k]:
                m += Lc[k, q]
                if per_image:
                    g[k, q] = gk
                else:
                    g[k] = gk.reshape(B, P)
        total += m / kp if kp else 0.0
    if per_image:
        total = total / B
    return total, (Lc if per_image else Lc[:, 0]), g


# ---------------------------------------------------------------- planes for the tests
def make_plane(kind, n, L, seed):
    """fp32 [n, L] probabilities of the named kind (tests/test_gpu_lovasz.py lists them)."""
    gen = np.random.default_rng(seed)
    x = np.linspace(0.0, 1.0, L, dtype=np.float64)[None, :].repeat(n, 0)
    if kind == "smooth":
        p = 0.5 + 0.45 * np.sin(7.0 * x + np.arange(n)[:, None]) + 0.04 * gen.standard_normal((n, L))
    elif kind == "eighths":
        p = np.round(gen.random((n, L)) * 8.0) / 8.0
    elif kind == "constant":
        p = np.full((n, L), 0.375)
    elif kind == "sorted":
        p = 1.0 - x * 0.999
    elif kind == "reversed":
        p = x * 0.999
    elif kind == "lowest digit":     # errors 0.5 + j 2^-24, j < 256: the keys differ in their lowest byte alone
        p = 0.5 + gen.integers(0, 256, (n, L)) * 2.0 ** -24
    elif kind == "highest digit":    # powers of two far apart: the low three bytes of every key are the same
        p = 2.0 ** -(2.0 * gen.integers(0, 60, (n, L)))
    elif kind == "zeros and ones":
        p = gen.integers(0, 2, (n, L)).astype(np.float64)
    else:
        raise ValueError(kind)
    return np.clip(p, 0.0, 1.0).astype(np.float32)


def make_truth(n, L, seed, void=0.0, positive=0.3):
    """uint8 [n, L]: 1 = the class, 0 = not, 255 = void."""
    gen = np.random.default_rng(seed)
    t = (gen.random((n, L)) < positive).astype(np.uint8)
    if void > 0:
        t[gen.random((n, L)) < void] = 255
    return t
