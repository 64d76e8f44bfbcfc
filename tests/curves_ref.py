"""CPU restatement of vitseg_pr_counts (include/vitseg_curves.h): the precision-recall counts of one class' score map over all
thresholds, with a pixel tolerance.  Test infrastructure, imported like util.py; the score is confidence_ref's under a mask
that states the class everywhere, the disc a brute-force loop over its offsets on arrays padded with "absent", the counts three
bincounts.

Per pixel i: q_i = confidence_ref.confidence(lowres, full(cls), kind); valid(i): gt_i != ignore_label; pos(i): valid and
gt_i == cls; D = {(dy, dx): dy^2 + dx^2 <= tol2}; bin(q) = (q * bins) >> 16.
    pred   valid i by bin(q_i)
    hit    valid i with a pos j, i - j in D, by bin(q_i)
    found  pos j by bin(max{q_i: i valid, inside the frame, i - j in D})
"""
import numpy as np
import torch

import confidence_ref as CR

ABSENT = -1


def disc(tol2):
    """the offsets (dy, dx) with dy^2 + dx^2 <= tol2"""
    r = int(np.floor(np.sqrt(tol2)))
    while (r + 1) * (r + 1) <= tol2:
        r += 1
    return [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dy * dy + dx * dx <= tol2]


def disc_max(a, tol2, absent=ABSENT):
    """out[..., y, x] = max over (dy, dx) in D of a[..., y + dy, x + dx], `absent` outside the frame; a: integer [..., H, W]"""
    a = np.asarray(a)
    offs = disc(tol2)
    r = max(dy for dy, _ in offs)
    H, W = a.shape[-2:]
    pad = np.full(a.shape[:-2] + (H + 2 * r, W + 2 * r), absent, dtype=a.dtype)
    pad[..., r:r + H, r:r + W] = a
    out = np.full(a.shape, absent, dtype=a.dtype)
    for dy, dx in offs:
        np.maximum(out, pad[..., r + dy:r + dy + H, r + dx:r + dx + W], out=out)
    return out


def scores(lowres, S, cls, kind):
    """q int64 [n, S, S] of class `cls` at every pixel"""
    n = lowres.shape[0]
    return CR.confidence(lowres, torch.full((n, S, S), cls, dtype=torch.uint8), kind)[1]


def planes(q, gt, cls, tol2, ignore_label=-1):
    """(valid bool, pos bool, hit bool, best int64: the disc maximum of the valid scores, ABSENT where the disc holds none)"""
    q = np.asarray(q).astype(np.int64)
    t = np.asarray(gt).astype(np.int64)
    valid = t != ignore_label
    pos = valid & (t == cls)
    hit = valid & (disc_max(pos.astype(np.int8), tol2, 0) > 0)
    best = disc_max(np.where(valid, q, ABSENT).astype(np.int32), tol2).astype(np.int64)   # (q < 2^16: the narrow type is exact)
    return valid, pos, hit, best


def counts_from_planes(q, valid, pos, hit, best, bins):
    """int64 [n, bins, 3] from the planes of `planes`"""
    q = np.asarray(q).astype(np.int64)
    n = q.shape[0]
    out = np.zeros((n, bins, 3), dtype=np.int64)
    for b in range(n):
        assert (best[b][pos[b]] >= q[b][pos[b]]).all()   # a true pixel is in its own disc
        out[b, :, 0] = np.bincount((q[b][valid[b]] * bins) >> 16, minlength=bins)
        out[b, :, 1] = np.bincount((q[b][hit[b]] * bins) >> 16, minlength=bins)
        out[b, :, 2] = np.bincount((best[b][pos[b]] * bins) >> 16, minlength=bins)
    return out


def pr_counts(lowres, gt, cls, kind, bins, tol2, ignore_label=-1):
    """int64 [n, bins, 3] of a low-res head output fp32 [n, C, g, g] and a ground truth uint8 [n, S, S]"""
    q = scores(lowres, gt.shape[-1], cls, kind)
    return counts_from_planes(q, *planes(q, gt, cls, tol2, ignore_label), bins)
