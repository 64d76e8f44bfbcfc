"""CPU restatement of vitseg_decide (include/vitseg_decide.h): a class decided by threshold, with hysteresis.  Test
infrastructure, imported like util.py; the score is curves_ref's (confidence_ref under a mask that states the class everywhere),
the components scipy.ndimage.label's.

Per pixel i: weak(i): q_i >= low_q; strong(i): q_i >= high_q; kept(i): weak and its 4- / 8-connected component of weak pixels
holds a strong one.  mask_i = value where kept, else off, or with a base what base states unless that is `value` (then off).
counts per image: (weak, strong, kept).
"""
import numpy as np

import curves_ref as CV

STRUCTURE = {4: np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool), 8: np.ones((3, 3), bool)}


def kept_planes(q, high_q, low_q, connectivity=4):
    """(weak, strong, kept) bool [n, S, S] of the scores q integer [n, S, S]"""
    from scipy import ndimage
    q = np.asarray(q).astype(np.int64)
    weak, strong = q >= low_q, q >= high_q
    kept = np.zeros(q.shape, bool)
    for b in range(q.shape[0]):
        lab, _ = ndimage.label(weak[b], structure=STRUCTURE[connectivity])
        keep = np.unique(lab[strong[b]])
        kept[b] = np.isin(lab, keep[keep > 0])
    return weak, strong, kept


def apply(kept, base, value, off=0):
    """uint8 mask of the kept plane under the base rule"""
    if base is None:
        rest = np.full(kept.shape, off, np.uint8)
    else:
        rest = np.asarray(base).astype(np.uint8).copy()
        rest[rest == value] = off
    return np.where(kept, np.uint8(value), rest).astype(np.uint8)


def decide_q(q, high_q, low_q, connectivity=4, base=None, value=1, off=0):
    """(mask uint8 [n, S, S], counts int64 [n, 3]) from the scores"""
    weak, strong, kept = kept_planes(q, high_q, low_q, connectivity)
    counts = np.stack([p.reshape(p.shape[0], -1).sum(axis=1) for p in (weak, strong, kept)], axis=1).astype(np.int64)
    return apply(kept, base, value, off), counts


def decide(lowres, S, cls, kind, high_q, low_q, connectivity=4, base=None, value=None, off=0):
    """(mask, counts) of a low-res head output fp32 [n, C, g, g]"""
    q = CV.scores(lowres, S, cls, kind)
    return decide_q(q, high_q, low_q, connectivity, base, cls if value is None else value, off)
