#!/usr/bin/env python3
"""Writes tests/golden/clean/clean.npz: the masks of tests/clean_ref.clean_cases() and, for each of them and each variant
(min_area, fill_holes, max_hole_area, connectivity), the cleaned mask and the six statistics of vitseg_clean_mask
(include/vitseg.h) computed with scipy, independently of the numpy restatement: scipy.ndimage.label per class with a
bincount for the small regions; scipy.ndimage.label of the background, the components off the frame and the classes on
their dilation ring for the holes.  For the two-class cases without an area limit the filled mask is also required to be
scipy.ndimage.binary_fill_holes of the foreground, bit for bit.  Needs scipy.
Keys: "<case>.mask" uint8 [H, W]; "<case>.background" int; "<case>.a<min_area>.f<fill>.h<max_hole_area>.c<conn>.mask" uint8
[H, W] and "....stats" int32 [6]."""
import os
import sys

import numpy as np
from scipy import ndimage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clean_ref as K  # noqa: E402


def clean_scipy(m, min_area, fill_holes, max_hole_area, connectivity, background):
    out = m.copy()
    st = dict.fromkeys(K.STATS, 0)
    structure = None if connectivity == 4 else np.ones((3, 3), dtype=bool)
    if min_area > 1:
        for c in np.unique(m):
            if int(c) == background:
                continue
            lab, nf = ndimage.label(m == c, structure=structure)
            small = np.bincount(lab.reshape(-1), minlength=nf + 1) < min_area
            small[0] = False
            st["regions_removed"] += int(small.sum())
            st["pixels_removed"] += int(small[lab].sum())
            out[small[lab]] = background
    if fill_holes:
        src = out.copy()
        lab, nf = ndimage.label(src == background)   # the cross: 4-connected, binary_fill_holes' default structure
        on_frame = set(np.unique(np.concatenate([lab[0], lab[-1], lab[:, 0], lab[:, -1]]))) - {0}
        for k, sl in enumerate(ndimage.find_objects(lab), start=1):
            if k in on_frame:
                continue
            sl = tuple(slice(s.start - 1, s.stop + 1) for s in sl)   # off the frame: the window grown by one stays inside
            comp = lab[sl] == k
            ring = ndimage.binary_dilation(comp) & ~comp
            classes = np.unique(src[sl][ring])
            assert background not in classes
            area = int(comp.sum())
            if max_hole_area > 0 and area > max_hole_area:
                st["holes_over_area"] += 1
            elif len(classes) != 1:
                st["holes_mixed"] += 1
            else:
                st["holes_filled"] += 1
                st["pixels_filled"] += area
                out[sl][comp] = classes[0]
    return out, np.array([st[k] for k in K.STATS], np.int32)


def main():
    out = {}
    for name, (m, bg) in K.clean_cases().items():
        out[f"{name}.mask"] = m
        out[f"{name}.background"] = np.int32(bg)
        for v in K.variants(name):
            cm, st = clean_scipy(m, *v, bg)
            a, f, h, c = v
            if f and not h and name in K.TWO_CLASS:
                step1, _ = clean_scipy(m, a, 0, 0, c, bg)
                fg = int(m[m != bg][0])
                assert np.array_equal(cm != bg, ndimage.binary_fill_holes(step1 != bg)) and set(np.unique(cm)) <= {bg, fg}
            out[K.key(name, v) + ".mask"] = cm
            out[K.key(name, v) + ".stats"] = st
            print(f"{name:20s} {m.shape} bg {bg} min_area {a} fill {f} max_hole {h:4d} conn {c}: "
                  + " ".join(f"{k}={x}" for k, x in zip(K.STATS, st)))
    path = os.path.join(ROOT, "tests", "golden", "clean", "clean.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
