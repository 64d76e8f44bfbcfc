#!/usr/bin/env python3
"""Writes tests/golden/regions/regions.npz: the masks of tests/regions_ref.golden_cases() and, for each of them and each
(connectivity, background) of GOLDEN_VARIANTS, the region records the reference's own rule gives -- scipy.ndimage.label
per class present + np.argwhere per label (model/CE/testViTModel.py:34-42,171-185), extended by area and first pixel.
Needs scipy.  Keys: "<case>.mask" uint8 [H, W]; "<case>.c<conn>.b<bg>" int32 [k, 7]."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import regions_ref as R  # noqa: E402


def main():
    out = {}
    for name, m in R.golden_cases().items():
        out[f"{name}.mask"] = m
        for conn, bg in R.GOLDEN_VARIANTS:
            rec, _ = R.scipy_records(m, bg, conn)
            out[f"{name}.c{conn}.b{bg}"] = rec
            print(f"{name:16s} {m.shape} connectivity {conn} background {bg:2d}: {len(rec)} regions")
    path = os.path.join(ROOT, "tests", "golden", "regions", "regions.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
