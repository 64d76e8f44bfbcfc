#!/usr/bin/env python3
"""Writes tests/golden/sdf/sdf.npz: the masks of tests/sdf_ref.golden_cases(), scipy's distance_transform_edt of ~mask
("<case>.ext_d2") and of mask ("<case>.int_d2") as exact int32 squared distances (round(dist^2)), and for the cases of
NORMALIZED_CASES the normalised float32 pair of compute_sdf (model/PAED/segmentation.py:6-34) restated with scipy
("<case>.ext", "<case>.int").  Needs scipy."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sdf_ref as R  # noqa: E402


def main():
    out = {}
    for name, m in R.golden_cases().items():
        b = m != 0
        out[f"{name}.mask"] = m
        out[f"{name}.ext_d2"] = R.scipy_d2(~b).astype(np.int32)
        out[f"{name}.int_d2"] = R.scipy_d2(b).astype(np.int32)
        if name in R.NORMALIZED_CASES:
            out[f"{name}.ext"], out[f"{name}.int"] = R.scipy_compute_sdf(m)
        print(f"{name:20s} {m.shape} mask pixels {int(b.sum())}")
    path = os.path.join(ROOT, "tests", "golden", "sdf", "sdf.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
