#!/usr/bin/env python3
"""Writes tests/golden/distance/distance.npz: the class maps of tests/distance_ref.golden_cases() ("<case>.gt", "<case>.pred",
"<case>.classes") and, for both modes and the percentiles 0, 50, 95 and 100, what vitseg_distance_stats must return for them,
computed with scipy (distance_transform_edt, binary_erosion): "<case>.m<mode>.p<num>_<den>.i" int64 [K, 6] and ".f" float64
[K, 2].  Needs scipy."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import distance_ref as R  # noqa: E402


def main():
    out = {}
    for name, (gt, pred, classes) in R.golden_cases().items():
        out[f"{name}.gt"], out[f"{name}.pred"] = gt, pred
        out[f"{name}.classes"] = np.asarray(classes, np.int32)
        for mode in (0, 1):
            res = R.stats_ref_multi(gt[None], pred[None], classes, mode, R.GOLDEN_PERCENTILES, route="scipy")
            for (num, den), (si, sf) in res.items():
                out[f"{name}.m{mode}.p{num}_{den}.i"] = si[0]
                out[f"{name}.m{mode}.p{num}_{den}.f"] = sf[0]
        print(f"{name:24s} {gt.shape} classes {classes}")
    path = os.path.join(ROOT, "tests", "golden", "distance", "distance.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 256 * 1024


if __name__ == "__main__":
    main()
