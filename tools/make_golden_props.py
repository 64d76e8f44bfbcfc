#!/usr/bin/env python3
"""Writes tests/golden/props/props.npz: the masks of tests/props_ref.golden_cases() and the rows vitseg_region_props
(include/vitseg.h) has to return for them, computed from the definitions alone -- tests/props_ref.props_naive, region by
region from np.argwhere -- on the labelling of the real scipy.ndimage.label (regions_ref.scipy_records: one call per class
present) and scipy's distance_transform_edt, independently of the numpy restatement's union-find and of its loop over the
labels.  Needs scipy.
Keys: "<case>.mask" uint8 [H, W]; "<case>.classes" int32 [K]; "<case>.params" int32 [2] (background, connectivity);
"<case>.props" int64 [k, 20]."""
import os
import sys

import numpy as np
from scipy import ndimage  # noqa: F401  (the helpers import it lazily: fail here, with a clear message)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import props_ref as PR  # noqa: E402
import regions_ref as RR  # noqa: E402


def main():
    out = {}
    for name, (m, classes, background, connectivity) in PR.golden_cases().items():
        rows = PR.props_naive(m, classes, background, connectivity, records=RR.scipy_records)
        out[f"{name}.mask"] = m
        out[f"{name}.classes"] = np.asarray(classes, np.int32)
        out[f"{name}.params"] = np.asarray([background, connectivity], np.int32)
        out[f"{name}.props"] = rows
        measured = rows[rows[:, 14] >= 0]
        print(f"{name:18s} {m.shape} classes {classes} bg {background} conn {connectivity}: {len(rows)} regions, "
              f"{len(measured)} measured, skeleton pixels {int(measured[:, 15].sum())}, frame regions {int((rows[:, 13] > 0).sum())}")
    path = os.path.join(ROOT, "tests", "golden", "props", "props.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
