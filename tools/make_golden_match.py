#!/usr/bin/env python3
"""Writes tests/golden/match/match.npz: the maps of tests/match_ref.match_cases() and what vitseg_region_match
(include/vitseg.h) has to return for them, computed from the definitions alone -- tests/match_ref.match_naive, every
predicted region of a class against every true one through boolean masks -- on the labelling of the real scipy.ndimage.label
(regions_ref.scipy_records: one call per class present), independently of the numpy restatement's union-find and of its
sorted pair keys.  Needs scipy.
Keys: "<case>.pred", "<case>.gt" uint8 [n, H, W]; "<case>.classes" int32 [K]; "<case>.params" int32 [7] (connectivity,
background, ignore_label, thr_num, thr_den, cov_num, cov_den); "<case>.stats" int64 [n, K, 8]; "<case>.pred_table.<i>",
"<case>.gt_table.<i>" int32 [k, 3] per image: (first pixel, partner's first pixel or -1, covered pixels) of every listed region
by first pixel."""
import os
import sys

import numpy as np
from scipy import ndimage  # noqa: F401  (regions_ref.scipy_records imports it lazily: fail here, with a clear message)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import match_ref as M  # noqa: E402
import regions_ref as R  # noqa: E402


def main():
    out = {}
    for name, c in M.match_cases().items():
        kw = M.case_kwargs(c)
        stats, pinfo, ginfo = M.match_ref(c["pred"], c["gt"], c["classes"], form=M.match_naive, records=R.scipy_records, **kw)
        out[f"{name}.pred"], out[f"{name}.gt"] = c["pred"], c["gt"]
        out[f"{name}.classes"] = np.asarray(c["classes"], np.int32)
        out[f"{name}.params"] = np.asarray([c["connectivity"], c["background"], c["ignore_label"], *c["thr"], *c["cov"]], np.int32)
        out[f"{name}.stats"] = stats
        for i in range(len(stats)):
            out[f"{name}.pred_table.{i}"] = M.table(pinfo[i])
            out[f"{name}.gt_table.{i}"] = M.table(ginfo[i])
        tot = stats.sum(axis=(0, 1))
        print(f"{name:28s} {c['pred'].shape} K {len(c['classes']):2d} conn {c['connectivity']} thr {c['thr']} cov {c['cov']}: "
              + " ".join(f"{k}={int(v)}" for k, v in zip(M.STATS[:5], tot[:5])))
    path = os.path.join(ROOT, "tests", "golden", "match", "match.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
