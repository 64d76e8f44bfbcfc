#!/usr/bin/env python3
"""Times vitseg_sdf (csrc/sdf.hip: both fields, normalised) with hipEvents -- the median of --iters calls after warm-up --
at 4 x 224^2, 32 x 224^2, 32 x 512^2 and 8 x 1024^2 on four mask kinds: empty, cracks (thin random polylines), blobs and
a checkerboard; and, where scipy is importable, the host compute_sdf (model/PAED/segmentation.py:6-34) per mask.

    python tools/sdf_probe.py [--iters 20] [--out profiles/<tag>_sdf.txt] [--no-host]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sdf_ref as R  # noqa: E402
from visiontransformer_amd import sdf  # noqa: E402

SHAPES = [(4, 224), (32, 224), (32, 512), (8, 1024)]
KINDS = ("empty", "cracks", "blobs", "checker")


def batch(kind, n, S):
    return np.stack([R.kind_mask(kind, 100 + i, S, S) for i in range(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--no-host", action="store_true", help="skip the scipy timing (e.g. under rocprofv3)")
    a = ap.parse_args()
    lines = [f"vitseg_sdf, both fields, normalize = 1; median of {a.iters} hipEvent-timed calls after 3 warm-up calls",
             f"{'batch':12s} {'kind':8s} {'us/call':>10s} {'us/mask':>10s} {'Mpix/s':>10s}"]
    for n, S in SHAPES:
        for kind in KINDS:
            m = torch.from_numpy(batch(kind, n, S)).cuda()
            for _ in range(3):
                sdf._launch(m, True)
            ts = []
            for _ in range(a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                sdf._launch(m, True)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3)
            us = float(np.median(ts))
            lines.append(f"{f'{n} x {S}^2':12s} {kind:8s} {us:10.1f} {us / n:10.2f} {n * S * S / us:10.0f}")
            print(lines[-1], flush=True)
    try:
        import scipy  # noqa: F401
        have_scipy = not a.no_host
    except ImportError:
        have_scipy = False
        lines.append("host: scipy not importable here, compute_sdf not timed")
    for S in (224, 512, 1024) if have_scipy else ():
        for kind in KINDS:
            m = R.kind_mask(kind, 100, S, S)
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                R.scipy_compute_sdf(m)
                ts.append((time.perf_counter() - t0) * 1e6)
            lines.append(f"host: compute_sdf (scipy), one {S}^2 {kind} mask: {float(np.median(ts)):.0f} us")
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
