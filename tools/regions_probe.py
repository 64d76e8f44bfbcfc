#!/usr/bin/env python3
"""Times vitseg_regions (csrc/regions.hip) with hipEvents at n = 32, 512 x 512, on blobs and uniform random masks of 2
and 17 classes, a checkerboard and a serpentine (2 classes by construction), 4-connectivity, background 0, labels
written; and, when scipy is present, the reference's per-class scipy loop (testViTModel.py:34-42,171-185) on one image.

    python tools/regions_probe.py [--iters 20] [--out profiles/<tag>_regions.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import regions_ref as R  # noqa: E402
from visiontransformer_amd import regions  # noqa: E402

N, S = 32, 512


def inputs():
    rs = np.random.RandomState(0)
    yield "blobs", 2, R.blobs(1, S, S, 2, n=N)
    yield "blobs", 17, R.blobs(2, S, S, 17, n=N)
    yield "uniform", 2, rs.randint(0, 2, size=(N, S, S)).astype(np.uint8)
    yield "uniform", 17, rs.randint(0, 17, size=(N, S, S)).astype(np.uint8)
    yield "checkerboard", 2, np.broadcast_to(R.checkerboard(S, S), (N, S, S)).copy()
    yield "serpentine", 2, np.broadcast_to(R.serpentine(S, S), (N, S, S)).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out")
    ap.add_argument("--no-host", action="store_true", help="skip the scipy loop (e.g. under rocprofv3)")
    a = ap.parse_args()
    lines = [f"vitseg_regions, n = {N}, {S} x {S}, connectivity 4, background 0, labels written; "
             f"median of {a.iters} hipEvent-timed calls (max_regions = the largest count: no truncation)"]
    lines.append(f"{'input':14s} {'C':>3s} {'regions/img':>12s} {'us':>10s} {'Mpix/s':>10s}")
    for name, C, m in inputs():
        md = torch.from_numpy(m).cuda()
        counts, _, _ = regions._launch(md, 0, 4, 0, False)
        cap = int(counts.max())
        for _ in range(3):
            regions._launch(md, 0, 4, cap, True)
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            regions._launch(md, 0, 4, cap, True)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        us = float(np.median(ts))
        lines.append(f"{name:14s} {C:3d} {float(counts.float().mean()):12.0f} {us:10.1f} {N * S * S / us:10.0f}")
        print(lines[-1], flush=True)
    try:
        from scipy import ndimage  # noqa: F401
        have_scipy = not a.no_host
    except ImportError:
        have_scipy = False
        lines.append("host: scipy not installed, the reference's loop was not timed")
    for C in ((2, 17) if have_scipy else ()):
        m = R.blobs(C, S, S, C)
        t0 = time.perf_counter()
        k = len(R.scipy_records(m, 0, 4)[0])
        dt = (time.perf_counter() - t0) * 1e6
        lines.append(f"host: the reference's loop (scipy.ndimage.label per class + np.argwhere per label), one {S} x {S} "
                     f"blobs image of {C} classes, {k} regions: {dt:.0f} us (x {N} for the batch: {dt * N / 1e6:.1f} s)")
        print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
