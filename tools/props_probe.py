#!/usr/bin/env python3
"""Times vitseg_region_props (csrc/props.hip) with hipEvents at n = 32, 512 x 512, on the masks of tools/regions_probe.py
(blobs and uniform random masks of 2 and 17 classes, a checkerboard, a serpentine) plus one region that fills the frame;
4-connectivity, background 0, labels written; with no skeleton class (K = 0: the labelling plus the shape pass), with one and
with four.  Beside it vitseg_regions alone on the same batch, the four calls taking turns inside one loop so that drift hits
them alike; the spread (min .. max) stands beside every median.  When scipy is present, also the host's loop on one image:
scipy.ndimage.label per class + sum_labels of the coordinate grids + distance_transform_edt per skeleton class.

    python tools/props_probe.py [--iters 15] [--out profiles/<tag>_props.txt]"""
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
SKELETON_CLASSES = {0: [], 1: [1], 4: [1, 2, 3, 4]}


def inputs():
    rs = np.random.RandomState(0)
    yield "blobs", 2, R.blobs(1, S, S, 2, n=N)
    yield "blobs", 17, R.blobs(2, S, S, 17, n=N)
    yield "uniform", 2, rs.randint(0, 2, size=(N, S, S)).astype(np.uint8)
    yield "uniform", 17, rs.randint(0, 17, size=(N, S, S)).astype(np.uint8)
    yield "checkerboard", 2, np.broadcast_to(R.checkerboard(S, S), (N, S, S)).copy()
    yield "serpentine", 2, np.broadcast_to(R.serpentine(S, S), (N, S, S)).copy()
    yield "full frame", 1, np.ones((N, S, S), np.uint8)


def host_loop(m, classes):
    """The host's answer for one image: per class present, label + sums of the coordinate grids; per skeleton class the EDT."""
    from scipy import ndimage
    yy, xx = np.mgrid[:m.shape[0], :m.shape[1]].astype(np.float64)
    k = 0
    for c in np.unique(m):
        if c == 0:
            continue
        X = m == c
        lab, nf = ndimage.label(X)
        idx = np.arange(1, nf + 1)
        for g in (X, yy, xx, yy * yy, xx * xx, xx * yy):
            ndimage.sum_labels(g, lab, idx)
        if int(c) in classes:
            ndimage.maximum(ndimage.distance_transform_edt(X), lab, idx)
        k += nf
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=15)
    ap.add_argument("--out")
    ap.add_argument("--no-host", action="store_true", help="skip the scipy loop (e.g. under rocprofv3)")
    a = ap.parse_args()
    lines = [f"vitseg_region_props, n = {N}, {S} x {S}, connectivity 4, background 0, labels written, max_regions = the largest "
             f"count; milliseconds, median (min .. max) of {a.iters} hipEvent-timed calls, the calls of a row taking turns",
             f"{'input':14s} {'C':>3s} {'regions/img':>11s} {'vitseg_regions':>22s} {'props K=0':>22s} {'props K=1':>22s} "
             f"{'props K=4':>22s}"]
    for name, C, m in inputs():
        md = torch.from_numpy(m).cuda()
        counts, _, _ = regions._launch(md, 0, 4, 0, False)
        cap = int(counts.max())
        calls = {"regions": lambda: regions._launch(md, 0, 4, cap, True)}
        for K, cls in SKELETON_CLASSES.items():
            calls[K] = lambda cls=cls: regions._launch_props(md, cls, 0, 4, 0, cap, True)
        ts = {k: [] for k in calls}
        for it in range(a.iters + 2):
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f()
                e1.record()
                e1.synchronize()
                if it >= 2:   # two rounds of warm-up for every call
                    ts[k].append(e0.elapsed_time(e1))
        cell = lambda v: f"{np.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})".rjust(22)
        lines.append(f"{name:14s} {C:3d} {float(counts.float().mean()):11.0f} " + " ".join(cell(ts[k]) for k in calls))
        print(lines[-1], flush=True)
    try:
        from scipy import ndimage  # noqa: F401
        have_scipy = not a.no_host
    except ImportError:
        have_scipy = False
        lines.append("host: scipy not installed, the host loop was not timed")
    for C in ((2, 17) if have_scipy else ()):
        m = R.blobs(C, S, S, C)
        for K, cls in SKELETON_CLASSES.items():
            t0 = time.perf_counter()
            k = host_loop(m, cls)
            dt = (time.perf_counter() - t0) * 1e3
            lines.append(f"host: label + sum_labels per class, distance_transform_edt for {K} classes (no skeleton), one {S} x {S} "
                         f"blobs image of {C} classes, {k} regions: {dt:.1f} ms (x {N} for the batch: {dt * N / 1e3:.2f} s)")
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
