#!/usr/bin/env python3
"""Times vitseg_region_polygons (csrc/polygons.hip) with hipEvents at n = 32, 512 x 512, on the masks of
tools/regions_probe.py (blobs, uniform random, checkerboard, serpentine), 4-connectivity, background 0, capacities at the true
counts, beside vitseg_regions alone on the same masks.  The host answers (cv2.findContours, skimage.measure.find_contours) are
not installed where this runs, so there is no host baseline: none is invented.

    python tools/polygons_probe.py [--iters 20] [--out profiles/<tag>_polygons.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from regions_probe import N, S, inputs  # noqa: E402
from visiontransformer_amd import _ext, _lib, polygons, regions  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    fn = _ext.ext_symbol("polygons", "vitseg_region_polygons")
    nbytes = _ext.ext_symbol("polygons", "vitseg_region_polygons_scratch_bytes")(N, S, S)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"vitseg_region_polygons, n = {N}, {S} x {S}, connectivity 4, background 0, labels written, capacities at the "
             f"largest counts; median of {a.iters} hipEvent-timed calls; beside it vitseg_regions alone (tools/regions_probe.py); "
             f"scratch {nbytes / 2**20:.0f} MiB"]
    lines.append(f"{'input':14s} {'C':>3s} {'rings/img':>10s} {'vertices/img':>13s} {'polygons us':>12s} {'regions us':>11s} {'ratio':>6s}")
    for name, C, m in inputs():
        md = torch.from_numpy(m).cuda()
        counts = polygons._launch(md, 0, 4, 0, 0, False)[0].cpu().numpy()
        max_rings, max_vertices = int(counts[N:2 * N].max()), int(counts[2 * N:].view(np.int64).max())
        cnt = torch.empty(4 * N, dtype=torch.int32, device="cuda")
        rings = torch.empty((N, max_rings, 4), dtype=torch.int64, device="cuda")
        vertices = torch.empty((N, max_vertices, 2), dtype=torch.int32, device="cuda")
        labels = torch.empty((N, S, S), dtype=torch.int32, device="cuda")

        def call():
            _lib.check(fn(md.data_ptr(), N, S, S, 4, 0, cnt.data_ptr(), cnt[N:].data_ptr(), cnt[2 * N:].data_ptr(), rings.data_ptr(),
                          max_rings, vertices.data_ptr(), max_vertices, labels.data_ptr(), scratch.data_ptr(), nbytes, stream))
        us = timed(call, a.iters)
        cap = int(counts[:N].max())
        base = timed(lambda: regions._launch(md, 0, 4, cap, True), a.iters)
        lines.append(f"{name:14s} {C:3d} {counts[N:2 * N].mean():10.0f} {counts[2 * N:].view(np.int64).mean():13.0f} {us:12.1f} "
                     f"{base:11.1f} {us / base:6.1f}")
        print(lines[-1], flush=True)
        del rings, vertices, labels
    lines.append("host: neither cv2 nor skimage is installed here; no host contour baseline was timed")
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
