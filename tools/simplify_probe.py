#!/usr/bin/env python3
"""Times vitseg_simplify_lines (csrc/simplify.hip) with hipEvents at n = 32, 512 x 512 on the rings of tools/polygons_probe.py's
masks and the branches of tools/centerlines_probe.py's masks, plus decreasing sawtooth lines (a round per tooth: the deepest
recursion a line can have), at the tolerances 0.75 and 2.0 px -- the simplification alone, beside vitseg_region_polygons /
vitseg_centerlines alone on the same masks -- with the points before -> after and the bytes copied back before -> after.
The time of each length class (wave: <= SHORT points, resident: <= RESIDENT, long) is that of the same call with the counts
of the other classes' lines set to 0 on the device, so that only that class's lines do any work.  The host answers
(cv2.approxPolyDP, shapely, skimage.measure.approximate_polygon) are not installed where this runs, so there is no host
baseline: none is invented.

    python tools/simplify_probe.py [--iters 10] [--out profiles/simplify_probe.txt]"""
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
from polygons_probe import timed  # noqa: E402
from centerlines_probe import thin_serpentine  # noqa: E402
from visiontransformer_amd import _ext, _lib, centerlines, polygons, simplify  # noqa: E402

TOLERANCES = (0.75, 2.0)
SHORT, RESIDENT = simplify.SHORT, simplify.RESIDENT


def sawtooth(count):
    """Teeth whose height shrinks from left to right: every base's winner is its leftmost point but one."""
    k = np.arange(count)
    return np.stack([np.where(k % 2 == 1, (count - k) + 4, 0), 2 * k], axis=1).astype(np.int32)


def outlines(md):
    counts = polygons._launch(md, 0, 4, 0, 0, False)[0].cpu().numpy()
    caps = (max(int(counts[N:2 * N].max()), 1), max(int(counts[2 * N:].view(np.int64).max()), 1))
    run = lambda: polygons._launch(md, 0, 4, caps[0], caps[1], False)
    cnt, rings, vertices, _, _ = run()
    return run, vertices, rings, cnt[N:2 * N].contiguous(), simplify.RING_COLS, 32   # bytes per row copied back today


def branches(md, thin):
    counts = centerlines._launch(md, -1, bool(thin), 0, 0, 0, 0)[0].cpu().numpy()
    caps = (max(int(counts[:N].max()), 1), max(int(counts[N:2 * N].max()), 1), max(int(counts[2 * N:].view(np.int64).max()), 1))
    run = lambda: centerlines._launch(md, -1, bool(thin), 0, *caps)
    cnt, _, rows, points = run()
    return run, points, rows, cnt[N:2 * N].contiguous(), simplify.BRANCH_COLS, 72


def teeth(count, per_image):
    pts = torch.from_numpy(np.tile(sawtooth(count), (N, per_image, 1))).cuda()
    rows = torch.tensor([[k * count, count, 0] for k in range(per_image)], dtype=torch.int64).repeat(N, 1, 1).cuda()
    return None, pts, rows, torch.full((N,), per_image, dtype=torch.int32, device="cuda"), (0, 1, 2), 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = [f"vitseg_simplify_lines, n = {N}, {S} x {S}, SHORT = {SHORT}, RESIDENT = {RESIDENT}, output capacity = input capacity; median "
             f"of {a.iters} hipEvent-timed calls, us; `tracing`: vitseg_region_polygons (rings) / vitseg_centerlines (branches) "
             f"alone on the same masks; wave / resident / long: the call with only that class's lines; bytes: what is copied to "
             f"the host per batch without -> with the simplification"]
    lines.append(f"{'input':24s} {'tol':>5s} {'lines/img':>10s} {'w/r/l % of points':>18s} {'points/img':>11s} {'kept/img':>9s} "
                 f"{'tracing':>9s} {'simplify':>9s} {'wave':>8s} {'resident':>9s} {'long':>9s} {'MB before':>10s} {'MB after':>9s}")
    cases = [(f"rings {name} C={C}", lambda m=m: outlines(torch.from_numpy(m).cuda())) for name, C, m in inputs()]
    cases += [(f"branches {name}", lambda m=m: branches(torch.from_numpy((m != 0).astype(np.uint8)).cuda(), 1))
              for name, C, m in inputs() if C == 2]
    cases += [("branches thin serpentine", lambda: branches(torch.from_numpy(thin_serpentine()).cuda(), 0)),
              (f"sawtooth {RESIDENT - 48} x 8", lambda: teeth(RESIDENT - 48, 8)), ("sawtooth 5000 x 8", lambda: teeth(5000, 8))]
    for name, make in cases:
        run, pts, rows, cnt, cols, row_bytes = make()
        tracing = timed(run, a.iters) if run is not None else float("nan")
        length = rows[:, :, cols[1]]
        live = torch.arange(rows.shape[1], device="cuda")[None] < cnt[:, None]
        total = float((length * live).sum())
        share, only = [], []
        for lo, hi in ((0, SHORT), (SHORT, RESIDENT), (RESIDENT, 1 << 40)):
            sel = (length > lo) & (length <= hi)
            share.append(100.0 * float((length * (sel & live)).sum()) / max(total, 1.0))
            r = rows.clone()
            r[:, :, cols[1]] = torch.where(sel, length, torch.zeros_like(length))
            only.append(r)
        for tol in TOLERANCES:
            out = simplify.simplify_device(pts, rows, cnt, cols, tol)
            kept = out[0].cpu().numpy()
            us = timed(lambda: simplify.simplify_device(pts, rows, cnt, cols, tol), a.iters)
            per = [timed(lambda r=r: simplify.simplify_device(pts, r, cnt, cols, tol), a.iters) if s > 0 else 0.0
                   for r, s in zip(only, share)]
            before = (int(cnt.sum()) * row_bytes + total * pts.shape[2] * 4) / 1e6
            after = (int(cnt.sum()) * (row_bytes + 64) + float(kept.sum()) * pts.shape[2] * 4 + 8 * N) / 1e6
            lines.append(f"{name:24s} {tol:5.2f} {float(cnt.float().mean()):10.0f} {share[0]:5.0f}/{share[1]:5.0f}/{share[2]:5.0f}  "
                         f"{total / N:11.0f} {kept.mean():9.0f} {tracing:9.1f} {us:9.1f} {per[0]:8.1f} {per[1]:9.1f} {per[2]:9.1f} "
                         f"{before:10.2f} {after:9.2f}")
            print(lines[-1], flush=True)
        del pts, rows, only
    lines.append("the simplify column includes the allocation of outputs and scratch by simplify_device (torch's caching allocator) "
                 "and the memsets; a class column is a whole call, so the three do not add up to the first")
    lines.append("host: neither cv2, shapely nor skimage is installed here; no host simplification baseline was timed")
    print("\n".join(lines[-2:]))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
