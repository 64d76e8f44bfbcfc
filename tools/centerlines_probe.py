#!/usr/bin/env python3
"""Times vitseg_centerlines (csrc/centerlines.hip) with hipEvents at n = 32, 512 x 512, thin = 1 on the masks of
tools/regions_probe.py (blobs, uniform random, checkerboard, serpentine) read as binary, and thin = 0 on a one-pixel-wide
serpentine (the longest chain: the most pointer-jumping rounds), capacities at the true counts, beside vitseg_skeleton alone
on the same masks: the difference is what the tracing adds.  No host tracer (skan) is installed where this runs, so there is
no host baseline: none is invented.

    python tools/centerlines_probe.py [--iters 20] [--out profiles/<tag>_centerlines.txt]"""
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
from visiontransformer_amd import _ext, _lib, centerlines, skeleton  # noqa: E402


def thin_serpentine():
    """Full rows every second row, joined at alternating ends: one chain through half the image."""
    m = np.zeros((S, S), np.uint8)
    for k, y in enumerate(range(0, S, 2)):
        m[y, :] = 1
        if y + 2 < S:
            m[y:y + 3, S - 1 if k % 2 == 0 else 0] = 1
    return np.repeat(m[None], N, axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    fn = _ext.ext_symbol("centerlines", "vitseg_centerlines")
    nbytes = _ext.ext_symbol("centerlines", "vitseg_centerlines_scratch_bytes")(N, S, S, 0)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"vitseg_centerlines, n = {N}, {S} x {S}, value -1, route 0, capacities at the largest counts; median of {a.iters} "
             f"hipEvent-timed calls; beside it vitseg_skeleton alone (thin = 1) on the same masks; scratch {nbytes / 2**20:.0f} MiB"]
    lines.append(f"{'input':18s} {'thin':>4s} {'nodes/img':>10s} {'branches/img':>13s} {'points/img':>11s} {'centerlines us':>15s} "
                 f"{'skeleton us':>12s} {'added us':>9s}")
    cases = [(name, 1, m) for name, C, m in inputs() if C == 2] + [("thin serpentine", 0, thin_serpentine())]
    for name, thin, m in cases:
        md = torch.from_numpy((m != 0).astype(np.uint8)).cuda()
        counts = centerlines._launch(md, -1, bool(thin), 0, 0, 0, 0)[0].cpu().numpy()
        nodes_n, branches_n, points_n = counts[:N], counts[N:2 * N], counts[2 * N:].view(np.int64)
        caps = (max(int(nodes_n.max()), 1), max(int(branches_n.max()), 1), max(int(points_n.max()), 1))
        cnt = torch.empty(4 * N, dtype=torch.int32, device="cuda")
        nodes = torch.empty((N, caps[0], 4), dtype=torch.int32, device="cuda")
        branches = torch.empty((N, caps[1], 9), dtype=torch.int64, device="cuda")
        points = torch.empty((N, caps[2], 3), dtype=torch.int32, device="cuda")

        def call():
            _lib.check(fn(md.data_ptr(), N, S, S, -1, thin, 0, cnt.data_ptr(), cnt[N:].data_ptr(), cnt[2 * N:].data_ptr(),
                          nodes.data_ptr(), caps[0], branches.data_ptr(), caps[1], points.data_ptr(), caps[2], scratch.data_ptr(),
                          nbytes, stream))
        us = timed(call, a.iters)
        base = timed(lambda: skeleton._launch(md, 0, False), a.iters) if thin else 0.0
        lines.append(f"{name:18s} {thin:4d} {nodes_n.mean():10.0f} {branches_n.mean():13.0f} {points_n.mean():11.0f} {us:15.1f} "
                     f"{base:12.1f} {us - base:9.1f}")
        print(lines[-1], flush=True)
        del nodes, branches, points
    lines.append("host: skan is not installed here; no host tracing baseline was timed")
    print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
