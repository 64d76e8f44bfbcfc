#!/usr/bin/env python3
"""Times vitseg_skeleton and vitseg_skeleton_stats (csrc/skeleton.hip) with hipEvents -- the median of --iters calls after
warm-up -- at 32 x 512^2 (resident route) on crack-like, blob and full-plane masks, at 4 x 1024^2 on the resident route and
at 2 x 2048^2 on the global one; the statistics at 32 x 512^2 for 2 and 17 classes; and, next to them, the time of the
per-pixel numpy restatement (tests/skeleton_ref.py) for one image on this box, scaled to the batch (skipped for masks that
take more than 64 passes).

    python tools/skeleton_probe.py [--iters 5] [--out profiles/<tag>_skeleton.txt] [--no-host]"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import skeleton_ref as R  # noqa: E402
from visiontransformer_amd import _lib  # noqa: E402

ROUTE_NAMES = {1: "resident", 2: "global"}


def masks(kind, n, S):
    if kind == "crack":
        return np.stack([R.crack(S, S, i, 1 + i % 2) for i in range(n)])
    if kind == "blobs":
        return np.stack([R.blobs(S, S, i) for i in range(n)])
    return np.ones((n, S, S), np.uint8)


def class_maps(n, S, K, seed):
    """Class 0 the background, classes 1 .. K - 1 crack bands drawn over each other."""
    out = np.zeros((n, S, S), np.uint8)
    for i in range(n):
        for c in range(1, K):
            out[i][R.crack(S, S, seed + 31 * i + c, 1 + c % 2) == 1] = c
    return out


def timed(call, iters):
    call()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy timing (e.g. under rocprofv3)")
    a = ap.parse_args()
    fn = _lib.symbol("vitseg_skeleton")
    size = _lib.symbol("vitseg_skeleton_scratch_bytes")
    st = torch.cuda.current_stream().cuda_stream
    lines = [f"vitseg_skeleton; median of {a.iters} hipEvent-timed calls after 1 warm-up call",
             f"{'n x S^2':>12s} {'mask':6s} {'route':9s} {'passes min..max':>16s} {'ms/call':>10s} {'us/image':>10s} {'numpy ms/image':>15s}"]
    print("\n".join(lines), flush=True)
    for n, S, route, kinds in [(32, 512, 1, ("crack", "blobs", "full")), (32, 512, 2, ("crack", "blobs", "full")),
                               (4, 1024, 1, ("crack", "blobs", "full")), (2, 2048, 2, ("crack", "blobs", "full"))]:
        nbytes = size(n, S, S, route)
        if nbytes == 0:
            lines.append(f"{n:4d} x {S:4d}^2: the {ROUTE_NAMES[route]} route does not take this plane on this device")
            print(lines[-1], flush=True)
            continue
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        out = torch.empty((n, S, S), dtype=torch.uint8, device="cuda")
        passes = torch.empty(n, dtype=torch.int32, device="cuda")
        for kind in kinds:
            m_host = masks(kind, n, S)
            m = torch.from_numpy(m_host).cuda()
            call = lambda: _lib.check(fn(m.data_ptr(), n, S, S, route, out.data_ptr(), passes.data_ptr(), scratch.data_ptr(),
                                         nbytes, st))
            ms = timed(call, a.iters)
            p = passes.cpu().numpy()
            host = ""
            if not a.no_host and p.max() <= 64:
                t0 = time.perf_counter()
                ref, rp = R.skeleton_one(m_host[0])
                host = f"{(time.perf_counter() - t0) * 1e3:.0f}"
                assert rp == p[0] and np.array_equal(ref, out[0].cpu().numpy()), (kind, S, route)
            lines.append(f"{n:4d} x {S:4d}^2 {kind:6s} {ROUTE_NAMES[route]:9s} {f'{p.min()}..{p.max()}':>16s} {ms:10.3f} "
                         f"{ms * 1e3 / n:10.1f} {host:>15s}")
            print(lines[-1], flush=True)
    fs = _lib.symbol("vitseg_skeleton_stats")
    N, S = 32, 512
    lines.append(f"vitseg_skeleton_stats, {N} x {S}^2, classes 0 (background) .. K - 1 (crack bands); automatic route")
    lines.append(f"{'classes':>8s} {'ms/call':>10s} {'us/(image, class)':>18s} {'numpy ms/image':>15s}")
    print("\n".join(lines[-2:]), flush=True)
    nbytes = _lib.symbol("vitseg_skeleton_stats_scratch_bytes")(N, S, S, 0)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    for K in (2, 17):
        gt, pred = class_maps(N, S, K, 1000), class_maps(N, S, K, 2000)
        g, p = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()
        si = torch.empty((N, K, 10), dtype=torch.int64, device="cuda")
        sf = torch.empty((N, K, 2), dtype=torch.float64, device="cuda")
        cls = (ctypes.c_int32 * K)(*range(K))
        call = lambda: _lib.check(fs(p.data_ptr(), g.data_ptr(), N, S, S, cls, K, 0, si.data_ptr(), sf.data_ptr(),
                                     scratch.data_ptr(), nbytes, st))
        ms = timed(call, a.iters)
        host = ""
        if not a.no_host:   # the crack classes alone: the restatement needs minutes for the background's hundreds of passes
            t0 = time.perf_counter()
            ei, _ = R.stats_ref(gt[:1], pred[:1], list(range(1, K)))
            host = f"{(time.perf_counter() - t0) * 1e3:.0f} (classes 1..{K - 1})"
            assert np.array_equal(ei[0], si[0, 1:].cpu().numpy()), K
        lines.append(f"{K:8d} {ms:10.2f} {ms * 1e3 / (N * K):18.1f} {host:>15s}")
        print(lines[-1], flush=True)
    lines.append(f"scratch of the statistics: {nbytes / 2 ** 20:.0f} MiB")
    print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
