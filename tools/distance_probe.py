#!/usr/bin/env python3
"""Times vitseg_distance_stats (csrc/distance.hip) with hipEvents -- the median of --iters calls after warm-up -- at
32 x 512^2 for 2 and 17 classes in both modes (sets, borders) at the 95th percentile; and, where scipy is importable, the
same statistics of one image taken with scipy on the host (distance_transform_edt + binary_erosion + sort: the loop of
tests/distance_ref.py), scaled to the batch.

    python tools/distance_probe.py [--iters 10] [--out profiles/<tag>_distance.txt] [--no-host]"""
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
import distance_ref as R  # noqa: E402
from visiontransformer_amd import _lib  # noqa: E402

N, S = 32, 512


def maps(num_classes):
    gt = np.stack([R.class_map(100 + i, S, S, num_classes) for i in range(N)])
    pred = np.stack([R.shifted(g, 3, -2) if i % 2 else R.class_map(200 + i, S, S, num_classes) for i, g in enumerate(gt)])
    return gt, pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--no-host", action="store_true", help="skip the scipy timing (e.g. under rocprofv3)")
    a = ap.parse_args()
    fn = _lib.symbol("vitseg_distance_stats")
    nbytes = _lib.symbol("vitseg_distance_scratch_bytes")(N, S, S)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    lines = [f"vitseg_distance_stats, {N} x {S}^2, percentile 95; median of {a.iters} hipEvent-timed calls after 2 warm-up calls; "
             f"scratch {nbytes / 2 ** 20:.0f} MiB",
             f"{'classes':>8s} {'mode':8s} {'ms/call':>10s} {'us/(image, class)':>18s}"]
    try:
        import scipy  # noqa: F401
        have_scipy = not a.no_host
    except ImportError:
        have_scipy = False
        lines.append("host: scipy not importable here, the host loop not timed")
    host = []
    for K in (2, 17):
        gt, pred = maps(K)
        g, p = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()
        si = torch.empty((N, K, 6), dtype=torch.int64, device="cuda")
        sf = torch.empty((N, K, 2), dtype=torch.float64, device="cuda")
        cls = (ctypes.c_int32 * K)(*range(K))
        st = torch.cuda.current_stream().cuda_stream
        for mode, mname in ((0, "sets"), (1, "borders")):
            call = lambda: _lib.check(fn(p.data_ptr(), g.data_ptr(), N, S, S, cls, K, mode, 19, 20, si.data_ptr(), sf.data_ptr(),
                                         scratch.data_ptr(), nbytes, st))
            for _ in range(2):
                call()
            ts = []
            for _ in range(a.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            ms = float(np.median(ts))
            lines.append(f"{K:8d} {mname:8s} {ms:10.2f} {ms * 1e3 / (N * K):18.1f}")
            print(lines[-1], flush=True)
            if have_scipy:
                t0 = time.perf_counter()
                R.stats_ref(gt[:1], pred[:1], list(range(K)), mode, 19, 20, route="scipy")
                dt = time.perf_counter() - t0
                host.append(f"host: scipy loop, one {S}^2 image, {K} classes, {mname}: {dt * 1e3:.0f} ms "
                            f"(x {N} images = {dt * N * 1e3:.0f} ms per batch)")
                print(host[-1], flush=True)
    lines += host
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
