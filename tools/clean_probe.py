#!/usr/bin/env python3
"""Times vitseg_clean_mask (csrc/clean.hip) with hipEvents at n = 32, 512 x 512 on speckled-blob masks of 2 and 17 classes
(tests/clean_ref.speckle), 4-connectivity, background 0: min_area alone, fill_holes alone and both, beside vitseg_regions
with labels written on the same masks in the same process, the calls taken in turn so that all four see the same machine.
When scipy is present, also the host loop the clean-up replaces, once per mask set: the copy back, then per image and class
scipy.ndimage.label + bincount, then binary_fill_holes per class.

    python tools/clean_probe.py [--iters 30] [--min-area 8] [--out profiles/clean_probe.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clean_ref as K  # noqa: E402
from visiontransformer_amd import _lib, regions  # noqa: E402

N, S = 32, 512


def clean_call(md, min_area, fill_holes):
    """One enqueue-only vitseg_clean_mask call with statistics on preallocated buffers: () -> None."""
    n, H, W = md.shape
    out = torch.empty_like(md)
    stats = torch.empty((n, 8), dtype=torch.int32, device=md.device)
    scratch = torch.empty(_lib.symbol("vitseg_clean_scratch_bytes")(n, H, W), dtype=torch.uint8, device=md.device)
    f = _lib.symbol("vitseg_clean_mask")
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        _lib.check(f(md.data_ptr(), out.data_ptr(), n, H, W, 4, 0, min_area, int(fill_holes), 0, stats.data_ptr(),
                     scratch.data_ptr(), scratch.numel(), stream))
    return call, stats


def regions_call(md):
    n, H, W = md.shape
    counts, _, _ = regions._launch(md, 0, 4, 0, False)
    cap = int(counts.max())
    scratch = torch.empty(_lib.symbol("vitseg_regions_scratch_bytes")(n, H, W), dtype=torch.uint8, device=md.device)
    recs = torch.empty((n, cap, 8), dtype=torch.int32, device=md.device)
    labels = torch.empty((n, H, W), dtype=torch.int32, device=md.device)
    f = _lib.symbol("vitseg_regions")
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        _lib.check(f(md.data_ptr(), n, H, W, 4, 0, counts.data_ptr(), recs.data_ptr(), cap, labels.data_ptr(),
                     scratch.data_ptr(), scratch.numel(), stream))
    return call, float(counts.float().mean())


def timed(call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3


def host_loop(md, min_area):
    """The host answer, timed from the device mask to the cleaned host mask: seconds for the batch."""
    from scipy import ndimage
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = md.cpu().numpy()
    out = m.copy()
    for i in range(len(m)):
        for c in np.unique(m[i]):
            if c == 0:
                continue
            lab, nf = ndimage.label(m[i] == c)
            small = np.bincount(lab.reshape(-1), minlength=nf + 1) < min_area
            small[0] = False
            out[i][small[lab]] = 0
        for c in np.unique(out[i]):
            if c == 0:
                continue
            filled = ndimage.binary_fill_holes(out[i] == c)
            out[i][filled & (out[i] == 0)] = c
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--min-area", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clean_probe.json"))
    ap.add_argument("--no-host", action="store_true", help="skip the scipy loop")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the GPU"
    result = dict(n=N, size=S, iters=a.iters, min_area=a.min_area, connectivity=4, background=0, device=torch.cuda.get_device_name(0),
                  note="us per call, median [min, max] of hipEvent-timed calls taken in turn; ratio = median over "
                       "vitseg_regions' (labels written, no truncation) on the same masks", rows=[])
    print(f"{'C':>3s} {'call':28s} {'us median':>10s} {'min':>9s} {'max':>9s} {'x regions':>9s} {'Mpix/s':>9s}")
    for C in (2, 17):
        md = torch.from_numpy(K.speckle(40 + C, S, S, C, n=N)).cuda()
        reg, per_image = regions_call(md)
        calls = {"vitseg_regions + labels": reg}
        stats = {}
        for name, ma, fh in (("clean: min_area", a.min_area, False), ("clean: fill_holes", 0, True),
                             ("clean: min_area + fill_holes", a.min_area, True)):
            calls[name], stats[name] = clean_call(md, ma, fh)
        for _ in range(5):
            for c in calls.values():
                c()
        torch.cuda.synchronize()
        ts = {k: [] for k in calls}
        for _ in range(a.iters):
            for k, c in calls.items():
                ts[k].append(timed(c))
        base = float(np.median(ts["vitseg_regions + labels"]))
        for k, v in ts.items():
            med = float(np.median(v))
            row = dict(classes=C, call=k, us_median=round(med, 1), us_min=round(min(v), 1), us_max=round(max(v), 1),
                       ratio_to_regions=round(med / base, 3), mpix_per_s=round(N * S * S / med))
            if k in stats:
                row["stats_mean_per_image"] = dict(zip(_lib.CLEAN_STATS, stats[k][:, :6].float().mean(0).tolist()))
            else:
                row["regions_per_image"] = per_image
            result["rows"].append(row)
            print(f"{C:3d} {k:28s} {med:10.1f} {min(v):9.1f} {max(v):9.1f} {med / base:9.2f} {N * S * S / med:9.0f}", flush=True)
        try:
            import scipy  # noqa: F401
            have = not a.no_host
        except ImportError:
            have = False
            result.setdefault("host_note", "scipy not installed: the host loop was not timed")
        if have:
            sec = host_loop(md, a.min_area)
            both = float(np.median(ts["clean: min_area + fill_holes"]))
            result["rows"].append(dict(classes=C, call="host: copy back + scipy label / bincount / binary_fill_holes per class",
                                       us_median=round(sec * 1e6), ratio_to_device_clean=round(sec * 1e6 / both)))
            print(f"{C:3d} host loop (copy back + scipy per class): {sec * 1e3:.0f} ms for the batch, "
                  f"{sec * 1e6 / both:.0f} x the device call", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(a.out)


if __name__ == "__main__":
    main()
