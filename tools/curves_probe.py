#!/usr/bin/env python3
"""Times vitseg_pr_counts (csrc/curves.hip) with hipEvents at n = 32, 512 x 512, g = 32, C = 2 and 17, both score kinds, 256
bins, at a tolerance of 0, 2, 5 and 16 pixels, on three ground truths: the one-pixel centre-line of tools/centerlines_probe.py
and the blobs of tools/regions_probe.py (sparse), and a full frame of true pixels (the worst case for "found": every pixel
takes the disc maximum).  Beside it, in the same process and taking turns inside one loop so that drift hits them alike,
  floor  vitseg_confidence writing the quantised map on the same inputs: the same regeneration of the score, no dilation;
  hist   the confidence.calibration_hist launch with 256 bins: the tolerance-0 call does its work plus two more tables.
The spread (min .. max) stands beside every median.  The last lines say whether the tolerance-0 call stays within the
histogram's time plus twice its observed spread.

    python tools/curves_probe.py [--iters 20] [--out profiles/curves_probe.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import regions_ref as R  # noqa: E402
from centerlines_probe import thin_serpentine  # noqa: E402
from visiontransformer_amd import _ext, _lib, confidence  # noqa: E402

N, S, G, BINS = 32, 512, 32, 256
TOLERANCES = (0, 2, 5, 16)


def ground_truths(C):
    yield "centre-line", thin_serpentine()
    yield "blobs", (R.blobs(C, S, S, C, n=N) == 1).astype(np.uint8)
    yield "full frame", np.ones((N, S, S), np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = "cuda:0"
    fn = _ext.ext_symbol("curves", "vitseg_pr_counts")
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"vitseg_pr_counts, n = {N}, {S} x {S}, g = {G}, class 1, {BINS} bins; milliseconds on one MI355X, median (min .. max) "
             f"of {a.iters} hipEvent-timed calls taking turns; floor: vitseg_confidence writing the quantised map; hist: the "
             f"calibration histogram's launch at {BINS} bins",
             f"{'ground truth':12s} {'C':>3s} {'kind':>6s} {'true px':>9s} " + " ".join(
                 f"{w:>22s}" for w in ["floor", "hist"] + [f"tolerance {t}" for t in TOLERANCES])]
    over = []
    for C in (2, 17):
        z = torch.randn((N, C, G, G), generator=torch.Generator().manual_seed(C)).mul_(3.0).to(dev)
        stated = torch.ones((N, S, S), dtype=torch.uint8, device=dev)
        q = torch.empty((N, S, S), dtype=torch.uint16, device=dev)
        hist = torch.empty((N, BINS, 3), dtype=torch.int64, device=dev)
        counts = torch.empty((N, BINS, 3), dtype=torch.int64, device=dev)
        for name, m in ground_truths(C):
            gt = torch.from_numpy(m).to(dev)
            for kind in ("prob", "margin"):
                def curve(tol):
                    _lib.check(fn(z.data_ptr(), gt.data_ptr(), N, C, G, S, 1, confidence.KINDS[kind], BINS, tol * tol, -1,
                                  counts.data_ptr(), None, 0, stream))
                calls = {"floor": lambda: confidence._launch(z, stated, kind, conf_q=q),
                         "hist": lambda: confidence._launch(z, stated, kind, gt=gt, hist=hist)}
                calls.update({f"tol{t}": (lambda t=t: curve(t)) for t in TOLERANCES})
                # the calls agree on what they count: every pixel once, every true pixel once
                curve(TOLERANCES[-1])
                calls["hist"]()
                assert int(counts[..., 0].sum()) == N * S * S == int(hist[..., 0].sum()) and int(counts[..., 2].sum()) == int(m.sum())
                assert torch.equal(counts[..., 0], hist[..., 0])
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
                cell = lambda v: f"{np.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})".rjust(22)
                lines.append(f"{name:12s} {C:3d} {kind:>6s} {int(m.sum()) // N:9d} " + " ".join(cell(v) for v in ts.values()))
                print(lines[-1], flush=True)
                bound = float(np.median(ts["hist"])) + 2.0 * (max(ts["hist"]) - min(ts["hist"]))
                if float(np.median(ts["tol0"])) > bound:
                    over.append(f"{name} C={C} {kind}: {np.median(ts['tol0']):.3f} vs {bound:.3f} ms")
    lines.append("tolerance 0 within the histogram's time plus twice its spread in every cell" if not over else
                 "tolerance 0 ABOVE the histogram's time plus twice its spread: " + "; ".join(over))
    print(lines[0] + "\n" + lines[1] + "\n" + lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
