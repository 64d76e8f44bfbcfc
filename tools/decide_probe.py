#!/usr/bin/env python3
"""Times vitseg_decide (csrc/decide.hip) with hipEvents at n = 32, 512 x 512, for C = 2 with the "prob" score and C = 17 with the
"margin": the plain cut and the hysteresis call at connectivity 4 and 8, on three score planes:
  blobs       a smooth random head output at g = 32: blobs of weak pixels, some with a strong core;
  noise       full-size logits (g == S) of independent noise: single-pixel speckle, the most components;
              both cut at 0.4 / 0.6 for "prob"; the margin of one class among 17 is 0 on most pixels, so there the cuts are the
              30 % and 70 % points of the positive scores;
  full frame  a flat head output at g = 32 with one peak per image, low_q = 0 and high_q at the peak's score: every pixel weak,
              one component per image, kept by the few strong pixels at the peak.
Beside it, in the same process and taking turns inside one loop so that drift hits them alike,
  map      vitseg_confidence writing the quantised 16-bit map on the same inputs: the same regeneration of the score;
  regions  vitseg_regions alone (its six launches, three of them the labelling the hysteresis call runs) on the mask that call
           kept, at the same connectivity.
The spread (min .. max) stands beside every median.  The last lines compare the plain cut with the map's time plus its spread
and each hysteresis call with map + regions.

    python tools/decide_probe.py [--iters 20] [--out profiles/decide_probe.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visiontransformer_amd import _ext, _lib, confidence, decide  # noqa: E402

N, S, G = 32, 512, 32


def as_int(q16):
    """a uint16 device tensor as int32"""
    return q16.view(torch.int16).to(torch.int32) & 0xFFFF


def score_map(z, cls, kind):
    dev = z.device
    return as_int(confidence.confidence_map(z, torch.full((N, S, S), cls, dtype=torch.uint8, device=dev), kind=kind, quantised=True))


def planes(C, cls, kind, dev):
    """(name, lowres, high_q, low_q) per score plane"""
    gen = torch.Generator().manual_seed(C)
    for name, g in (("blobs", G), ("noise", S)):
        z = torch.randn((N, C, g, g), generator=gen).mul_(3.0).to(dev)
        hq, lq = decide.threshold_to_q(0.6), decide.threshold_to_q(0.4)
        if kind == "margin":
            q = score_map(z, cls, kind)
            pos = q[q > 0][::97].float()   # (a sample: torch.quantile takes at most 2^24 values)
            lq, hq = int(torch.quantile(pos, 0.3)), int(torch.quantile(pos, 0.7))
        yield name, z, hq, lq
    z = torch.zeros((N, C, G, G))
    z[:, cls, 5, 7] = 3.0
    z = z.to(dev)
    yield "full frame", z, int(score_map(z, cls, kind).max()), 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = "cuda:0"
    fn = _ext.ext_symbol("decide", "vitseg_decide")
    regions = _lib.symbol("vitseg_regions")
    stream = torch.cuda.current_stream().cuda_stream
    names = ["map", "plain cut", "hysteresis 4", "regions 4", "hysteresis 8", "regions 8"]
    lines = [f"vitseg_decide, n = {N}, {S} x {S}, g = {G} (noise: g = {S}); milliseconds on one MI355X, median (min .. max) of "
             f"{a.iters} hipEvent-timed calls taking turns; map: vitseg_confidence writing the quantised map; regions: "
             f"vitseg_regions alone on the mask the hysteresis call beside it kept",
             f"{'plane':10s} {'C':>3s} {'kind':>6s} {'low_q':>6s} {'high_q':>6s} {'weak px':>8s} {'strong':>8s} {'kept 4':>8s} {'kept 8':>8s} " + " ".join(
                 f"{w:>22s}" for w in names)]
    notes = []
    nbytes = _ext.ext_symbol("decide", "vitseg_decide_scratch_bytes")(N, S, 1)
    rbytes = _lib.symbol("vitseg_regions_scratch_bytes")(N, S, S)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    mask = torch.empty((N, S, S), dtype=torch.uint8, device=dev)
    kept4 = torch.empty((N, S, S), dtype=torch.uint8, device=dev)
    kept8 = torch.empty((N, S, S), dtype=torch.uint8, device=dev)
    counts = torch.empty((N, 3), dtype=torch.int64, device=dev)
    rcounts = torch.empty((N,), dtype=torch.int32, device=dev)
    qmap = torch.empty((N, S, S), dtype=torch.uint16, device=dev)
    for C, cls, kind in ((2, 1, "prob"), (17, 1, "margin")):
        stated = torch.full((N, S, S), cls, dtype=torch.uint8, device=dev)
        for name, z, hq, lq in planes(C, cls, kind, dev):
            g = int(z.shape[-1])

            def cut(high, low, conn, out=mask):
                _lib.check(fn(z.data_ptr(), N, C, g, S, cls, confidence.KINDS[kind], high, low, conn, None, 1, 0, out.data_ptr(),
                              counts.data_ptr(), scratch.data_ptr(), nbytes, stream))
            # the calls agree with one another: the counts are those of the map, the kept pixels those of the mask
            confidence._launch(z, stated, kind, conf_q=qmap)
            q = as_int(qmap)
            cut(hq, lq, 8, kept8)
            c8 = counts.sum(dim=0).tolist()
            assert c8[2] == int((kept8 == 1).sum())
            cut(hq, lq, 4, kept4)
            c4 = counts.sum(dim=0).tolist()
            assert c4[:2] == c8[:2] == [int((q >= lq).sum()), int((q >= hq).sum())] and c4[1] <= c4[2] <= c8[2] <= c4[0]
            assert c4[2] == int((kept4 == 1).sum())
            cut(hq, hq, 4)
            assert torch.equal(mask == 1, q >= hq) and counts.sum(dim=0).tolist() == [c4[1]] * 3
            def label(kept, conn):
                _lib.check(regions(kept.data_ptr(), N, S, S, conn, 0, rcounts.data_ptr(), None, 0, None, scratch.data_ptr(), rbytes,
                                   stream))
            calls = {"map": lambda: confidence._launch(z, stated, kind, conf_q=qmap),
                     "plain cut": lambda: cut(hq, hq, 4),
                     "hysteresis 4": lambda: cut(hq, lq, 4),
                     "regions 4": lambda: label(kept4, 4),
                     "hysteresis 8": lambda: cut(hq, lq, 8),
                     "regions 8": lambda: label(kept8, 8)}
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
            lines.append(f"{name:10s} {C:3d} {kind:>6s} {lq:6d} {hq:6d} {c4[0] // N:8d} {c4[1] // N:8d} {c4[2] // N:8d} {c8[2] // N:8d} " +
                         " ".join(cell(ts[k]) for k in names))
            print(lines[-1], flush=True)
            med = {k: float(np.median(v)) for k, v in ts.items()}
            bound = med["map"] + (max(ts["map"]) - min(ts["map"]))
            notes.append(f"{name} C={C} {kind}: plain cut {med['plain cut']:.3f} vs map + its spread {bound:.3f} "
                         f"({'within' if med['plain cut'] <= bound else 'ABOVE'}); hysteresis 4 {med['hysteresis 4']:.3f} vs map + regions "
                         f"{med['map'] + med['regions 4']:.3f}; hysteresis 8 {med['hysteresis 8']:.3f} vs "
                         f"{med['map'] + med['regions 8']:.3f}")
    lines += notes
    print("\n".join(lines[:2] + notes), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
