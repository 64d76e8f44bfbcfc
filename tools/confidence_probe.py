#!/usr/bin/env python3
"""Times vitseg_confidence (csrc/confidence.hip) with hipEvents at n = 32, 512 x 512, g = 32, C = 2 and 17, on the masks of
tools/regions_probe.py (blobs, uniform random, checkerboard, serpentine) plus one region that fills the frame: the call with
the fp32 map alone, with the region rows (labels of vitseg_regions computed before, for both sides) and with the 16-bin
histogram.  Beside each the ATen composition that gives the same results without the kernel: the decoder tail writing the
full-size fp32 logits (predict_mask(return_logits=True)'s tail), then torch.sigmoid, gather at the mask, the rounding and
index_add_ / scatter_reduce by label or bin.  The two sides of a cell take turns inside one loop so that drift hits them
alike; the spread (min .. max) stands beside every median.  The device call also gets its achieved bytes/s against the
mandatory traffic per pixel (mask 1 B + map 4 B; mask 1 B + labels 4 B; mask 1 B + ground truth 1 B).  Exit status 1 when the
device call is slower than the composition in any cell.

    python tools/confidence_probe.py [--iters 10] [--kind prob] [--out profiles/<tag>_confidence.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import regions_ref as R  # noqa: E402
from visiontransformer_amd import _lib, confidence, regions  # noqa: E402

N, S, G, BINS, LOW_Q = 32, 512, 32, 16, 32768
TRAFFIC = {"map": 5, "rows": 5, "hist": 2}   # mandatory bytes per pixel


def inputs(C):
    rs = np.random.RandomState(C)
    yield "blobs", R.blobs(C, S, S, C, n=N)
    yield "uniform", rs.randint(0, C, size=(N, S, S)).astype(np.uint8)
    yield "checkerboard", np.broadcast_to(R.checkerboard(S, S), (N, S, S)).copy()
    yield "serpentine", np.broadcast_to(R.serpentine(S, S), (N, S, S)).copy()
    yield "full frame", np.ones((N, S, S), np.uint8)


def tail_logits(z, logits):
    """the decoder tail with the logits written: what predict_mask(return_logits=True) launches after the head"""
    n, C, g, _ = z.shape
    mask = torch.empty((n, S, S), dtype=torch.uint8, device=z.device)
    _lib.check(_lib.lib().vitseg_op_upsample_argmax(z.data_ptr(), logits.data_ptr(), mask.data_ptr(), n, C, g, S,
                                                    torch.cuda.current_stream().cuda_stream))


def aten_scores(z, logits, mask, kind):
    tail_logits(z, logits)
    sg = torch.sigmoid(logits)
    idx = mask.long()[:, None]
    p = sg.gather(1, idx)[:, 0]
    if kind == "margin":
        p = (p - sg.scatter(1, idx, -1.0).max(dim=1).values).clamp_(0.0, 1.0)
    return p


def aten_rows(z, logits, mask, labels, cap, kind):
    q = torch.round(aten_scores(z, logits, mask, kind) * 65535.0).long().view(-1)
    lab = labels.view(N, -1).long()
    key = (lab + torch.arange(N, device=lab.device)[:, None] * cap).view(-1)
    keep = lab.view(-1) >= 0
    key, q = key[keep], q[keep]
    out = torch.zeros((N * cap, 4), dtype=torch.int64, device=q.device)
    out[:, 0].index_add_(0, key, torch.ones_like(q))
    out[:, 1].index_add_(0, key, q)
    out[:, 2].scatter_reduce_(0, key, 65535 - q, "amax")
    out[:, 3].index_add_(0, key, (q < LOW_Q).long())
    return out.view(N, cap, 4)


def aten_hist(z, logits, mask, gt, kind):
    q = torch.round(aten_scores(z, logits, mask, kind) * 65535.0).long().view(N, -1)
    key = (((q * BINS) >> 16) + torch.arange(N, device=q.device)[:, None] * BINS).view(-1)
    q = q.view(-1)
    out = torch.zeros((N * BINS, 3), dtype=torch.int64, device=q.device)
    out[:, 0].index_add_(0, key, torch.ones_like(q))
    out[:, 1].index_add_(0, key, (mask == gt).view(-1).long())
    out[:, 2].index_add_(0, key, q)
    return out.view(N, BINS, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--kind", default="prob", choices=["prob", "margin"])
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = "cuda:0"
    lines = [f"vitseg_confidence ({a.kind}), n = {N}, {S} x {S}, g = {G}; milliseconds, median (min .. max) of {a.iters} "
             f"hipEvent-timed calls, device call | ATen composition (tail with logits, sigmoid, gather, rounding, index_add_), "
             f"taking turns; GB/s: the device call against its mandatory traffic; x: composition / device",
             f"{'input':13s} {'C':>3s} {'regions':>8s} " + " ".join(f"{w + ' device':>24s} {'GB/s':>6s} {w + ' ATen':>24s} {'x':>6s}"
                                                                  for w in TRAFFIC)]
    slower = []
    for C in (2, 17):
        z = torch.randn((N, C, G, G), generator=torch.Generator().manual_seed(C)).mul_(3.0).to(dev)
        logits = torch.empty((N, C, S, S), dtype=torch.float32, device=dev)
        for name, m in inputs(C):
            mask = torch.from_numpy(m).to(dev)
            gt = torch.from_numpy(np.roll(m, 3, axis=2).copy()).to(dev)
            counts, _, _ = regions._launch(mask, 0, 4, 0, False)
            cap = max(int(counts.max()), 1)
            _, _, labels = regions._launch(mask, 0, 4, cap, True)
            conf = torch.empty((N, S, S), dtype=torch.float32, device=dev)
            rows = torch.empty((N, cap, 4), dtype=torch.int64, device=dev)
            hist = torch.empty((N, BINS, 3), dtype=torch.int64, device=dev)
            calls = {
                "map": (lambda: confidence._launch(z, mask, a.kind, conf=conf), lambda: aten_scores(z, logits, mask, a.kind)),
                "rows": (lambda: confidence._launch(z, mask, a.kind, labels=labels, scores=rows, low_q=LOW_Q),
                         lambda: aten_rows(z, logits, mask, labels, cap, a.kind)),
                "hist": (lambda: confidence._launch(z, mask, a.kind, gt=gt, hist=hist), lambda: aten_hist(z, logits, mask, gt, a.kind)),
            }
            # the two sides compute the same thing (the composition's fp32 sigmoid is ATen's device kernel: the maps may
            # differ in the last bit, the integer counts of pixels may not)
            calls["rows"][0]()
            want = aten_rows(z, logits, mask, labels, cap, a.kind)
            assert torch.equal(rows[..., 0], want[..., 0]), "pixel counts differ"
            calls["hist"][0]()
            assert int(hist[..., 0].sum()) == N * S * S
            ts = {k: ([], []) for k in calls}
            for it in range(a.iters + 2):
                for k, pair in calls.items():
                    for side, f in enumerate(pair):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        f()
                        e1.record()
                        e1.synchronize()
                        if it >= 2:   # two rounds of warm-up for every call
                            ts[k][side].append(e0.elapsed_time(e1))
            cell = lambda v: f"{np.median(v):8.3f} ({min(v):.3f} .. {max(v):.3f})".rjust(24)
            parts = []
            for k, (d, h) in ts.items():
                md, mh = float(np.median(d)), float(np.median(h))
                parts.append(f"{cell(d)} {N * S * S * TRAFFIC[k] / md / 1e6:6.0f} {cell(h)} {mh / md:6.1f}")
                if md > mh:
                    slower.append((name, C, k, md, mh))
            lines.append(f"{name:13s} {C:3d} {float(counts.float().mean()):8.0f} " + " ".join(parts))
            print(lines[-1], flush=True)
    lines.append("device call no slower than the composition in every cell" if not slower else
                 "SLOWER than the composition: " + "; ".join(f"{n} C={c} {k}: {d:.3f} vs {h:.3f} ms" for n, c, k, d, h in slower))
    print(lines[0] + "\n" + lines[1] + "\n" + lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
