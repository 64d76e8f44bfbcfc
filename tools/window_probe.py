#!/usr/bin/env python3
"""Times sliding-window inference against the plain composition it replaces, on the same build and the same tile forwards:

  windowed      ViTSegmentationModel.predict_mask_windowed, mask only: gather + vitseg_forward_lowres per chunk of tiles,
                then ONE vitseg_window_blend launch over the low-res tiles;
  composition   predict_mask(tiles, return_logits=True) per chunk (the full-resolution logits of every tile are written),
                then a torch weighted accumulate per tile, a divide, sigmoid and argmax.

4 images of 2048 x 1536, S = 512, stride 384 (20 windows per image), ViT-B/16, bf16, "linear" weights, one class count per
run.  Reports ms (hipEvents, median) for the forwards and for the blend / the torch tail separately, and the blend's
achieved GB/s against its byte model: H W bytes of mask + C H W 4 bytes when logits are written + the low-res reads.
Not a test; reads nothing but the package.

    timeout 300 python tools/window_probe.py --classes 2 [--iters 5] [--out profiles/<tag>_window_c2.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visiontransformer_amd import _lib  # noqa: E402
from visiontransformer_amd.model import ViTSegmentationModel  # noqa: E402

B, H, W, S, STRIDE, TILE_BATCH = 4, 1536, 2048, 512, 384, 32


def timed(fn, iters):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--out")
    a = ap.parse_args()
    C = a.classes
    dev = "cuda:0"
    model = ViTSegmentationModel(C, 16, 768, 12, 12, image_size=S, precision=a.precision, device=dev).eval()
    model.reset_parameters(seed=1)
    x = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(0)).to(dev)
    oy, ox = _lib.window_origins(H, S, STRIDE), _lib.window_origins(W, S, STRIDE)
    ny, nx = len(oy), len(ox)
    T = B * ny * nx
    i = torch.arange(S, dtype=torch.float32)
    w1 = torch.minimum(i + 1, S - i).to(dev)
    wt = (w1[:, None] * w1[None, :])[None]

    def lowres():
        return model._window_lowres(x, False, S, STRIDE, "linear", TILE_BATCH)

    def tile_logits():   # the composition's forwards: full-resolution logits of every tile, chunk by chunk
        out = []
        for first in range(0, T, TILE_BATCH):
            ids = range(first, min(first + TILE_BATCH, T))
            tiles = torch.stack([x[t // (ny * nx), :, oy[(t // nx) % ny]:oy[(t // nx) % ny] + S, ox[t % nx]:ox[t % nx] + S] for t in ids])
            out.append(model.predict_mask(tiles, return_logits=True)[1])
        return out

    def torch_tail(chunks):
        acc = torch.zeros((B, C, H, W), device=dev)
        ws = torch.zeros((B, 1, H, W), device=dev)
        t = 0
        for lg in chunks:
            for k in range(lg.shape[0]):
                b, y, xx = t // (ny * nx), oy[(t // nx) % ny], ox[t % nx]
                acc[b, :, y:y + S, xx:xx + S] += wt * lg[k]
                ws[b, :, y:y + S, xx:xx + S] += wt
                t += 1
        return (acc / ws).sigmoid().argmax(dim=1).to(torch.uint8)

    for _ in range(2):   # warm-up of every shape the timed windows use
        plan = lowres()
        model._window_blend(plan, False, True)
        model._window_blend(plan, True, True)
        chunks = tile_logits()
        ref = torch_tail(chunks)
    torch.cuda.synchronize()
    fwd_ms, fwd_min, plan = timed(lowres, a.iters)
    blend_ms, blend_min, mask = timed(lambda: model._window_blend(plan, False, True), 4 * a.iters)
    both_ms, both_min, _ = timed(lambda: model._window_blend(plan, True, True), 4 * a.iters)
    cfwd_ms, cfwd_min, chunks = timed(tile_logits, a.iters)
    tail_ms, tail_min, ref = timed(lambda: torch_tail(chunks), a.iters)
    differ = int((mask != ref).sum())
    low_bytes = T * C * (S // 16) ** 2 * 4
    model_mask = B * H * W + low_bytes
    model_both = model_mask + B * C * H * W * 4
    tile_bytes = T * C * S * S * 4
    lines = [
        f"sliding-window probe: {B} x {W}x{H}, S = {S}, stride {STRIDE} ({ny} x {nx} windows per image, {T} tiles, {TILE_BATCH} per "
        f"forward), ViT-B/16, {a.precision}, C = {C}, linear weights; median (min) of {a.iters} hipEvent-timed runs, ms",
        f"windowed:    forwards (gather + forward_lowres) {fwd_ms:9.3f} ({fwd_min:.3f})   blend, mask only {blend_ms:8.4f} ({blend_min:.4f})"
        f"   total {fwd_ms + blend_ms:9.3f}",
        f"composition: forwards (slice + predict_mask with logits) {cfwd_ms:9.3f} ({cfwd_min:.3f})   torch accumulate + divide + argmax "
        f"{tail_ms:8.3f} ({tail_min:.3f})   total {cfwd_ms + tail_ms:9.3f}",
        f"blend, mask only:      byte model {model_mask / 1e6:8.1f} MB -> {model_mask / blend_ms / 1e6:8.1f} GB/s",
        f"blend, logits + mask:  {both_ms:8.4f} ({both_min:.4f}) ms, byte model {model_both / 1e6:8.1f} MB -> {model_both / both_ms / 1e6:8.1f} GB/s",
        f"the composition's per-tile full-resolution logits: {tile_bytes / 1e6:.1f} MB written by the forwards and read back by the tail",
        f"mask pixels where the composition (torch arithmetic, other summation) differs from the blend: {differ} of {B * H * W}",
    ]
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
