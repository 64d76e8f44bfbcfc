#!/usr/bin/env python3
"""Times the training augmentation (vitseg_augment: warp + colour jitter of the images and nearest warp of the 256 x 256
masks, ONE launch) against what it stands beside, each at the same output size:

  preprocess    Preprocessor.images (uint8 S x S -> fp32, the un-augmented ToTensor) + Preprocessor.masks (256 x 256 -> S x S):
                what an un-augmented step costs today, the yardstick;
  torch         F.affine_grid + F.grid_sample (bilinear) of the fp32 image, a 3x4 colour matrix + clamp, and a second
                grid_sample (nearest) of the mask through float: the ATen composition the kernel replaces.

Shapes: 32 x 512^2 and 64 x 224^2, source uint8 NHWC and fp32 NCHW, the source at the output's size, a random rotation /
scale / translate / flip per sample ("full" preset ranges), border "constant".  Reports ms (hipEvents, median and min) and
the kernel's achieved GB/s against its byte model: 12 B written + 3 B (uint8) or 12 B (fp32) read per image pixel, 1 B written
per mask pixel + the 256 x 256 mask bytes read; the share of the 8 TB/s HBM peak beside it.  `apply` is Augmenter.apply from
the host's side: the matrix composition, two table uploads and the launch.  Not a test; reads nothing but the package.

    timeout 300 python tools/augment_probe.py [--iters 20] [--out profiles/<tag>_augment.txt]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visiontransformer_amd import _lib  # noqa: E402
from visiontransformer_amd.augment import Augmenter  # noqa: E402
from visiontransformer_amd.preprocess import Preprocessor  # noqa: E402

HBM_PEAK = 8.0e12
MASK = 256
FULL = dict(hflip=0.5, vflip=0.5, rot90=True, rotate=15.0, scale=(0.8, 1.25), translate=0.1, brightness=0.2, contrast=0.2,
            saturation=0.2)


def timed(fn, iters):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), float(np.min(ts))


def probe(n, S, fmt, iters, dev):
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (n, S, S, 3), generator=g, dtype=torch.uint8).to(dev)
    f32 = u8.permute(0, 3, 1, 2).float().div(255).contiguous()
    src = u8 if fmt == "u8" else f32
    mask = torch.randint(0, 17, (n, MASK, MASK), generator=g, dtype=torch.uint8).to(dev)
    A = Augmenter(S, device=dev, border="constant", fill_label=255, seed=1, **FULL)
    params = A.sample(n, key=(0, 0))
    tab = torch.from_numpy(np.concatenate([A.matrices(params, (S, S), (S, S)), A.matrices(params, (MASK, MASK), (S, S))])).to(dev)
    col = torch.from_numpy(A.colour(params)).to(dev)
    x = torch.empty((n, 3, S, S), device=dev)
    y = torch.empty((n, S, S), dtype=torch.uint8, device=dev)
    desc = (_lib.CAugmentMask * 1)(_lib.CAugmentMask(mask.data_ptr(), tab.data_ptr() + n * 48, y.data_ptr(), 0, 0, MASK, MASK, S, S))
    fill = (C.c_float * 3)(0, 0, 0)
    fn = _lib.symbol("vitseg_augment")
    st = torch.cuda.current_stream().cuda_stream

    def kernel(with_mask=True, with_colour=True):
        _lib.check(fn(src.data_ptr(), int(fmt == "f32"), n, S, S, S, S, tab.data_ptr(), col.data_ptr() if with_colour else None,
                      x.data_ptr(), desc, int(with_mask), _lib.AUGMENT_CONSTANT, fill, 255, st))

    prep = Preprocessor(S, device=dev)
    aff = Augmenter.affine(params).reshape(n, 2, 3)
    aff[:, :, 2] = aff[:, :, 0] + aff[:, :, 1] + 2 * aff[:, :, 2] - 1   # the unit square's affine in affine_grid's [-1, 1] frame
    theta = torch.from_numpy(aff).float().to(dev)
    cm = col.view(n, 3, 4)

    def torch_path():
        img = src.permute(0, 3, 1, 2).float().div(255) if fmt == "u8" else src
        grid = F.affine_grid(theta, (n, 3, S, S), align_corners=False)
        w = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        out = (torch.einsum("nck,nkhw->nchw", cm[:, :, :3], w) + cm[:, :, 3, None, None]).clamp_(0, 1)
        m = F.grid_sample(mask[:, None].float(), grid, mode="nearest", padding_mode="zeros", align_corners=False)
        return out, m[:, 0].to(torch.uint8)

    for _ in range(3):   # warm-up of every timed shape
        kernel()
        kernel(False, False)
        A.apply(src, mask, params=params)
        prep.images(u8)
        prep.masks(mask, (S, S), dtype=torch.uint8)
        torch_path()
    torch.cuda.synchronize()
    k_ms, k_min = timed(kernel, iters)
    ki_ms, ki_min = timed(lambda: kernel(False, False), iters)
    a_ms, a_min = timed(lambda: A.apply(src, mask, params=params), iters)
    pi_ms, pi_min = timed(lambda: prep.images(u8), iters)
    pm_ms, pm_min = timed(lambda: prep.masks(mask, (S, S), dtype=torch.uint8), iters)
    t_ms, t_min = timed(torch_path, iters)
    px = n * S * S
    img_bytes = px * 12 + px * (3 if fmt == "u8" else 12)
    all_bytes = img_bytes + px + n * MASK * MASK
    pre_bytes = px * 15
    bw = lambda b, ms: f"{b / ms / 1e6:7.1f} GB/s = {100 * b / ms / 1e-3 / HBM_PEAK:4.1f} % of peak"
    return [
        f"{n} x {S}^2, source {fmt}: median (min) of {iters} hipEvent-timed runs, ms",
        f"  vitseg_augment, image + colour + mask {k_ms:8.4f} ({k_min:.4f})   byte model {all_bytes / 1e6:7.1f} MB -> {bw(all_bytes, k_ms)}",
        f"  vitseg_augment, image alone           {ki_ms:8.4f} ({ki_min:.4f})   byte model {img_bytes / 1e6:7.1f} MB -> {bw(img_bytes, ki_ms)}",
        f"  Augmenter.apply (host tables + launch){a_ms:8.4f} ({a_min:.4f})",
        f"  Preprocessor.images (uint8 {S}^2)      {pi_ms:8.4f} ({pi_min:.4f})   byte model {pre_bytes / 1e6:7.1f} MB -> {bw(pre_bytes, pi_ms)}",
        f"  Preprocessor.masks (256^2 -> {S}^2)     {pm_ms:8.4f} ({pm_min:.4f})   images + masks {pi_ms + pm_ms:8.4f}",
        f"  torch affine_grid + grid_sample x2 + colour {t_ms:8.4f} ({t_min:.4f})",
        f"  augment / (images + masks) = {k_ms / (pi_ms + pm_ms):.2f}   image alone / images = {ki_ms / pi_ms:.2f}   torch / augment = {t_ms / k_ms:.1f}",
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = "cuda:0"
    lines = ["augmentation probe: vitseg_augment against the un-augmented pre-processing and the ATen composition"]
    for n, S in ((32, 512), (64, 224)):
        for fmt in ("u8", "f32"):
            lines += probe(n, S, fmt, a.iters, dev)
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
