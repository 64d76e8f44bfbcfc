#!/usr/bin/env python3
"""Times the test-time-augmentation merge (vitseg_tta_blend: K low-res maps -> merged fp32 [n, C, S, S] + mask, ONE launch)
against what it stands beside, in the same run:

  forward   one view's vitseg_forward_lowres of ViT-B/16 at the same batch and size (fp32 and bf16): the K = 8 blend has to
            cost less than ONE of the K forwards it follows, or the fusion has not done its job;
  aten      the ATen composition of the same result: per view F.interpolate (bilinear) + flip / rot90 (+ sigmoid), a weighted
            sum, a division, then sigmoid -> argmax: about 3 K + 2 passes over [n, C, S, S] floats.

Shapes: 32 x 512^2, C = 2 and 17, K = 1, 4, 8 (the first ops of d4 on the 32 x 32 grid), both merge modes.  Each timed call
is bracketed by hipEvents after a warm-up of the same shape; the figure is the median (and min) of `--iters` calls.  The byte
model of the blend is its stores, 4 n C S^2 + n S^2 (the low-res maps stay in L2); GB/s and the share of the 8 TB/s HBM peak
are given beside it.  Not a test; reads nothing but the package.

    timeout 600 python tools/tta_probe.py [--iters 20] [--out profiles/tta_probe.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visiontransformer_amd import _lib  # noqa: E402
from visiontransformer_amd.model import ViTSegmentationModel  # noqa: E402

HBM_PEAK = 8.0e12
N, S, P = 32, 512, 16


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


def unview(y, op):
    z = torch.rot90(y, -(op & 3), dims=(-2, -1))
    return torch.flip(z, [-1]) if op >> 2 else z


def aten_merge(lows, ops, mode):
    if len(lows) == 1:
        u = unview(F.interpolate(lows[0], size=(S, S), mode="bilinear", align_corners=False), ops[0])
        res = u.sigmoid() if mode else u
    else:
        acc = None
        for low, op in zip(lows, ops):
            u = unview(F.interpolate(low, size=(S, S), mode="bilinear", align_corners=False), op)
            t = u.sigmoid() if mode else u
            acc = t.clone() if acc is None else acc.add_(t)
        res = acc.div_(float(len(lows)))
    return res, (res if mode else res.sigmoid()).argmax(dim=1).to(torch.uint8)


def probe_blend(Cc, K, mode, iters, dev):
    g = S // P
    gen = torch.Generator().manual_seed(Cc * 100 + K)
    lows = [torch.randn((N, Cc, g, g), generator=gen).to(dev) for _ in range(K)]
    ops = list(range(K))
    merged = torch.empty((N, Cc, S, S), device=dev)
    mask = torch.empty((N, S, S), dtype=torch.uint8, device=dev)
    descs = (_lib.CTTAView * K)(*[_lib.CTTAView(z.data_ptr(), g, op, 1.0) for z, op in zip(lows, ops)])
    fn, st = _lib.symbol("vitseg_tta_blend"), torch.cuda.current_stream().cuda_stream

    def blend(want_merged=True):
        _lib.check(fn(descs, K, N, Cc, S, mode, merged.data_ptr() if want_merged else None, mask.data_ptr(), st))

    for _ in range(3):   # warm-up of every timed shape
        blend()
        blend(False)
        ref, ref_mask = aten_merge(lows, ops, mode)
    torch.cuda.synchronize()
    # the two computations agree (ATen's GPU kernels round differently: a tolerance, not bits)
    err = float((merged - ref).abs().max())
    differ = float((mask != ref_mask).float().mean())
    del ref, ref_mask
    b_ms, b_min = timed(blend, iters)
    m_ms, m_min = timed(lambda: blend(False), iters)
    a_ms, a_min = timed(lambda: aten_merge(lows, ops, mode), max(3, iters // 4))
    stores = 4 * N * Cc * S * S + N * S * S
    return dict(C=Cc, K=K, mode=["logits", "probs"][mode], blend_ms=b_ms, blend_min_ms=b_min, blend_mask_only_ms=m_ms,
                blend_mask_only_min_ms=m_min, aten_ms=a_ms, aten_min_ms=a_min, store_bytes=stores,
                blend_gbps=stores / b_ms / 1e6, blend_share_of_hbm_peak=stores / (b_ms * 1e-3) / HBM_PEAK,
                aten_over_blend=a_ms / b_ms, max_abs_diff_to_aten=err, mask_share_differing_from_aten=differ)


def probe_forward(Cc, precision, iters, dev):
    m = ViTSegmentationModel(Cc, P, 768, 12, 12, image_size=S, precision=precision, device=dev).eval()
    x = torch.rand((N, 3, S, S), generator=torch.Generator().manual_seed(1)).to(dev)
    low = torch.empty((N, Cc, S // P, S // P), device=dev)
    ws, lp = m.workspace(N, S), m._bf16_arena()
    cfg = C.byref(_lib.CConfig.from_config(m.cfg))
    fn, st = _lib.symbol("vitseg_forward_lowres"), torch.cuda.current_stream().cuda_stream

    def fwd():
        _lib.check(fn(cfg, S, m.arena.data_ptr(), None if lp is None else lp.data_ptr(), x.data_ptr(), N, m.precision,
                      low.data_ptr(), ws.data_ptr(), ws.numel(), st))

    for _ in range(3):
        fwd()
    torch.cuda.synchronize()
    ms, mn = timed(fwd, iters)
    return dict(C=Cc, precision=precision, forward_ms=ms, forward_min_ms=mn)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tta_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on the MI355X: there is nothing to report without one"
    dev = "cuda:0"
    res = dict(what="vitseg_tta_blend at 32 x 512^2 against one view's forward (ViT-B/16) and the ATen composition; ms are "
                    "medians of hipEvent-timed calls after warm-up", batch=N, size=S, iters=a.iters, forward=[], blend=[])
    for Cc in (2, 17):
        for precision in ("fp32", "bf16"):
            res["forward"].append(probe_forward(Cc, precision, a.iters, dev))
            print(json.dumps(res["forward"][-1]), flush=True)
        torch.cuda.empty_cache()
        for K in (1, 4, 8):
            for mode in (0, 1):
                res["blend"].append(probe_blend(Cc, K, mode, a.iters, dev))
                print(json.dumps(res["blend"][-1]), flush=True)
    fastest = {Cc: min(f["forward_ms"] for f in res["forward"] if f["C"] == Cc) for Cc in (2, 17)}
    k8 = [b for b in res["blend"] if b["K"] == 8]
    res["relations"] = dict(
        k8_blend_below_one_forward=all(b["blend_ms"] < fastest[b["C"]] for b in k8),
        k8_blend_over_fastest_forward=max(b["blend_ms"] / fastest[b["C"]] for b in k8),
        blend_not_slower_than_aten=all(b["blend_ms"] <= b["aten_ms"] for b in res["blend"]),
        least_aten_over_blend=min(b["aten_over_blend"] for b in res["blend"]))
    print(json.dumps(res["relations"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
