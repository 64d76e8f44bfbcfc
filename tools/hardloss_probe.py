#!/usr/bin/env python3
"""Times the hard-pixel losses (csrc/hardloss.hip) with hipEvents at 32 x 512^2, g = 32, C = 2 and 17, beside
vitseg_ce_loss_opts with its gradient in the same process: 10 calls per repetition, 5 repetitions, the median and the spread
(max - min) of the per-call time.  uint8 targets, 5 % of them the ignored label, nine in ten of the rest the arg-max class of
their low-res cell (a model that is mostly right), class weights set.

By traffic: the focal call moves the bytes of vitseg_ce_loss_opts, so its time is reported beside that call's median plus that
call's own max - min.  The OHEM call adds one 4 B / pixel plane write and four plane reads (two histogram rounds, the sum pass,
the gradient kernel) to the 4 C B / pixel gradient write; its ratio to vitseg_ce_loss_opts is reported, with no target.

    python tools/hardloss_probe.py [--calls 10] [--reps 5] [--out profiles/hardloss_probe.txt]"""
import argparse
import ctypes as C
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visiontransformer_amd import _ext, _lib  # noqa: E402

B, S, G = 32, 512, 32


def timed(fn, calls, reps):
    """Per-call microseconds of `fn`, one figure per repetition of `calls` back-to-back calls (after one warm-up)."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / calls)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = "cuda:0"
    L = _lib.lib()
    sym = lambda name: _ext.ext_symbol("hardloss", name)
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"hardloss_probe: {B} x {S}^2 pixels, g = {G}; {a.calls} calls x {a.reps} repetitions, us per call: median [min .. max]",
             "uint8 targets, 5 % the ignored label 255, nine in ten of the rest the arg-max class of their low-res cell, class weights "
             "0.5 .. 2; every call with grad_logits and stats, hipEvents around back-to-back calls on one stream"]

    def row(name, ts, note=""):
        lines.append(f"{name:<58} {np.median(ts):9.1f} [{min(ts):9.1f} .. {max(ts):9.1f}]{note}")
        print(lines[-1], flush=True)
        return float(np.median(ts))

    def note(text):
        lines.append(text)
        print(text, flush=True)

    for C_ in (2, 17):
        gen = torch.Generator(device=dev).manual_seed(C_)
        z = torch.randn(B, C_, G, G, generator=gen, device=dev) * 3.0
        t = z.argmax(dim=1).repeat_interleave(S // G, dim=1).repeat_interleave(S // G, dim=2)
        flip = torch.rand(t.shape, generator=gen, device=dev) < 0.1
        t = torch.where(flip, torch.randint(0, C_, t.shape, generator=gen, device=dev), t)
        t[torch.rand(t.shape, generator=gen, device=dev) < 0.05] = 255
        t = t.to(torch.uint8).contiguous()
        w = torch.linspace(0.5, 2.0, C_, device=dev)
        grad = torch.empty(B, C_, S, S, device=dev)
        loss = torch.empty(1, device=dev)
        stats = torch.zeros(4, dtype=torch.int64, device=dev)
        scr = torch.empty(L.vitseg_ce_scratch_bytes(B, S), dtype=torch.uint8, device=dev)
        oscr = torch.empty(int(_lib.symbol("vitseg_ce_options_scratch_bytes")(B, S)), dtype=torch.uint8, device=dev)
        hscr = torch.empty(int(sym("vitseg_hard_loss_scratch_bytes")(B, S)), dtype=torch.uint8, device=dev)
        o = _lib.CCEOptions(1, 0, 255, w.data_ptr(), 0.0, oscr.data_ptr(), oscr.numel())
        args = (z.data_ptr(), t.data_ptr(), 1, grad.data_ptr(), scr.data_ptr(), loss.data_ptr(), B, C_, G, S, C.byref(o))

        def plain():
            _lib.check(_lib.symbol("vitseg_ce_loss_opts")(*args, 1.0, stream))

        def hard(gamma=0.0, thresh=float("inf"), q16=0):
            h = _ext.CHardOptions(gamma, thresh, 0, q16, 0, hscr.data_ptr(), hscr.numel())
            return lambda: _lib.check(sym("vitseg_hard_ce_loss")(*args, C.byref(h), 1.0, None, stats.data_ptr(), stream))

        note(f"C = {C_}: grad_logits {grad.numel() * 4 / 2 ** 20:.0f} MiB, plane {B * S * S * 4 / 2 ** 20:.0f} MiB")
        # the pair held against each other, interleaved twice so that a drift of the device shows in both
        t_plain, t_focal = timed(plain, a.calls, a.reps), timed(hard(2.0), a.calls, a.reps)
        t_plain2, t_focal2 = timed(plain, a.calls, a.reps), timed(hard(2.0), a.calls, a.reps)
        base = row("  vitseg_ce_loss_opts with its gradient", t_plain)
        row("  vitseg_ce_loss_opts, second run", t_plain2)
        for ts, tp, name in ((t_focal, t_plain, "  focal only, gamma = 2"), (t_focal2, t_plain2, "  focal only, second run")):
            bound = float(np.median(tp)) + (max(tp) - min(tp))
            row(name, ts, f"   plain median + its spread {bound:.1f}: {'within' if np.median(ts) <= bound else 'OUTSIDE'}")
        for name, fn in (("  OHEM keep 0.25, no threshold", hard(0.0, float("inf"), 16384)),
                         ("  OHEM keep 0.25, threshold 0.7", hard(0.0, float(np.float32(-math.log(0.7))), 16384)),
                         ("  focal 2 + OHEM keep 0.25, threshold 0.7", hard(2.0, float(np.float32(-math.log(0.7))), 16384))):
            med = row(name, timed(fn, a.calls, a.reps))
            n_valid, k, n_hard, _ = stats.tolist()
            note(f"      {med / base:.3f} of vitseg_ce_loss_opts; n_valid {n_valid}, k {k}, |H| {n_hard} ({n_hard / n_valid:.3f})")
        del grad
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
