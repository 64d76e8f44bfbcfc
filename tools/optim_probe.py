#!/usr/bin/env python3
"""Times the fine-tuning optimiser's launches (csrc/optim.hip) with hipEvents at the ViT-B/16 512 arena (88.2 M floats) beside
the plain vitseg_adamw_step in the same process: 20 launches per repetition, 5 repetitions, the median and the spread
(max - min) of the per-launch time.

The gate: the grouped step kernel with one group, no clipping and no EMA may cost at most the plain kernel's median plus the
plain kernel's own max - min over its five repetitions (the extra traffic is one map byte per 64 floats).  The rest is checked
against what the traffic predicts, not gated: the norm pass reads 4 of the step's 28 bytes per element (about 1/7 of its
time), the EMA adds 8 (about 36/28), a frozen backbone removes its share of all traffic.

    python tools/optim_probe.py [--launches 20] [--reps 5] [--out profiles/optim_probe.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visiontransformer_amd import _ext, _lib, optim  # noqa: E402
from visiontransformer_amd.config import ViTSegConfig  # noqa: E402

LR, WD, B1, B2, EPS = 1e-4, 1e-2, 0.9, 0.999, 1e-8


def timed(fn, launches, reps):
    """Per-launch microseconds of `fn`, one figure per repetition of `launches` back-to-back launches (after one warm-up)."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / launches)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    cfg = ViTSegConfig(2, 16, 768, 12, 12, image_size=512)
    n = _lib.param_count(cfg)
    dev = "cuda:0"
    sym = lambda name: _ext.ext_symbol("optim", "vitseg_optim_" + name)
    gen = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, generator=gen, device=dev) * 0.02
    g = torch.randn(n, generator=gen, device=dev) * 1e-3
    m, v, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"optim_probe: ViT-B/16 512 arena, {n} floats ({n * 4 / 2 ** 20:.0f} MiB per buffer); {a.launches} launches x {a.reps} "
             f"repetitions, us per launch: median [min .. max]"]

    def row(name, ts, note=""):
        lines.append(f"{name:<58} {np.median(ts):9.1f} [{min(ts):9.1f} .. {max(ts):9.1f}]{note}")
        print(lines[-1], flush=True)
        return float(np.median(ts))

    def note(text):
        lines.append(text)
        print(text, flush=True)

    step_no = [0]

    def plain():
        step_no[0] += 1
        _lib.check(_lib.lib().vitseg_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, LR, B1, B2, EPS, WD,
                                                step_no[0], 1.0, stream))

    class Route:
        def __init__(self, groups):
            self.G = len(groups.table)
            self.table = torch.from_numpy(groups.table).to(dev)
            self.cmap = torch.from_numpy(groups.chunk_map).to(dev)
            self.nbytes = sym("scratch_bytes")(n, self.G)
            self.scratch = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
            self.state = torch.zeros(8, dtype=torch.float32, device=dev)

        def norm(self):
            _lib.check(sym("grad_norm")(g.data_ptr(), n, self.cmap.data_ptr(), self.table.data_ptr(), self.G, 1.0,
                                        self.scratch.data_ptr(), self.nbytes, stream))

        def prepare(self, flags=0):
            _lib.check(sym("prepare")(self.state.data_ptr(), self.table.data_ptr(), self.G, n, flags, LR, B1, B2, WD, 1.0,
                                      self.scratch.data_ptr(), self.nbytes, stream))

        def step(self, with_ema=False):
            _lib.check(sym("step")(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), ema.data_ptr() if with_ema else None, n,
                                   self.cmap.data_ptr(), self.state.data_ptr(), B1, B2, EPS, 1.0, 0.999, self.scratch.data_ptr(),
                                   self.nbytes, stream))

        def whole(self, flags, with_ema):
            if flags:
                self.norm()
            self.prepare(flags)
            self.step(with_ema)

    one = Route(optim.ArenaGroups([[1.0, 1.0]], np.zeros(n // 64, dtype=np.uint8)))
    layered = Route(optim.arena_groups(cfg, layer_decay=0.75, no_decay="default", freeze="embeddings"))
    head_only = Route(optim.arena_groups(cfg, freeze="backbone"))
    all_flags = optim.FLAG_NORM | optim.FLAG_CLIP | optim.FLAG_SKIP
    one.prepare()
    layered.prepare()
    head_only.prepare()
    # the gated pair, interleaved twice so that a drift of the device shows in both
    t_plain = timed(plain, a.launches, a.reps)
    t_one = timed(one.step, a.launches, a.reps)
    t_plain2 = timed(plain, a.launches, a.reps)
    t_one2 = timed(one.step, a.launches, a.reps)
    base = row("vitseg_adamw_step (plain, today's single launch)", t_plain)
    row("vitseg_adamw_step, second run", t_plain2)
    bound = base + (max(t_plain) - min(t_plain))
    med = row("vitseg_optim_step, one group, no clip, no EMA", t_one, f"   bound {bound:.1f}: {'met' if np.median(t_one) <= bound else 'MISSED'}")
    bound2 = float(np.median(t_plain2)) + (max(t_plain2) - min(t_plain2))
    row("vitseg_optim_step, one group, second run", t_one2, f"   bound {bound2:.1f}: {'met' if np.median(t_one2) <= bound2 else 'MISSED'}")
    t = row("vitseg_optim_grad_norm, one group", timed(one.norm, a.launches, a.reps))
    note(f"    norm / step = {t / med:.3f} (4 / 28 = {4 / 28:.3f} by traffic)")
    row("vitseg_optim_prepare (one block), with the norm's partials", timed(lambda: one.prepare(all_flags), a.launches, a.reps))
    one.prepare()
    t = row("vitseg_optim_step, one group, EMA", timed(lambda: one.step(True), a.launches, a.reps))
    note(f"    EMA step / step = {t / med:.3f} (36 / 28 = {36 / 28:.3f} by traffic)")
    row("vitseg_optim_step, 28 groups (layer decay, embeddings frozen)", timed(layered.step, a.launches, a.reps))
    frozen = float(head_only.table[head_only.cmap.long(), 0].eq(0).float().mean())
    t = row("vitseg_optim_step, backbone frozen", timed(head_only.step, a.launches, a.reps))
    note(f"    {frozen:.4f} of the chunks frozen: {t / med:.4f} of the one-group step's time")
    row("vitseg_optim_grad_norm, backbone frozen", timed(head_only.norm, a.launches, a.reps))
    note("whole optimiser steps (every launch of a step, back to back), beside today's single launch:")
    row("  groups only: prepare + step", timed(lambda: layered.whole(0, False), a.launches, a.reps))
    row("  groups + clip + skip: norm + prepare + step", timed(lambda: layered.whole(all_flags, False), a.launches, a.reps))
    row("  groups + clip + skip + EMA: norm + prepare + step", timed(lambda: layered.whole(all_flags, True), a.launches, a.reps))
    row("  backbone frozen + clip + skip + EMA", timed(lambda: head_only.whole(all_flags, True), a.launches, a.reps))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
