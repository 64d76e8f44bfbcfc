#!/usr/bin/env python3
"""Times the Lovasz-Softmax term on the fused path (csrc/lovasz.hip) with hipEvents at 32 x 512^2, g = 32 -- the inputs of
tools/cldice_probe.py -- for C = 2 with K = 1 and C = 17 with K = 1, 4 and 16, each pooled and per image.  Medians of five
repetitions of ten calls with their gradient, us per call, three things side by side in one process:
  - vitseg_ce_lovasz_loss (CE + 0.5 Dice + 0.5 Lovasz, with grad_logits);
  - vitseg_ce_dice_loss alone on the same inputs;
  - the ATen composition on the device: full-size logits (F.interpolate) -> softmax -> torch.sort per class -> cumsum -> autograd.

The traffic ESTIMATE of the term per listed class, with N = 32 x 512^2 keys: the plane pass writes 8 N bytes; each of the four
radix passes reads 4 N (histogram) + 8 N (scatter) and writes 8 N, plus 1 KiB of histogram per tile of 2048 keys written, scanned
and read; the rank passes read 4 N + 8 N and scatter 4 N.  That is 104 N bytes, 3.5 GB at N = 2^23, 870 us at 4 TB/s.  The probe
prints the estimate beside the measured difference; it is an estimate (the clDice one was off ninefold).

--ab PREV.so: also times vitseg_ce_loss_opts and vitseg_ce_dice_loss of a second build of the library (the parent commit's)
in the same process, alternating with this build's, and says whether the medians agree within the parent's own spread.
--only NAME: runs the new call alone, for a kernel trace (rocprofv3 --kernel-trace --stats); NAME = C,K,per_image.

    python tools/lovasz_probe.py [--calls 10] [--reps 5] [--ab PREV.so] [--out profiles/lovasz_probe.txt]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

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


def inputs(C_, dev):
    gen = torch.Generator(device=dev).manual_seed(C_)
    z = torch.randn(B, C_, G, G, generator=gen, device=dev) * 3.0
    t = z.argmax(dim=1).repeat_interleave(S // G, dim=1).repeat_interleave(S // G, dim=2)
    flip = torch.rand(t.shape, generator=gen, device=dev) < 0.1
    t = torch.where(flip, torch.randint(0, C_, t.shape, generator=gen, device=dev), t)
    t[torch.rand(t.shape, generator=gen, device=dev) < 0.05] = 255
    return z, t.to(torch.uint8).contiguous()


def _lovasz_flat(p, fg):
    """One class on one segment: p, fg flat tensors of the valid pixels (the published lovasz_softmax_flat's body)."""
    errors = (fg - p).abs()
    errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
    gt = fg[perm]
    gts = gt.sum()
    inter = gts - gt.cumsum(0)
    union = gts + (1.0 - gt).cumsum(0)
    jac = 1.0 - inter / union
    jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
    return torch.dot(errors_sorted, jac)


def aten_composition(z, t, classes, per_image, weight):
    """CE + 0.5 Dice + weight Lovasz from ATen ops and autograd on the device."""
    C_ = z.shape[1]
    zz = z.detach().clone().requires_grad_(True)
    up = F.interpolate(zz, size=(S, S), mode="bilinear", align_corners=False)
    tl = t.long()
    void = tl == 255
    ce = F.cross_entropy(up, tl, ignore_index=255)
    p = torch.softmax(up, dim=1)
    keep = (~void).float()
    onehot = F.one_hot(torch.where(void, torch.zeros_like(tl), tl), C_).permute(0, 3, 1, 2).float() * keep[:, None]
    pk = p * keep[:, None]
    I, P, T = (pk * onehot).sum((0, 2, 3)), pk.sum((0, 2, 3)), onehot.sum((0, 2, 3))
    dice = (1.0 - (2.0 * I + 1e-6) / (P + T + 1e-6)).mean()
    lov = 0.0
    segments = [(slice(b, b + 1), ~void[b:b + 1]) for b in range(B)] if per_image else [(slice(0, B), ~void)]
    for sl, valid in segments:
        terms = []
        for c in classes:
            fg = onehot[sl, c][valid]
            if fg.sum() == 0:   # classes='present' (a host read, as in the published code)
                continue
            terms.append(_lovasz_flat(p[sl, c][valid], fg))
        if terms:
            lov = lov + sum(terms) / len(terms)
    loss = ce + 0.5 * dice + weight * lov / len(segments)
    loss.backward()
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ab")
    ap.add_argument("--only")
    ap.add_argument("--no-aten", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = "cuda:0"
    if not torch.cuda.is_available():
        raise SystemExit("lovasz_probe needs the GPU: a timing taken anywhere else says nothing")
    L = _lib.lib()
    sym = lambda name: _ext.ext_symbol("lovasz", name)
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"lovasz_probe: {B} x {S}^2 pixels, g = {G}; {a.calls} calls x {a.reps} repetitions, us per call: median [min .. max]",
             "uint8 targets, 5 % the ignored label 255, nine in ten of the rest the arg-max class of their low-res cell; CE + 0.5 Dice "
             "+ 0.5 Lovasz (present classes), every call with grad_logits, hipEvents around back-to-back calls on one stream"]

    def row(name, ts, note=""):
        lines.append(f"{name:<62} {np.median(ts):10.1f} [{min(ts):10.1f} .. {max(ts):10.1f}]{note}")
        print(lines[-1], flush=True)
        return float(np.median(ts))

    def note(text):
        lines.append(text)
        print(text, flush=True)

    def setup(C_):
        z, t = inputs(C_, dev)
        grad = torch.empty(B, C_, S, S, device=dev)
        terms = torch.empty(4, device=dev)
        scr = torch.empty(L.vitseg_ce_scratch_bytes(B, S), dtype=torch.uint8, device=dev)
        oscr = torch.empty(int(_lib.symbol("vitseg_ce_options_scratch_bytes")(B, S)), dtype=torch.uint8, device=dev)
        dscr = torch.empty(int(_lib.symbol("vitseg_dice_options_scratch_bytes")(B, C_, S)), dtype=torch.uint8, device=dev)
        o = _lib.CCEOptions(1, 0, 255, None, 0.0, oscr.data_ptr(), oscr.numel())
        d = _lib.CDiceOptions(1.0, 0.5, 1e-6, 1, dscr.data_ptr(), dscr.numel())
        args = (z.data_ptr(), t.data_ptr(), 1, grad.data_ptr(), scr.data_ptr(), terms.data_ptr(), B, C_, G, S, C.byref(o))
        keep = (z, t, grad, terms, scr, oscr, dscr, o, d)
        return z, t, args, d, terms, keep

    def new_call(args, d, C_, K, per_image):
        classes = list(range(1, K + 1)) if C_ > K else [C_ - 1]
        cscr = torch.empty(int(sym("vitseg_lovasz_scratch_bytes")(B, K, S)), dtype=torch.uint8, device=dev)
        arr = (C.c_int32 * K)(*classes)
        c = _ext.CLovaszOptions(0.5, K, arr, per_image, 1, cscr.data_ptr(), cscr.numel(), None, None, None)
        fn = lambda: _lib.check(sym("vitseg_ce_lovasz_loss")(*args, C.byref(d), C.byref(c), 1.0, stream))
        fn.keep = (cscr, arr, c)
        return fn, classes, cscr.numel()

    if a.only:
        C_, K, per_image = (int(v) for v in a.only.split(","))
        z, t, args, d, terms, keep = setup(C_)
        fn, _, _ = new_call(args, d, C_, K, per_image)
        for _ in range(a.calls + 1):
            fn()
        torch.cuda.synchronize()
        print("terms", terms.tolist())
        return

    prev = None
    if a.ab:
        prev = C.CDLL(os.path.abspath(a.ab))
        for name in ("vitseg_ce_loss_opts", "vitseg_ce_dice_loss"):
            getattr(prev, name).restype = C.c_int
            getattr(prev, name).argtypes = _lib.symbol(name).argtypes

    for C_ in (2, 17):
        z, t, args, d, terms, keep = setup(C_)
        N = B * S * S
        note(f"C = {C_}: grad_logits {B * C_ * S * S * 4 / 2 ** 20:.0f} MiB, one plane {N * 4 / 2 ** 20:.0f} MiB")
        opts = lambda lib: (lambda: _lib.check(lib.vitseg_ce_loss_opts(*args, 1.0, stream)))
        dice = lambda lib: (lambda: _lib.check(lib.vitseg_ce_dice_loss(*args, C.byref(d), 1.0, stream)))
        _lib.symbol("vitseg_ce_loss_opts"), _lib.symbol("vitseg_ce_dice_loss")   # bound
        base = row("  vitseg_ce_dice_loss with its gradient", timed(dice(L), a.calls, a.reps))
        if prev is not None:   # parent | this build | parent | this build, so that a drift of the device shows in both
            for name, mk in (("vitseg_ce_loss_opts", opts), ("vitseg_ce_dice_loss", dice)):
                p1, n1 = timed(mk(prev), a.calls, a.reps), timed(mk(L), a.calls, a.reps)
                p2, n2 = timed(mk(prev), a.calls, a.reps), timed(mk(L), a.calls, a.reps)
                pp, nn = p1 + p2, n1 + n2
                row(f"  A/B {name}: parent", pp)
                spread = max(pp) - min(pp)
                ok = abs(np.median(nn) - np.median(pp)) <= spread
                row(f"  A/B {name}: this build", nn, f"   parent's spread {spread:.1f}: {'within' if ok else 'OUTSIDE'}")
        for K in ((1,) if C_ == 2 else (1, 4, 16)):
            for per_image in (0, 1):
                fn, classes, nbytes = new_call(args, d, C_, K, per_image)
                how = "per image" if per_image else "pooled"
                med = row(f"  vitseg_ce_lovasz_loss K = {K}, {how}", timed(fn, a.calls, a.reps))
                est_bytes = 104 * N * K
                est = est_bytes / 4e12 * 1e6
                note(f"      {med / base:.2f} of vitseg_ce_dice_loss; the term costs {med - base:.1f} us; ESTIMATE 104 B x {K} x {N} keys = "
                     f"{est_bytes / 1e9:.2f} GB, {est:.1f} us at 4 TB/s: achieved {est / max(med - base, 1e-9):.2f} of it; scratch "
                     f"{nbytes / 2 ** 20:.0f} MiB; terms {[round(v, 6) for v in terms.tolist()]}")
                if not a.no_aten:
                    at = timed(lambda: aten_composition(z, t, classes, per_image, 0.5), max(a.calls // 5, 1), a.reps)
                    am = row(f"  ATen composition K = {K}, {how}", at)
                    under = med - base < min(at)
                    note(f"      the fused call takes {med / am:.3f} of it; the term alone {'lies under' if under else 'DOES NOT lie under'} "
                         f"the composition's fastest repetition ({min(at):.1f})")
                del fn
                torch.cuda.empty_cache()
        del keep, z, t
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
