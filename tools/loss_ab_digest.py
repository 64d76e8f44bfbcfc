#!/usr/bin/env python3
"""Bitwise A/B of the fused losses between two builds of libvitseg (every sum runs in a fixed order; the OHEM histograms are
integer atomics: the same bits on every call).  Copy the old build to visiontransformer_amd/csrc/libvitseg_prev.so, rebuild,
then run each side as a process of its own and diff the outputs:
    python tools/loss_ab_digest.py prev [case-name prefix ...] > a.txt
    python tools/loss_ab_digest.py new  [case-name prefix ...] > b.txt
The four C entry points (vitseg_ce_loss, vitseg_ce_loss_opts, vitseg_ce_dice_loss, vitseg_hard_ce_loss) are driven directly.
Per case one line: a SHA-256 over the loss, the gradient, the terms, the stats and the per-pixel plane, whichever the form has.
Every output and scratch buffer arrives filled with 0xff bytes (NaN), so a stale read shows.
Forms: plain (both target types); the CE options (ignore, weights, smoothing, all three, a fully ignored batch, a bad label);
Dice (both weights, ce_weight = 0, dice_weight = 0, without background, with the CE options); focal; OHEM by fraction, by
threshold and by min_kept, and focal with OHEM; each with and without grad_logits.
Shapes (B, C, g, S): the small ones of the tests, and the smallest at which each fixed-order sum enters its four-chain loop
(more than 3072 partials): 4 x 512^2 for the 256-pixel blocks, 13 x 512^2 for the 1024-pixel count and sum passes,
25 x 512^2 for the 2048-pixel Dice sum."""
import ctypes as C
import functools
import hashlib
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import visiontransformer_amd._lib as L  # noqa: E402

if len(sys.argv) < 2 or sys.argv[1] not in ("prev", "new"):
    sys.exit(__doc__)
if sys.argv[1] == "prev":
    L.LIB_PATH = L.LIB_PATH.replace("libvitseg.so", "libvitseg_prev.so")
from visiontransformer_amd import _ext  # noqa: E402

DEV = "cuda:0"
SHAPES = [(3, 2, 7, 28), (3, 17, 7, 28), (2, 3, 5, 40), (1, 1, 16, 64), (4, 2, 32, 512), (13, 2, 32, 512), (25, 2, 32, 512)]
ALL3 = dict(ignore=True, weights=True, eps=0.1)
THRESH = float(torch.tensor(-math.log(0.7), dtype=torch.float32))
# name: (entry point, options of the form)
FORMS = {
    "plain_i64": ("ce", dict(i64=True)),
    "plain_u8": ("ce", dict()),
    "opts_null_i64": ("opts", dict(null=True, i64=True)),
    "opts_defaults": ("opts", dict()),
    "opts_ignore": ("opts", dict(ignore=True)),
    "opts_ignore_i64": ("opts", dict(ignore=True, i64=True)),
    "opts_weights": ("opts", dict(weights=True)),
    "opts_smoothing": ("opts", dict(eps=0.1)),
    "opts_all3": ("opts", ALL3),
    "opts_all_ignored": ("opts", dict(ALL3, all_ignored=True)),
    "opts_bad_label": ("opts", dict(ALL3, bad=True)),
    "dice_1_1": ("dice", dict(null=True)),
    "dice_1_1_i64": ("dice", dict(null=True, i64=True)),
    "dice_ce0": ("dice", dict(null=True, cw=0.0)),
    "dice_dice0": ("dice", dict(null=True, dw=0.0)),
    "dice_no_background": ("dice", dict(null=True, background=False, smooth=1.0)),
    "dice_all3": ("dice", dict(ALL3, cw=2.0, dw=0.5)),
    "dice_all3_ce0": ("dice", dict(ALL3, cw=0.0)),
    "dice_bad_label": ("dice", dict(ALL3, bad=True)),
    "hard_nothing": ("hard", dict(null=True)),
    "hard_nothing_opts": ("hard", dict(ignore=True, weights=True)),
    "hard_stats_only": ("hard", dict(null=True, stats=True)),
    "focal_2": ("hard", dict(ignore=True, weights=True, gamma=2.0, stats=True, plane=True)),
    "focal_2_null_i64": ("hard", dict(null=True, gamma=2.0, i64=True)),
    "focal_bad_label": ("hard", dict(ignore=True, weights=True, gamma=2.0, bad=True, stats=True)),
    "ohem_fraction": ("hard", dict(ignore=True, weights=True, q16=16384, stats=True, plane=True)),
    "ohem_threshold": ("hard", dict(ignore=True, weights=True, thresh=THRESH, stats=True)),
    "ohem_min_kept": ("hard", dict(null=True, thresh=THRESH, min_kept=100, stats=True, i64=True)),
    "ohem_all_ignored": ("hard", dict(ignore=True, q16=16384, all_ignored=True, stats=True)),
    "focal_ohem": ("hard", dict(ignore=True, weights=True, gamma=2.0, q16=16384, thresh=THRESH, stats=True, plane=True)),
}


def poisoned(nbytes):
    return torch.full((max(int(nbytes), 1),), 0xFF, dtype=torch.uint8, device=DEV)


@functools.lru_cache(maxsize=1)
def inputs(shape):
    """the low-res logits, the int64 labels and the pixels that the ignoring forms ignore: once per shape, not modified"""
    B, C_, g, S = shape
    gen = torch.Generator().manual_seed(1000 * B + 10 * C_ + g)
    z = (torch.randn(B, C_, g, g, generator=gen) * 3.0).float()
    t = torch.randint(0, C_, (B, S, S), generator=gen)
    return z, t, torch.rand(B, S, S, generator=gen) < 0.1


def run(shape, form, want_grad):
    B, C_, g, S = shape
    entry, f = FORMS[form]
    if f.get("background") is False and C_ < 2:
        return None
    z, t, some = inputs(shape)
    t = t.clone()
    ii = 255
    if f.get("ignore"):
        t[some] = ii
    if f.get("all_ignored"):
        t[:] = ii
    if f.get("bad"):
        t[0, S // 2, S // 3] = C_
    t = t if f.get("i64") else t.to(torch.uint8)
    w = torch.linspace(0.5, 2.0, C_) if f.get("weights") else None
    zd, td = z.to(DEV), t.to(DEV)
    wd = w.to(DEV) if w is not None else None
    lib = L.lib()
    stream = torch.cuda.current_stream().cuda_stream
    scr = poisoned(lib.vitseg_ce_scratch_bytes(B, S))
    out = dict(loss=poisoned(4), grad=poisoned(4 * B * C_ * S * S) if want_grad else None)
    ce = None
    if not f.get("null"):
        oscr = poisoned(L.ce_opts_symbol("vitseg_ce_options_scratch_bytes")(B, S))
        ce = L.CCEOptions(int(bool(f.get("ignore") or f.get("all_ignored"))), 0, ii, wd.data_ptr() if wd is not None else None,
                          f.get("eps", 0.0), oscr.data_ptr(), oscr.numel())
    cep = C.byref(ce) if ce is not None else None
    gp = out["grad"].data_ptr() if want_grad else None
    head = (zd.data_ptr(), td.data_ptr(), int(t.dtype == torch.uint8), gp, scr.data_ptr())
    if entry == "ce":
        L.check(lib.vitseg_ce_loss(*head, out["loss"].data_ptr(), B, C_, g, S, stream))
    elif entry == "opts":
        L.check(L.ce_opts_symbol("vitseg_ce_loss_opts")(*head, out["loss"].data_ptr(), B, C_, g, S, cep, 0.5, stream))
    elif entry == "dice":
        out["terms"] = poisoned(12)
        del out["loss"]
        dscr = poisoned(L.dice_symbol("vitseg_dice_options_scratch_bytes")(B, C_, S))
        d = L.CDiceOptions(f.get("cw", 1.0), f.get("dw", 1.0), f.get("smooth", 1e-6), int(f.get("background", True)), dscr.data_ptr(),
                           dscr.numel())
        L.check(L.dice_symbol("vitseg_ce_dice_loss")(*head, out["terms"].data_ptr(), B, C_, g, S, cep, C.byref(d), 0.5, stream))
    else:
        sym = lambda name: _ext.ext_symbol("hardloss", name)
        hscr = poisoned(sym("vitseg_hard_loss_scratch_bytes")(B, S))
        if f.get("stats"):
            out["stats"] = poisoned(32)
        if f.get("plane"):
            out["plane"] = poisoned(4 * B * S * S)
        h = _ext.CHardOptions(f.get("gamma", 0.0), f.get("thresh", float("inf")), f.get("min_kept", 0), f.get("q16", 0), 0,
                              hscr.data_ptr(), hscr.numel())
        L.check(sym("vitseg_hard_ce_loss")(*head, out["loss"].data_ptr(), B, C_, g, S, cep, C.byref(h), 0.5,
                                           out["plane"].data_ptr() if "plane" in out else None,
                                           out["stats"].data_ptr() if "stats" in out else None, stream))
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for k in ("loss", "grad", "terms", "stats", "plane"):
        if out.get(k) is not None:
            h.update(out[k].cpu().numpy().tobytes())
    first = out["terms"] if "terms" in out else out["loss"]
    return f"sha256 {h.hexdigest()} loss {float(first.view(torch.float32)[0]):.9g}"


if __name__ == "__main__":
    want = sys.argv[2:]
    for shape in SHAPES:
        for form in FORMS:
            for want_grad in (True, False):
                name = f"{'x'.join(map(str, shape))}_{form}_{'grad' if want_grad else 'nograd'}"
                if want and not any(name.startswith(w) for w in want):
                    continue
                res = run(shape, form, want_grad)
                if res is not None:
                    print(f"{name}: {res}", flush=True)
