"""A class decided by threshold, with hysteresis, on the device.

`curves.ods(...)["threshold"]` is the cut at which a crack model scores best over a data set; this module applies it.  One call
of `vitseg_decide` (csrc/decide.hip, include/vitseg_decide.h) re-generates every pixel's 16-bit score q of class `cls` from the
low-res head output [n, C, g, g] -- `confidence.confidence_map(..., quantised=True)` under a mask that states `cls` everywhere,
the plane `curves.pr_counts` bins, bit for bit -- and writes the uint8 mask of the pixels kept:
  plain cut    q >= high_q;
  hysteresis   q >= low_q, and the pixel hangs together, through pixels with q >= low_q, with one that has q >= high_q
               (skimage.filters.apply_hysteresis_threshold on the host): a faint continuation of a confident crack survives,
               isolated faint speckle does not.
The reference cuts its binary model at a fixed 0.5 (model/PAED/classes.py:308-330) and has no hysteresis.  Everything downstream
(clean, regions, polygons, centerlines) reads the mask alone and works on the decided mask unchanged.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _common, _ext, _lib
from . import confidence as _conf

COUNT_FIELDS = ("weak", "strong", "kept")
Q_ONE = _conf.Q_ONE
Q_NONE = Q_ONE + 1   # a threshold no pixel reaches


def _symbol(name: str):
    return _ext.ext_symbol("decide", name)


def threshold_to_q(t) -> int:
    """The smallest integer q with q / 65535 >= t for a threshold 0 <= t <= 1, the division evaluated in floating point: the
    expression `curves.curve_from_counts` reports its thresholds with, so threshold_to_q(curves.ods(c)["threshold"]) is
    curves.threshold_q(k, bins) exactly.  ValueError for anything but a finite real number in range."""
    if isinstance(t, bool) or not isinstance(t, (int, float, np.integer, np.floating)) or not math.isfinite(float(t)) \
            or not 0.0 <= float(t) <= 1.0:
        raise ValueError(f"a threshold must be a finite number in 0..1, got {t!r}")
    t = float(t)
    q = min(max(int(math.ceil(t * Q_ONE)), 0), Q_ONE)
    while q > 0 and (q - 1) / Q_ONE >= t:
        q -= 1
    while q / Q_ONE < t:   # (t <= 1 = 65535 / 65535: ends at Q_ONE at the latest)
        q += 1
    return q


def check_options(cls=1, threshold=0.5, low=None, connectivity=4, kind="prob", value=None, off=0, high_q=None, low_q=None):
    """The argument checks of `threshold_mask` that need no tensor; returns (high_q, low_q, value).  The thresholds are
    `threshold` / `low` in 0..1 (threshold_to_q) or, instead, the integers `high_q` / `low_q` in 0..65536; without a low one the
    call is the plain cut (low_q == high_q)."""
    _common.integer("cls", cls, 0, 254)
    if kind not in _conf.KINDS:
        raise ValueError(f"kind must be one of {sorted(_conf.KINDS)}, got {kind!r}")
    _common.connectivity(connectivity)
    if high_q is not None:
        hq = _common.integer("high_q", high_q, 0, Q_NONE)
    else:
        hq = threshold_to_q(threshold)
    if low_q is not None and low is not None:
        raise ValueError("give the low threshold as low= or as low_q=, not both")
    if low_q is not None:
        lq = _common.integer("low_q", low_q, 0, Q_NONE)
    else:
        lq = hq if low is None else threshold_to_q(low)
    if lq > hq:
        raise ValueError(f"the low threshold must not exceed the high one, got low_q={lq} > high_q={hq}")
    value = int(cls) if value is None else _common.integer("value", value, 0, 255)
    _common.integer("off", off, 0, 255)
    if value == int(off):
        raise ValueError(f"value and off must differ, got {value} for both")
    return hq, lq, value


def check_model_options(num_classes: int, cls=1, threshold=0.5, low=None, connectivity=4, kind="prob") -> int:
    """`check_options` for a model of `num_classes` classes (model.predict_threshold, predict, the worker, the evaluation
    scripts); returns the mask value of a kept pixel: `cls`, or 1 for a one-class model, whose only class 0 is the foreground
    its ground truth labels 1.  A dropped pixel becomes 0, so class 0 of a many-class model cannot be the one decided."""
    check_options(cls, threshold, low, connectivity, kind, value=1)
    if int(cls) >= int(num_classes):
        raise ValueError(f"the threshold's class must be one of the model's {int(num_classes)} classes, got {cls!r}")
    if kind == "margin" and int(num_classes) < 2:
        raise ValueError("the margin needs at least 2 classes")
    if int(num_classes) > 1 and int(cls) == 0:
        raise ValueError("class 0 is what a pixel the threshold drops becomes: decide one of the classes 1.. by threshold")
    return 1 if int(num_classes) == 1 else int(cls)


def _checked(lowres, base, size, cls, kind):
    """Returns (lowres [n, C, g, g] fp32 contiguous, base [n, S, S] uint8 or None, S, single)."""
    if not isinstance(lowres, torch.Tensor) or lowres.dtype != torch.float32 or lowres.dim() not in (3, 4):
        raise ValueError("lowres must be a float32 tensor [n, C, g, g] or [C, g, g]")
    single = lowres.dim() == 3
    if single:
        lowres = lowres[None]
    n, C, g, g2 = (int(d) for d in lowres.shape)
    if base is not None:
        if isinstance(base, np.ndarray):
            base = torch.from_numpy(base)
        if not isinstance(base, torch.Tensor) or base.dtype != torch.uint8 or base.dim() != (2 if single else 3):
            raise ValueError("base must be a uint8 tensor [n, S, S] ([S, S] with a single lowres)")
        if single:
            base = base[None]
        if int(base.shape[0]) != n or base.shape[1] != base.shape[2]:
            raise ValueError(f"lowres {tuple(lowres.shape)} and base {tuple(base.shape)} must be square and of one batch size")
        if size is not None and int(size) != int(base.shape[-1]):
            raise ValueError(f"size={size!r} contradicts base's side {int(base.shape[-1])}")
        S = int(base.shape[-1])
    else:
        if size is None:
            raise ValueError("give the output side as size= (or a base mask of that side)")
        S = _common.integer("size", size, 1, _conf.MAX_SIDE)
    if g != g2 or not (1 <= C <= 255 and 1 <= n <= _conf.MAX_BATCH and 1 <= S <= _conf.MAX_SIDE and 1 <= g <= S):
        raise ValueError(f"threshold_mask takes 1..255 classes, 1..{_conf.MAX_BATCH} images and square maps with "
                         f"1 <= g <= S <= {_conf.MAX_SIDE}, got lowres {tuple(lowres.shape)} and S={S}")
    if int(cls) >= C:
        raise ValueError(f"cls must be one of the {C} classes of lowres, got {cls!r}")
    if kind == "margin" and C < 2:
        raise ValueError("the margin needs at least 2 classes")
    if not lowres.is_cuda:
        raise RuntimeError("threshold_mask runs on the MI355X only: lowres must be a device tensor (there is no CPU fallback)")
    return lowres.contiguous(), None if base is None else base.to(lowres.device).contiguous(), S, single


@torch.no_grad()
def threshold_mask(lowres, cls: int = 1, threshold=0.5, low=None, connectivity: int = 4, kind: str = "prob", base=None,
                   value: Optional[int] = None, off: int = 0, return_counts: bool = False, *, size: Optional[int] = None,
                   high_q: Optional[int] = None, low_q: Optional[int] = None):
    """The mask of class `cls` decided by threshold under the low-res head output `lowres` (fp32 device tensor [n, C, g, g] or
    [C, g, g]; g == S: full-size logits as they stand): a uint8 device tensor [n, S, S] ([S, S] for a single image), S = `size`
    or `base`'s side.  A pixel is kept when its score (`kind`: "prob" or "margin", as in confidence.confidence_map) reaches
    `threshold`; with `low` it is kept when it reaches `low` and is `connectivity`-connected, through pixels that reach `low`,
    to one that reaches `threshold`.  `high_q` / `low_q` give the thresholds as 16-bit integers instead (0..65536).  Kept pixels
    become `value` (default: cls), the others `off`, or, with `base` (uint8 [n, S, S]), what base states there -- except that
    a base pixel equal to `value` becomes `off`: class `value` is decided by this rule, every other class by whoever wrote base.
    `return_counts`: (mask, int64 numpy [n, 3] of (weak, strong, kept) pixels per image), the only host synchronisation.
    One stream; there is no CPU fallback."""
    hq, lq, value = check_options(cls, threshold, low, connectivity, kind, value, off, high_q, low_q)
    lowres, base, S, single = _checked(lowres, base, size, cls, kind)
    n, C, g, _ = (int(d) for d in lowres.shape)
    dev = lowres.device
    mask = torch.empty((n, S, S), dtype=torch.uint8, device=dev)
    counts = torch.empty((n, 3), dtype=torch.int64, device=dev) if return_counts else None
    with torch.cuda.device(dev):
        nbytes = _symbol("vitseg_decide_scratch_bytes")(n, S, int(lq != hq))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        _lib.check(_symbol("vitseg_decide")(
            lowres.data_ptr(), n, C, g, S, int(cls), _conf.KINDS[kind], hq, lq, int(connectivity),
            None if base is None else base.data_ptr(), value, int(off), mask.data_ptr(),
            None if counts is None else counts.data_ptr(), None if scratch is None else scratch.data_ptr(), nbytes,
            torch.cuda.current_stream().cuda_stream))
    out = mask[0] if single else mask
    if return_counts:
        c = counts.cpu().numpy()
        return out, (c[0] if single else c)
    return out


def add_arguments(ap) -> None:
    """--threshold / --threshold-low / --threshold-class / --threshold-connectivity / --threshold-over-argmax of the worker
    and the evaluation scripts (the score's kind is their --threshold-kind / --score-kind)."""
    ap.add_argument("--threshold", type=float, metavar="T",
                    help="decide --threshold-class by its score instead of the argmax: a pixel is kept when its score "
                         "reaches T (0..1, e.g. the ODS threshold of <model>_pr_curve.csv); every mask is then that one, "
                         "before --min-area / --fill-holes")
    ap.add_argument("--threshold-low", type=float, metavar="L",
                    help="hysteresis: also keep a pixel that reaches L (<= T) and hangs together, through such pixels, with one "
                         "that reaches T")
    ap.add_argument("--threshold-class", type=int, default=1, metavar="C", help="the class --threshold decides (default 1)")
    ap.add_argument("--threshold-connectivity", type=int, default=4, choices=[4, 8], help="how --threshold-low's pixels hang together")
    ap.add_argument("--threshold-over-argmax", action="store_true",
                    help="keep the argmax mask's other classes: only --threshold-class is decided by the threshold, and a pixel "
                         "the argmax gave to it but the threshold drops becomes 0 (default: a mask of that class and 0 alone)")


__all__ = ["threshold_mask", "threshold_to_q", "check_options", "check_model_options", "add_arguments", "COUNT_FIELDS", "Q_ONE",
           "Q_NONE"]
