"""Confidence of a predicted mask, on the device: a score per pixel, a score row per region and a calibration histogram.

The quantity is the reference's own: its scripts decide by `logits.sigmoid()` followed by `argmax`
(model/CE/testViTModel.py:122-126), and the score is the sigmoid that won.  One launch of `vitseg_confidence`
(csrc/confidence.hip) re-generates every pixel's logits from the low-resolution head output [n, C, g, g] with the decoder
tail's exact arithmetic, so the full-size logits are never written, and returns
  * p = sigmoid(v_c) of the class c the mask states ("prob"), or its lead over the best other class ("margin"), as fp32 or as
    q = rint(p * 65535);
  * per region of `vitseg_regions` the int64 row (pixels, sum_q, max_deficit, n_low);
  * per image and confidence bin the int64 row (pixels, pixels with mask == gt, sum_q).
Everything the device returns is an integer or a single-rounded fp32 value; the ratios (mean score, accuracy, ECE, AP) are
host arithmetic on the integers: `scores_from_rows`, `calibration_from_hist`, `average_precision`.
"""
from __future__ import annotations

import math
from typing import List, Optional

import numpy as np
import torch

from . import _common, _lib
from . import regions as _regions

KINDS = {"prob": _lib.CONF_PROB, "margin": _lib.CONF_MARGIN}
SCORE_FIELDS = ("pixels", "sum_q", "max_deficit", "n_low")
HIST_FIELDS = ("pixels", "correct", "sum_q")
Q_ONE = 65535   # q of p = 1
MAX_SIDE, MAX_BATCH, MAX_BINS = 16384, 65535, 256


def low_to_q(low) -> int:
    """The `low_q` of a threshold 0 <= low <= 1: a pixel is "low" when q < low_q, i.e. when its 16-bit score lies below
    `low` (low = 0: no pixel; 65536 is reached by no threshold, every pixel then counts)."""
    if isinstance(low, bool) or not isinstance(low, (int, float, np.integer, np.floating)) or not 0.0 <= float(low) <= 1.0:
        raise ValueError(f"low must be a number in 0..1, got {low!r}")
    return int(math.ceil(float(low) * Q_ONE))


def _checked(lowres, mask, kind):
    """Validates what every device call shares; returns (lowres [n, C, g, g] fp32, mask [n, S, S] uint8, single)."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {sorted(KINDS)}, got {kind!r}")
    if not isinstance(lowres, torch.Tensor) or lowres.dtype != torch.float32 or lowres.dim() not in (3, 4):
        raise ValueError("lowres must be a float32 tensor [n, C, g, g] or [C, g, g]")
    if isinstance(mask, np.ndarray):
        mask = torch.from_numpy(mask)
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.dim() not in (2, 3):
        raise ValueError("mask must be a uint8 tensor [n, S, S] or [S, S]")
    single = mask.dim() == 2
    if single != (lowres.dim() == 3):
        raise ValueError(f"lowres {tuple(lowres.shape)} and mask {tuple(mask.shape)} must both be batched or both single")
    if single:
        lowres, mask = lowres[None], mask[None]
    n, C, g, g2 = (int(d) for d in lowres.shape)
    S = int(mask.shape[-1])
    if g != g2 or mask.shape[1] != mask.shape[2] or int(mask.shape[0]) != n:
        raise ValueError(f"lowres {tuple(lowres.shape)} and mask {tuple(mask.shape)} must be square and of one batch size")
    if not (1 <= C <= 255 and 1 <= n <= MAX_BATCH and 1 <= S <= MAX_SIDE and 1 <= g <= S):
        raise ValueError(f"confidence takes 1..255 classes, 1..{MAX_BATCH} images and 1 <= g <= S <= {MAX_SIDE}, got n={n} "
                         f"C={C} g={g} S={S}")
    if kind == "margin" and C < 2:
        raise ValueError("the margin needs at least 2 classes")
    if not lowres.is_cuda:
        raise RuntimeError("confidence runs on the MI355X only: lowres must be a device tensor (there is no CPU fallback)")
    return lowres.contiguous(), mask.to(lowres.device).contiguous(), single


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _launch(lowres, mask, kind, conf=None, conf_q=None, labels=None, scores=None, low_q=0, gt=None, ignore_label=-1, hist=None):
    """One vitseg_confidence call on the current stream of lowres' device (no host sync)."""
    n, C, g, _ = (int(d) for d in lowres.shape)
    S = int(mask.shape[-1])
    with torch.cuda.device(lowres.device):
        _lib.check(_lib.symbol("vitseg_confidence")(
            lowres.data_ptr(), mask.data_ptr(), n, C, g, S, KINDS[kind], _ptr(conf), _ptr(conf_q), _ptr(labels), _ptr(scores),
            0 if scores is None else int(scores.shape[1]), int(low_q), _ptr(gt), int(ignore_label), _ptr(hist),
            0 if hist is None else int(hist.shape[1]), torch.cuda.current_stream().cuda_stream))


@torch.no_grad()
def confidence_map(lowres, mask, kind: str = "prob", quantised: bool = False):
    """The score of every pixel of `mask` (uint8 [n, S, S] or [S, S]) under the low-res head output `lowres` (fp32 device
    tensor [n, C, g, g] or [C, g, g]; g == S: full-size logits as they stand): fp32 p, or with `quantised` the int-valued
    q = rint(p * 65535) as a uint16 tensor.  kind "prob": the sigmoid of the class the mask states -- on the decoder tail's
    own mask `logits.sigmoid().max(dim=1).values`; "margin": its lead over the best other class, 0 where the stated class
    did not win.  A mask value >= C scores 0.  One launch, no host sync."""
    lowres, mask, single = _checked(lowres, mask, kind)
    out = torch.empty(mask.shape, dtype=torch.uint16 if quantised else torch.float32, device=lowres.device)
    _launch(lowres, mask, kind, **({"conf_q": out} if quantised else {"conf": out}))
    return out[0] if single else out


@torch.no_grad()
def region_scores(lowres, mask, kind: str = "prob", low: float = 0.5, background: int = 0, connectivity: int = 4):
    """The regions of `mask` (regions.region_boxes' records, same order) with one score row each: per image (records int32
    [k, 7], rows int64 [k, 4]) -- lists for a batch, the pair of arrays for a single image.  A row is (pixels, sum_q,
    max_deficit, n_low): the region's area, the sum of its pixels' q, 65535 minus its smallest q, and the pixels with
    p below `low`; `scores_from_rows` turns it into ratios.  vitseg_regions (with labels) and vitseg_confidence are enqueued
    on one stream; the only host sync is the read of the counts (an image with more than regions.DEFAULT_MAX_REGIONS regions
    makes one more pair of calls sized to the largest count: the same bits)."""
    lowres, mask, single = _checked(lowres, mask, kind)
    low_q = low_to_q(low)
    _regions._checked(mask, background, connectivity)
    background = int(background)

    def run(max_regions):
        counts, recs, labels = _regions._launch(mask, background, connectivity, max_regions, True)
        rows = torch.empty((mask.shape[0], max_regions, 4), dtype=torch.int64, device=mask.device)
        _launch(lowres, mask, kind, labels=labels, scores=rows, low_q=low_q)
        return counts, recs, rows

    counts, recs, rows = run(_regions.DEFAULT_MAX_REGIONS)
    cnt = counts.cpu().numpy()
    if int(cnt.max()) > _regions.DEFAULT_MAX_REGIONS:
        counts, recs, rows = run(int(cnt.max()))
    k = int(cnt.max())
    rec, row = recs[:, :k, :7].cpu().numpy(), rows[:, :k].cpu().numpy()
    out_r = [np.ascontiguousarray(rec[i, :int(cnt[i])]) for i in range(len(cnt))]
    out_s = [np.ascontiguousarray(row[i, :int(cnt[i])]) for i in range(len(cnt))]
    return (out_r[0], out_s[0]) if single else (out_r, out_s)


@torch.no_grad()
def calibration_hist(lowres, mask, gt, bins: int = 16, ignore_label: Optional[int] = None, kind: str = "prob"):
    """The reliability counts of `mask` against the ground truth `gt` (uint8, mask's shape): int64 numpy [n, bins, 3] ([bins,
    3] for a single image), per image and confidence bin (q * bins) >> 16 the (pixels, pixels with mask == gt, sum_q).
    Pixels with gt == ignore_label are void.  Pool images by adding the arrays, then `calibration_from_hist`."""
    lowres, mask, single = _checked(lowres, mask, kind)
    _common.integer("bins", bins, 1, MAX_BINS)
    if ignore_label is not None and not _common.is_integer(ignore_label, 0, 255):
        raise ValueError(f"ignore_label must be None or an integer in 0..255, got {ignore_label!r}")
    if isinstance(gt, np.ndarray):
        gt = torch.from_numpy(gt)
    if not isinstance(gt, torch.Tensor) or gt.dtype != torch.uint8:
        raise ValueError("gt must be a uint8 tensor of the mask's shape")
    if single and gt.dim() == 2:
        gt = gt[None]
    if tuple(gt.shape) != tuple(mask.shape):
        raise ValueError(f"gt {tuple(gt.shape)} must have the mask's shape {tuple(mask.shape)}")
    gt = gt.to(lowres.device).contiguous()
    hist = torch.empty((mask.shape[0], int(bins), 3), dtype=torch.int64, device=lowres.device)
    _launch(lowres, mask, kind, gt=gt, ignore_label=-1 if ignore_label is None else int(ignore_label), hist=hist)
    out = hist.cpu().numpy()
    return out[0] if single else out


# ---- host arithmetic on the integers ----

def scores_from_rows(rows) -> List[dict]:
    """One dict per score row (int64 [k, 4]): score = sum_q / (65535 pixels), the region's mean p; score_min =
    (65535 - max_deficit) / 65535, its least confident pixel; low_fraction = n_low / pixels.  A row without pixels: nan."""
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] != len(SCORE_FIELDS):
        raise ValueError(f"rows must be [k, {len(SCORE_FIELDS)}], got {rows.shape}")
    nan = float("nan")
    out = []
    for px, sq, md, nl in ((int(v) for v in r) for r in rows):
        if px <= 0:
            out.append({"pixels": px, "score": nan, "score_min": nan, "low_fraction": nan})
        else:
            out.append({"pixels": px, "score": sq / (Q_ONE * px), "score_min": (Q_ONE - md) / Q_ONE, "low_fraction": nl / px})
    return out


def calibration_from_hist(hist) -> dict:
    """The reliability table and the expected calibration error of a histogram int64 [bins, 3], or of several [..., bins, 3]
    pooled by integer addition BEFORE the ratios are taken: {"n": per-bin pixels, "accuracy": correct / n, "confidence":
    sum_q / (65535 n) (nan for an empty bin), "total": N, "ece": sum_b n_b / N |accuracy_b - confidence_b| over the non-empty
    bins (nan when N = 0)}."""
    h = np.asarray(hist)
    if h.ndim < 2 or h.shape[-1] != len(HIST_FIELDS) or not np.issubdtype(h.dtype, np.integer):
        raise ValueError(f"hist must be an integer array [..., bins, {len(HIST_FIELDS)}], got {h.dtype} {h.shape}")
    h = h.reshape(-1, h.shape[-2], 3).astype(np.int64).sum(axis=0)
    nan = float("nan")
    n = [int(v) for v in h[:, 0]]
    acc = [int(c) / k if k else nan for c, k in zip(h[:, 1], n)]
    conf = [int(s) / (Q_ONE * k) if k else nan for s, k in zip(h[:, 2], n)]
    N = sum(n)
    ece = sum(k / N * abs(a - c) for k, a, c in zip(n, acc, conf) if k) if N else nan
    return {"n": n, "accuracy": acc, "confidence": conf, "total": N, "ece": ece}


def average_precision(scores, matched, n_gt: int) -> float:
    """AP of ranked detections: `scores` (any real numbers), `matched` (1 / True: the detection is a true positive), n_gt true
    objects.  Detections are sorted by score, descending; detections of equal score enter as ONE group (their order cannot
    matter); precision is replaced by its running maximum from the right (all-point interpolation) and
    AP = sum_k (R_k - R_{k-1}) P_k.  nan when n_gt == 0; 0 without detections."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    m = np.asarray(matched).reshape(-1).astype(bool)
    if s.shape != m.shape:
        raise ValueError(f"scores {s.shape} and matched {m.shape} must have one length")
    if isinstance(n_gt, bool) or not isinstance(n_gt, (int, np.integer)) or int(n_gt) < 0:
        raise ValueError(f"n_gt must be a non-negative integer, got {n_gt!r}")
    if np.isnan(s).any():
        raise ValueError("scores must not hold nan")
    n_gt = int(n_gt)
    if n_gt == 0:
        return float("nan")
    if int(m.sum()) > n_gt:
        raise ValueError(f"{int(m.sum())} matched detections but only {n_gt} true objects")
    order = np.argsort(-s, kind="stable")
    s, m = s[order], m[order]
    ends = np.flatnonzero(np.append(s[1:] != s[:-1], True)) if len(s) else np.zeros(0, dtype=np.int64)   # last of each group
    tp = np.cumsum(m)[ends]
    recall = tp / n_gt
    precision = tp / (ends + 1)
    precision = np.maximum.accumulate(precision[::-1])[::-1]
    return float(np.sum(np.diff(np.concatenate(([0.0], recall))) * precision))


# ---- the evaluation scripts' files ----

SCORES_CSV_COLUMNS = ["Model_ID", "Model_Name", "Batch_Num", "Image_Idx", "Region", "Class", "First", "Area", "Score", "Score_Min",
                      "Low_Fraction", "Matched", "AP", "N_GT"]   # the last two: the pooled row of a class (Batch_Num "pooled")
CALIBRATION_CSV_COLUMNS = ["Model_ID", "Model_Name", "Bin", "Lower", "Upper", "Pixels", "Accuracy", "Confidence", "ECE"]


def calibration_csv_rows(model_info, hist, bins: int) -> List[list]:
    """The rows of <model>_calibration.csv from the pooled histogram int64 [bins, 3]: one per bin (its score range, pixels,
    accuracy, mean confidence), then the "all" row with the pixel total and the ECE."""
    cal = calibration_from_hist(np.zeros((bins, 3), np.int64) if hist is None else hist)
    rows = [[model_info[0], model_info[1], b, b / bins, (b + 1) / bins, cal["n"][b], cal["accuracy"][b], cal["confidence"][b], ""]
            for b in range(bins)]
    rows.append([model_info[0], model_info[1], "all", 0.0, 1.0, cal["total"], "", "", cal["ece"]])
    return rows


def region_dicts(records, rows) -> List[dict]:
    """One dict per region of one image from `region_scores`' pair: class, first, area, score, score_min, low_fraction."""
    return [{"class": int(r[0]), "first": int(r[6]), "area": int(r[5]), "score": d["score"], "score_min": d["score_min"],
             "low_fraction": d["low_fraction"]} for r, d in zip(np.asarray(records), scores_from_rows(rows))]
