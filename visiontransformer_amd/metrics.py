"""Evaluation metrics on the device.

The reference's evaluation script (model/CE/datasetTestViTmodel.py:152-227) pulls every prediction to the host and
loops over classes in numpy to get, per image: pixel accuracy (%), mean IoU and mean Dice over the classes present
(nan-aware), and the sets of ground-truth / predicted / missing / false-positive classes, written to
`<model>_metrics.csv`.  Here one kernel (`vitseg_eval_counts`) reduces each (prediction, ground truth) pair to
integer class statistics on the GPU -- the ground truth is nearest-resized on the fly exactly as
`Image.fromarray(gt).resize(pred.shape[::-1], Image.NEAREST)` does -- and the metrics follow from those integers with
the reference's own formulas, so the CSV is identical (tests/test_preproc_cpu.py, tests/test_gpu_preproc.py).

Boundary distances (`Evaluator.distance_metrics`): how far a predicted region lies from the true one.  The reference's PAED
(pixel average Euclidean distance, model/PAED/classes.py:209-258) is two Python loops over all pixel pairs and was left
switched off; `vitseg_distance_stats` (csrc/distance.hip) gets the same sums from two exact distance transforms and a masked
reduction per class, together with the integers behind the Hausdorff distance, its percentiles (HD95, pooled as MedPy's
`hd95`) and the average symmetric distance.  `distances_from_stats` is the host arithmetic on those numbers.

Cracks (`Evaluator.crack_metrics`): structures one to five pixels wide, for which the overlap metrics barely register whether
the crack's course was found.  `vitseg_skeleton_stats` (csrc/skeleton.hip) thins the class sets of both maps to their
Zhang-Suen skeletons and counts what centre-line Dice (clDice), the crack length and the crack width need;
`crack_from_stats` is the host arithmetic.
"""
from __future__ import annotations

import csv
import ctypes
import math
import warnings
from fractions import Fraction
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .preprocess import NEAREST_PIL, nearest_table

# header of <model>_metrics.csv (datasetTestViTmodel.py:166-171); compareModels.py:27-47 reads these columns
CSV_COLUMNS = ["Model_ID", "Model_Name", "Patch_Size", "Hidden_Size", "Layers", "Heads", "Batch_Num", "Image_Idx",
               "Accuracy", "Mean_IoU", "Mean_Dice", "Inference_Time", "GT_Classes", "Pred_Classes", "Missing_Classes",
               "False_Positive_Classes"]


def metrics_from_counts(counts: np.ndarray, num_classes: int, total_pixels: int) -> dict:
    """counts: int64 [3, 256] of one image (|gt & pred|, |gt|, |pred| per label value) -> the metric columns of one
    CSV row, with the reference's arithmetic (datasetTestViTmodel.py:193-219)."""
    inter, ngt, npr = (counts[i] for i in range(3))
    mism = int(total_pixels - int(inter.sum()))
    acc = 100 * (1 - mism / total_pixels)
    ious, dices = [], []
    for c in range(num_classes):
        i, union, size = inter[c], ngt[c] + npr[c] - inter[c], ngt[c] + npr[c]
        ious.append(float("nan") if union == 0 else i / union)
        dices.append(float("nan") if size == 0 else 2 * i / size)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # all-nan (no class present) -> nan, as in the reference
        miou, mdice = float(np.nanmean(ious)), float(np.nanmean(dices))
    gtc = [int(v) for v in np.nonzero(ngt)[0]]
    prc = [int(v) for v in np.nonzero(npr)[0]]
    return dict(Accuracy=acc, Mean_IoU=miou, Mean_Dice=mdice, GT_Classes=gtc, Pred_Classes=prc,
                Missing_Classes=sorted(set(gtc) - set(prc)), False_Positive_Classes=sorted(set(prc) - set(gtc)),
                ious=ious, dices=dices)


DISTANCE_MODES = {"sets": 0, "borders": 1}
DISTANCE_KEYS = ("paed", "hausdorff", "hd_percentile", "assd", "mean_AP", "mean_PA")
# header of <model>_distance_metrics.csv (--distance-metrics of the evaluation scripts): the nan-aware class means per image
DISTANCE_CSV_COLUMNS = ["Model_ID", "Model_Name", "Batch_Num", "Image_Idx", "Mode", "Percentile", "Mean_PAED",
                        "Mean_Hausdorff", "Mean_HD_Percentile", "Mean_ASSD", "Per_Class"]


def percentile_fraction(percentile):
    """A percentile 0..100 as the rational (pct_num, pct_den) of vitseg_distance_stats: 95 -> (19, 20), 99.5 -> (199, 200).
    ValueError outside 0..100 or when the denominator would pass 1000."""
    f = Fraction(str(percentile)) / 100
    if not 0 <= f <= 1 or f.denominator > 1000:
        raise ValueError(f"percentile must lie in 0..100 with at most one decimal, got {percentile!r}")
    return f.numerator, f.denominator


def distances_from_stats(stats_i, stats_f, pct_num: int, pct_den: int) -> list:
    """stats_i int64 [n, K, 6] and stats_f float64 [n, K, 2] of vitseg_distance_stats (include/vitseg.h) -> per image a list of
    K dicts.  A = the ground truth's pixels of the class (n of them), P = the prediction's (m):
      paed           the reference's formula (model/PAED/classes.py:228-254): 0 when both are empty, the sum / count of the
                     other when one is, else (sumAP + sumPA + 0.001) / (n + m + 0.001)
      hausdorff      sqrt(max(max_d2_AP, max_d2_PA))
      hd_percentile  np.percentile of the pooled distances at pct_num / pct_den, from the two order statistics
      assd           (sumAP + sumPA) / (n + m)
      mean_AP, mean_PA  the directed means sumAP / n, sumPA / m
    and n, m.  Everything but paed is nan when either set is empty (no distance is defined)."""
    si = np.asarray(stats_i, dtype=np.int64)
    sf = np.asarray(stats_f, dtype=np.float64)
    if si.ndim != 3 or si.shape[2] != 6 or sf.shape != si.shape[:2] + (2,):
        raise ValueError(f"stats_i must be [n, K, 6] and stats_f [n, K, 2], got {si.shape} and {sf.shape}")
    if not (0 <= pct_num <= pct_den and 1 <= pct_den <= 1000):
        raise ValueError(f"percentile {pct_num} / {pct_den} outside 0 <= num <= den <= 1000")
    nan = float("nan")
    out = []
    for i in range(si.shape[0]):
        row = []
        for k in range(si.shape[1]):
            n, m, mx_ap, mx_pa, lo2, hi2 = (int(v) for v in si[i, k])
            s_ap, s_pa = float(sf[i, k, 0]), float(sf[i, k, 1])
            d = dict(n=n, m=m, hausdorff=nan, hd_percentile=nan, assd=nan, mean_AP=nan, mean_PA=nan)
            if n == 0 and m == 0:
                d["paed"] = 0.0
            elif n == 0:
                d["paed"] = s_pa / m
            elif m == 0:
                d["paed"] = s_ap / n
            else:
                d["paed"] = (s_ap + s_pa + 0.001) / (n + m + 0.001)
                d["hausdorff"] = math.sqrt(max(mx_ap, mx_pa))
                frac = (pct_num * (n + m - 1) % pct_den) / pct_den
                lo, hi = math.sqrt(lo2), math.sqrt(hi2)
                d["hd_percentile"] = lo + (hi - lo) * frac
                d["assd"] = (s_ap + s_pa) / (n + m)
                d["mean_AP"], d["mean_PA"] = s_ap / n, s_pa / m
            row.append(d)
        out.append(row)
    return out


CRACK_KEYS = ("cldice", "cl_precision", "cl_sensitivity", "length_gt", "length_pred", "mean_width_gt", "mean_width_pred",
              "max_width_gt", "max_width_pred", "endpoints_gt", "endpoints_pred")
# header of <model>_crack_metrics.csv (--crack-metrics of the evaluation scripts): the nan-aware class means per image
CRACK_CSV_COLUMNS = ["Model_ID", "Model_Name", "Batch_Num", "Image_Idx", "Mean_clDice", "Mean_CL_Precision",
                     "Mean_CL_Sensitivity", "Mean_Length_GT", "Mean_Length_Pred", "Mean_Width_GT", "Mean_Width_Pred",
                     "Per_Class"]


def crack_from_stats(stats_i, stats_f) -> list:
    """stats_i int64 [n, K, 10] and stats_f float64 [n, K, 2] of vitseg_skeleton_stats (include/vitseg.h) -> per image a list
    of K dicts.  G = the ground truth's pixels of the class, P = the prediction's, S_X the skeleton of X:
      cl_precision    |S_P n G| / |S_P|: how much of the predicted centre line lies inside the true crack
      cl_sensitivity  |S_G n P| / |S_G|: how much of the true centre line the prediction covers
      cldice          their harmonic mean (0 when both are 0)
      length_gt, length_pred          |S_G|, |S_P|: the crack length in pixels
      mean_width_gt, mean_width_pred  2 sum sqrt(d2) / |S| - 1: twice the mean distance from the centre line to the edge
      max_width_gt, max_width_pred    2 sqrt(max d2) - 1
      endpoints_gt, endpoints_pred    skeleton pixels with exactly one set 8-neighbour
    and n = |G|, m = |P|.  A ratio whose denominator is 0 is nan, and cldice with it."""
    si = np.asarray(stats_i, dtype=np.int64)
    sf = np.asarray(stats_f, dtype=np.float64)
    if si.ndim != 3 or si.shape[2] != 10 or sf.shape != si.shape[:2] + (2,):
        raise ValueError(f"stats_i must be [n, K, 10] and stats_f [n, K, 2], got {si.shape} and {sf.shape}")
    nan = float("nan")
    out = []
    for i in range(si.shape[0]):
        row = []
        for k in range(si.shape[1]):
            n, m, sg, sp, sg_p, sp_g, mx_g, mx_p, e_g, e_p = (int(v) for v in si[i, k])
            prec = sp_g / sp if sp else nan
            sens = sg_p / sg if sg else nan
            if not (sp and sg):
                cld = nan
            else:
                cld = 2 * prec * sens / (prec + sens) if prec + sens > 0 else 0.0
            row.append(dict(n=n, m=m, cldice=cld, cl_precision=prec, cl_sensitivity=sens, length_gt=sg, length_pred=sp,
                            mean_width_gt=2 * float(sf[i, k, 0]) / sg - 1 if sg else nan,
                            mean_width_pred=2 * float(sf[i, k, 1]) / sp - 1 if sp else nan,
                            max_width_gt=2 * math.sqrt(mx_g) - 1 if sg else nan,
                            max_width_pred=2 * math.sqrt(mx_p) - 1 if sp else nan,
                            endpoints_gt=e_g, endpoints_pred=e_p))
        out.append(row)
    return out


class Evaluator:
    """Per-image metrics of uint8 predictions [n, S, S] against label maps of any size, counted on the GPU."""

    def __init__(self, num_classes: int, device="cuda:0"):
        self.num_classes = int(num_classes)
        self.device = torch.device(device)
        self._near: Dict[tuple, torch.Tensor] = {}

    def _nearest(self, in_size: int, out_size: int) -> torch.Tensor:
        key = (in_size, out_size)
        if key not in self._near:
            self._near[key] = torch.from_numpy(nearest_table(in_size, out_size, NEAREST_PIL)).to(self.device)
        return self._near[key]

    def counts(self, pred: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
        """int64 [n, 3, 256] class statistics (device tensor)."""
        if pred.dtype != torch.uint8 or pred.dim() != 3 or pred.shape[1] != pred.shape[2]:
            raise ValueError(f"pred must be uint8 [n, S, S], got {pred.dtype} {tuple(pred.shape)}")
        if gt.dim() != 3 or gt.shape[0] != pred.shape[0]:
            raise ValueError("Number of images and masks must be equal!")  # the reference's dataset check, classes.py:34-35
        pred = pred.to(self.device).contiguous()
        gt = gt.to(self.device).to(torch.uint8).contiguous()   # astype(np.uint8) in the reference (:195)
        n, S, _ = pred.shape
        Hg, Wg = gt.shape[1:]
        same = (Hg, Wg) == (S, S)
        yi = None if same else self._nearest(Hg, S)
        xi = None if same else self._nearest(Wg, S)
        out = torch.empty((n, 3, 256), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().vitseg_eval_counts(pred.data_ptr(), gt.data_ptr(), n, S, Hg, Wg,
                                                     None if yi is None else yi.data_ptr(),
                                                     None if xi is None else xi.data_ptr(), out.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream))
        return out

    def distance_stats(self, pred: torch.Tensor, gt: torch.Tensor, classes: Sequence[int], mode: int, pct_num: int,
                       pct_den: int):
        """(stats_i int64 [n, K, 6], stats_f float64 [n, K, 2]) device tensors of vitseg_distance_stats for uint8 predictions
        [n, H, W]; a ground truth of another size is nearest-resized first, as `counts` does on the fly."""
        if pred.dtype != torch.uint8 or pred.dim() != 3:
            raise ValueError(f"pred must be uint8 [n, H, W], got {pred.dtype} {tuple(pred.shape)}")
        if gt.dim() != 3 or gt.shape[0] != pred.shape[0]:
            raise ValueError("Number of images and masks must be equal!")
        classes = [int(c) for c in classes]
        if not classes or len(classes) > 256 or any(not 0 <= c <= 255 for c in classes):
            raise ValueError(f"classes must be 1..256 label values in 0..255, got {classes}")
        pred = pred.to(self.device).contiguous()
        gt = gt.to(self.device).to(torch.uint8).contiguous()
        n, H, W = (int(d) for d in pred.shape)
        K = len(classes)
        cls = (ctypes.c_int32 * K)(*classes)
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream().cuda_stream
            if tuple(gt.shape[1:]) != (H, W):
                Hg, Wg = (int(d) for d in gt.shape[1:])
                g2 = torch.empty((n, H, W), dtype=torch.uint8, device=self.device)
                _lib.check(_lib.lib().vitseg_resize_nearest_u8(gt.data_ptr(), n, Hg, Wg, self._nearest(Hg, H).data_ptr(),
                                                               self._nearest(Wg, W).data_ptr(), H, W, None, 0, g2.data_ptr(),
                                                               st))
                gt = g2
            nbytes = _lib.distance_symbol("vitseg_distance_scratch_bytes")(n, H, W)
            if nbytes == 0:
                raise ValueError(f"distance metrics: H and W must lie in 1..16384 and n in 1..32767, got {n} x {H} x {W}")
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            si = torch.empty((n, K, 6), dtype=torch.int64, device=self.device)
            sf = torch.empty((n, K, 2), dtype=torch.float64, device=self.device)
            _lib.check(_lib.distance_symbol("vitseg_distance_stats")(pred.data_ptr(), gt.data_ptr(), n, H, W, cls, K, int(mode),
                                                                     int(pct_num), int(pct_den), si.data_ptr(), sf.data_ptr(),
                                                                     scratch.data_ptr(), nbytes, st))
        return si, sf

    def distance_metrics(self, pred: torch.Tensor, gt: torch.Tensor, classes: Optional[Sequence[int]] = None,
                         mode: str = "sets", percentile=95) -> List[dict]:
        """Per image: dict(per_class={class: the dict of `distances_from_stats`}, paed=, hausdorff=, hd_percentile=, assd=,
        mean_AP=, mean_PA= the nan-aware means over the classes).  mode "sets": distances between the whole pixel sets of a
        class (the reference's PAED); "borders": between their 4-neighbour borders (the surface form of MedPy's hd / hd95 /
        assd).  classes=None: range(num_classes).  percentile: 0..100, at most one decimal (95 = HD95)."""
        if mode not in DISTANCE_MODES:
            raise ValueError(f"mode must be one of {sorted(DISTANCE_MODES)}, got {mode!r}")
        num, den = percentile_fraction(percentile)
        classes = list(range(self.num_classes)) if classes is None else [int(c) for c in classes]
        si, sf = self.distance_stats(pred, gt, classes, DISTANCE_MODES[mode], num, den)
        rows = distances_from_stats(si.cpu().numpy(), sf.cpu().numpy(), num, den)
        out = []
        for row in rows:
            d = dict(per_class=dict(zip(classes, row)))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)   # all-nan -> nan, as the overlap means
                for key in DISTANCE_KEYS:
                    d[key] = float(np.nanmean([r[key] for r in row]))
            out.append(d)
        return out

    def skeleton_stats(self, pred: torch.Tensor, gt: torch.Tensor, classes: Sequence[int], route: int = 0):
        """(stats_i int64 [n, K, 10], stats_f float64 [n, K, 2]) device tensors of vitseg_skeleton_stats for uint8 predictions
        [n, H, W]; a ground truth of another size is nearest-resized first, as `distance_stats` does.  One enqueue on the
        current stream; planes too large for the resident route (see skeleton.py) synchronise it."""
        if pred.dtype != torch.uint8 or pred.dim() != 3:
            raise ValueError(f"pred must be uint8 [n, H, W], got {pred.dtype} {tuple(pred.shape)}")
        if gt.dim() != 3 or gt.shape[0] != pred.shape[0]:
            raise ValueError("Number of images and masks must be equal!")
        classes = [int(c) for c in classes]
        if not classes or len(classes) > 256 or any(not 0 <= c <= 255 for c in classes):
            raise ValueError(f"classes must be 1..256 label values in 0..255, got {classes}")
        pred = pred.to(self.device).contiguous()
        gt = gt.to(self.device).to(torch.uint8).contiguous()
        n, H, W = (int(d) for d in pred.shape)
        K = len(classes)
        cls = (ctypes.c_int32 * K)(*classes)
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream().cuda_stream
            if tuple(gt.shape[1:]) != (H, W):
                Hg, Wg = (int(d) for d in gt.shape[1:])
                g2 = torch.empty((n, H, W), dtype=torch.uint8, device=self.device)
                _lib.check(_lib.lib().vitseg_resize_nearest_u8(gt.data_ptr(), n, Hg, Wg, self._nearest(Hg, H).data_ptr(),
                                                               self._nearest(Wg, W).data_ptr(), H, W, None, 0, g2.data_ptr(),
                                                               st))
                gt = g2
            nbytes = _lib.skeleton_symbol("vitseg_skeleton_stats_scratch_bytes")(n, H, W, int(route))
            if nbytes == 0:
                raise ValueError(f"crack metrics: H and W must lie in 1..16384 and n in 1..32767 (and the plane must fit the "
                                 f"route asked for), got {n} x {H} x {W}, route {route}")
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            si = torch.empty((n, K, 10), dtype=torch.int64, device=self.device)
            sf = torch.empty((n, K, 2), dtype=torch.float64, device=self.device)
            _lib.check(_lib.skeleton_symbol("vitseg_skeleton_stats")(pred.data_ptr(), gt.data_ptr(), n, H, W, cls, K,
                                                                     int(route), si.data_ptr(), sf.data_ptr(),
                                                                     scratch.data_ptr(), nbytes, st))
        return si, sf

    def crack_metrics(self, pred: torch.Tensor, gt: torch.Tensor, classes: Optional[Sequence[int]] = None) -> List[dict]:
        """Per image: dict(per_class={class: the dict of `crack_from_stats`}, cldice=, cl_precision=, ... the nan-aware means
        over the classes).  classes=None: range(num_classes); for cracks pass the crack classes alone -- the skeleton of a
        background that fills the image says little and takes as many passes as half its width."""
        classes = list(range(self.num_classes)) if classes is None else [int(c) for c in classes]
        si, sf = self.skeleton_stats(pred, gt, classes)
        rows = crack_from_stats(si.cpu().numpy(), sf.cpu().numpy())
        out = []
        for row in rows:
            d = dict(per_class=dict(zip(classes, row)))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)   # all-nan -> nan, as the overlap means
                for key in CRACK_KEYS:
                    d[key] = float(np.nanmean([float(r[key]) for r in row]))
            out.append(d)
        return out

    def evaluate(self, pred: torch.Tensor, gt: torch.Tensor) -> List[dict]:
        c = self.counts(pred, gt).cpu().numpy()
        px = int(pred.shape[1] * pred.shape[2])
        return [metrics_from_counts(c[i], self.num_classes, px) for i in range(c.shape[0])]


def csv_row(model_info: Sequence, batch_num: int, image_idx: int, m: dict, inference_time: float) -> list:
    """One row in the reference's schema; `model_info` = (Model_ID, Model_Name, Patch_Size, Hidden_Size, Layers, Heads)."""
    j = lambda v: "|".join(map(str, v))
    return list(model_info) + [batch_num, image_idx, m["Accuracy"], m["Mean_IoU"], m["Mean_Dice"], inference_time,
                               j(m["GT_Classes"]), j(m["Pred_Classes"]), j(m["Missing_Classes"]),
                               j(m["False_Positive_Classes"])]


def write_metrics_csv(path: str, rows: Sequence[Sequence]) -> None:
    with open(path, mode="w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CSV_COLUMNS)
        w.writerows(rows)


def distance_csv_row(model_info: Sequence, batch_num: int, image_idx: int, mode: str, percentile, m: dict) -> list:
    """One row of <model>_distance_metrics.csv from one image's dict of `Evaluator.distance_metrics`; Per_Class holds
    class:paed:hausdorff:hd_percentile:assd for every class present in either map, joined by "|"."""
    per = "|".join(f"{c}:{r['paed']:.6g}:{r['hausdorff']:.6g}:{r['hd_percentile']:.6g}:{r['assd']:.6g}"
                   for c, r in m["per_class"].items() if r["n"] or r["m"])
    return [model_info[0], model_info[1], batch_num, image_idx, mode, percentile, m["paed"], m["hausdorff"],
            m["hd_percentile"], m["assd"], per]


def write_distance_csv(path: str, rows: Sequence[Sequence]) -> None:
    with open(path, mode="w", newline="") as f:
        w = csv.writer(f)
        w.writerow(DISTANCE_CSV_COLUMNS)
        w.writerows(rows)


def crack_csv_row(model_info: Sequence, batch_num: int, image_idx: int, m: dict) -> list:
    """One row of <model>_crack_metrics.csv from one image's dict of `Evaluator.crack_metrics`; Per_Class holds
    class:cldice:length_gt:length_pred:mean_width_gt:mean_width_pred for every class present in either map, joined by "|"."""
    per = "|".join(f"{c}:{r['cldice']:.6g}:{r['length_gt']}:{r['length_pred']}:{r['mean_width_gt']:.6g}:{r['mean_width_pred']:.6g}"
                   for c, r in m["per_class"].items() if r["n"] or r["m"])
    return [model_info[0], model_info[1], batch_num, image_idx, m["cldice"], m["cl_precision"], m["cl_sensitivity"],
            m["length_gt"], m["length_pred"], m["mean_width_gt"], m["mean_width_pred"], per]


def write_crack_csv(path: str, rows: Sequence[Sequence]) -> None:
    with open(path, mode="w", newline="") as f:
        w = csv.writer(f)
        w.writerow(CRACK_CSV_COLUMNS)
        w.writerows(rows)
