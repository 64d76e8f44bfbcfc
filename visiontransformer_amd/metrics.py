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

Regions (`Evaluator.region_metrics`): how many defects were found, missed and raised falsely.  `vitseg_region_match`
(csrc/match.hip) labels the regions of both maps, counts the intersection of every (predicted, true) pair and matches the pairs
above an IoU threshold of one half or more, where no region has two partners (the panoptic quality of Kirillov et al. 2019,
PQ = SQ * RQ per class), beside coverage hit rates for thin structures; `matches_from_stats` is the host arithmetic on its
integers, and `pool_region_stats` sums them over a data set first, which is the form to report.
"""
from __future__ import annotations

import ctypes
import math
import warnings
from fractions import Fraction
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _common, _lib
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


REGION_KEYS = ("pq", "sq", "rq", "precision", "recall", "f1", "found_rate", "confirmed_rate", "mean_matched_iou")
# header of <model>_region_metrics.csv (--region-metrics of the evaluation scripts): one row per image and class, then one
# pooled row per class (Batch_Num "pooled") from the integers summed over all images
REGION_CSV_COLUMNS = ["Model_ID", "Model_Name", "Batch_Num", "Image_Idx", "Class", "IoU_Threshold", "Coverage", "N_GT", "N_Pred",
                      "TP", "FP", "FN", "GT_Found", "Pred_Confirmed", "Sum_Q", "Sum_I", "Sum_U", "PQ", "SQ", "RQ", "Precision",
                      "Recall", "F1", "Found_Rate", "Confirmed_Rate", "Mean_Matched_IoU"]


def _unit_fraction(value, what: str):
    f = Fraction(str(value))
    if f.denominator > 1000:
        raise ValueError(f"{what} must be a fraction with a denominator of at most 1000 (three decimals), got {value!r}")
    return f


def iou_threshold_fraction(threshold):
    """An IoU threshold as the rational (thr_num, thr_den) of vitseg_region_match: 0.5 -> (1, 2), 0.75 -> (3, 4).  ValueError
    below 0.5 (a region could have two partners), at 1 or above, or when the denominator would pass 1000."""
    f = _unit_fraction(threshold, "iou_threshold")
    if not Fraction(1, 2) <= f < 1:
        raise ValueError(f"iou_threshold must lie in 0.5 <= t < 1, got {threshold!r}")
    return f.numerator, f.denominator


def coverage_fraction(coverage):
    """A coverage 0 < c <= 1 as the rational (cov_num, cov_den) of vitseg_region_match; ValueError as above."""
    f = _unit_fraction(coverage, "coverage")
    if not 0 < f <= 1:
        raise ValueError(f"coverage must lie in 0 < c <= 1, got {coverage!r}")
    return f.numerator, f.denominator


def matches_from_stats(stats):
    """stats int64 [n, K, 8] of vitseg_region_match (include/vitseg.h) -> per image a list of K dicts (one list for a pooled
    [K, 8]).  With fp = n_pred - tp, fn = n_gt - tp and IoU sum = sum_q / 2^32:
      rq  tp / (tp + fp / 2 + fn / 2)     sq  IoU sum / tp     pq  IoU sum / (tp + fp / 2 + fn / 2) = sq * rq
      precision tp / n_pred, recall tp / n_gt, f1 2 tp / (n_pred + n_gt)
      found_rate gt_found / n_gt, confirmed_rate pred_confirmed / n_pred: the coverage hit rates
      mean_matched_iou  sum_i / sum_u: the IoU of all matched pixels pooled (sq weighs every pair alike)
    and the eight integers.  An entry whose denominator is 0 is nan."""
    st = np.asarray(stats, dtype=np.int64)
    if st.ndim not in (2, 3) or st.shape[-1] != 8:
        raise ValueError(f"stats must be [n, K, 8] or [K, 8], got {st.shape}")
    nan = float("nan")
    ratio = lambda a, b: a / b if b else nan
    out = []
    for img in (st[None] if st.ndim == 2 else st):
        row = []
        for rec in img:
            n_gt, n_pred, tp, found, confirmed, sq, si, su = (int(v) for v in rec)
            fp, fn = n_pred - tp, n_gt - tp
            iou_sum = sq / float(1 << 32)
            row.append(dict(n_gt=n_gt, n_pred=n_pred, tp=tp, fp=fp, fn=fn, gt_found=found, pred_confirmed=confirmed, sum_q=sq,
                            sum_i=si, sum_u=su, pq=ratio(iou_sum, tp + fp / 2 + fn / 2), sq=ratio(iou_sum, tp),
                            rq=ratio(tp, tp + fp / 2 + fn / 2), precision=ratio(tp, n_pred), recall=ratio(tp, n_gt),
                            f1=ratio(2 * tp, n_pred + n_gt), found_rate=ratio(found, n_gt),
                            confirmed_rate=ratio(confirmed, n_pred), mean_matched_iou=ratio(si, su)))
        out.append(row)
    return out[0] if st.ndim == 2 else out


def pool_region_stats(list_of_stats) -> np.ndarray:
    """int64 [K, 8]: the integers of vitseg_region_match summed over the images of every [n, K, 8] (or [K, 8]) in the list.  PQ
    is a data-set quantity: `matches_from_stats` of this sum is the figure to report, not a mean of per-image ratios."""
    parts = [np.asarray(s.cpu() if torch.is_tensor(s) else s, dtype=np.int64) for s in list_of_stats]
    if not parts or any(p.ndim not in (2, 3) or p.shape[-2:] != parts[0].shape[-2:] or p.shape[-1] != 8 for p in parts):
        raise ValueError("pool_region_stats needs a non-empty list of [n, K, 8] arrays with one K")
    return sum(p.reshape(-1, *p.shape[-2:]).sum(axis=0) for p in parts)


def _class_means(row: Sequence[dict], keys: Sequence[str]) -> Dict[str, float]:
    """The nan-aware mean over one image's per-class dicts, for every key."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # all-nan -> nan, as the overlap means
        return {key: float(np.nanmean([float(r[key]) for r in row])) for key in keys}


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

    @staticmethod
    def _label_values(classes) -> List[int]:
        classes = [int(c) for c in classes]
        if not classes or len(classes) > 256 or any(not 0 <= c <= 255 for c in classes):
            raise ValueError(f"classes must be 1..256 label values in 0..255, got {classes}")
        return classes

    def _device_pair(self, pred: torch.Tensor, gt: torch.Tensor, classes=None, size_only: bool = False):
        """(pred, gt, classes): the uint8 prediction [n, H, W] and the ground truth validated (then `classes`, when given) and
        contiguous on the device, the ground truth as uint8 and nearest-resized to the prediction's size when the sizes
        differ -- one enqueue on the current stream of the device.  size_only: `pred` only states the size and is passed
        through as it is."""
        if not size_only and (pred.dtype != torch.uint8 or pred.dim() != 3):
            raise ValueError(f"pred must be uint8 [n, H, W], got {pred.dtype} {tuple(pred.shape)}")
        if gt.dim() != 3 or gt.shape[0] != pred.shape[0]:
            raise ValueError("Number of images and masks must be equal!")   # the reference's dataset check, classes.py:34-35
        if classes is not None:
            classes = self._label_values(classes)
        if not size_only:
            pred = pred.to(self.device).contiguous()
        gt = gt.to(self.device).to(torch.uint8).contiguous()
        n, H, W = (int(d) for d in pred.shape)
        if tuple(gt.shape[1:]) != (H, W):
            Hg, Wg = (int(d) for d in gt.shape[1:])
            g2 = torch.empty((n, H, W), dtype=torch.uint8, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().vitseg_resize_nearest_u8(gt.data_ptr(), n, Hg, Wg, self._nearest(Hg, H).data_ptr(),
                                                               self._nearest(Wg, W).data_ptr(), H, W, None, 0, g2.data_ptr(),
                                                               torch.cuda.current_stream().cuda_stream))
            gt = g2
        return pred, gt, classes

    def resized_gt(self, gt: torch.Tensor, pred: torch.Tensor) -> torch.Tensor:
        """The ground truth as uint8 [n, H, W] on the device, nearest-resized to the prediction's size as `distance_stats`
        does (the tensor itself, cast, when the sizes agree)."""
        return self._device_pair(pred, gt, size_only=True)[1]

    def distance_stats(self, pred: torch.Tensor, gt: torch.Tensor, classes: Sequence[int], mode: int, pct_num: int,
                       pct_den: int):
        """(stats_i int64 [n, K, 6], stats_f float64 [n, K, 2]) device tensors of vitseg_distance_stats for uint8 predictions
        [n, H, W]; a ground truth of another size is nearest-resized first, as `counts` does on the fly."""
        pred, gt, classes = self._device_pair(pred, gt, classes)
        n, H, W = (int(d) for d in pred.shape)
        K = len(classes)
        cls = (ctypes.c_int32 * K)(*classes)
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream().cuda_stream
            nbytes = _lib.symbol("vitseg_distance_scratch_bytes")(n, H, W)
            if nbytes == 0:
                raise ValueError(f"distance metrics: H and W must lie in 1..16384 and n in 1..32767, got {n} x {H} x {W}")
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            si = torch.empty((n, K, 6), dtype=torch.int64, device=self.device)
            sf = torch.empty((n, K, 2), dtype=torch.float64, device=self.device)
            _lib.check(_lib.symbol("vitseg_distance_stats")(pred.data_ptr(), gt.data_ptr(), n, H, W, cls, K, int(mode),
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
        return [dict(per_class=dict(zip(classes, row)), **_class_means(row, DISTANCE_KEYS)) for row in rows]

    def skeleton_stats(self, pred: torch.Tensor, gt: torch.Tensor, classes: Sequence[int], route: int = 0):
        """(stats_i int64 [n, K, 10], stats_f float64 [n, K, 2]) device tensors of vitseg_skeleton_stats for uint8 predictions
        [n, H, W]; a ground truth of another size is nearest-resized first, as `distance_stats` does.  One enqueue on the
        current stream; planes too large for the resident route (see skeleton.py) synchronise it."""
        pred, gt, classes = self._device_pair(pred, gt, classes)
        n, H, W = (int(d) for d in pred.shape)
        K = len(classes)
        cls = (ctypes.c_int32 * K)(*classes)
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream().cuda_stream
            nbytes = _lib.symbol("vitseg_skeleton_stats_scratch_bytes")(n, H, W, int(route))
            if nbytes == 0:
                raise ValueError(f"crack metrics: H and W must lie in 1..16384 and n in 1..32767 (and the plane must fit the "
                                 f"route asked for), got {n} x {H} x {W}, route {route}")
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            si = torch.empty((n, K, 10), dtype=torch.int64, device=self.device)
            sf = torch.empty((n, K, 2), dtype=torch.float64, device=self.device)
            _lib.check(_lib.symbol("vitseg_skeleton_stats")(pred.data_ptr(), gt.data_ptr(), n, H, W, cls, K,
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
        return [dict(per_class=dict(zip(classes, row)), **_class_means(row, CRACK_KEYS)) for row in rows]

    def region_match_stats(self, pred: torch.Tensor, gt: torch.Tensor, classes: Sequence[int], iou=(1, 2), coverage=(1, 2),
                           connectivity: int = 4, background: int = 0, ignore_label: int = -1, return_info: bool = False):
        """stats int64 [n, K, 8] device tensor of vitseg_region_match for uint8 predictions [n, H, W]; a ground truth of
        another size is nearest-resized first, exactly as `distance_stats` does.  iou and coverage are (num, den) pairs.
        return_info: (stats, pred_info, gt_info, gt as compared), the int32 [n, H, W, 2] planes of include/vitseg.h.  One
        enqueue on the current stream."""
        pred, gt, classes = self._device_pair(pred, gt, classes)
        n, H, W = (int(d) for d in pred.shape)
        K = len(classes)
        cls = (ctypes.c_int32 * K)(*classes)
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream().cuda_stream
            nbytes = _lib.symbol("vitseg_region_match_scratch_bytes")(n, H, W)
            if nbytes == 0:
                raise ValueError(f"region metrics: H * W must stay below 2^31 and n in 1..32767, got {n} x {H} x {W}")
            scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            stats = torch.empty((n, K, 8), dtype=torch.int64, device=self.device)
            pinfo = torch.empty((n, H, W, 2), dtype=torch.int32, device=self.device) if return_info else None
            ginfo = torch.empty((n, H, W, 2), dtype=torch.int32, device=self.device) if return_info else None
            _lib.check(_lib.symbol("vitseg_region_match")(
                pred.data_ptr(), gt.data_ptr(), n, H, W, cls, K, int(connectivity), int(background), int(ignore_label),
                int(iou[0]), int(iou[1]), int(coverage[0]), int(coverage[1]), stats.data_ptr(),
                None if pinfo is None else pinfo.data_ptr(), None if ginfo is None else ginfo.data_ptr(), scratch.data_ptr(),
                nbytes, st))
        return (stats, pinfo, ginfo, gt) if return_info else stats

    def _region_arguments(self, classes, iou_threshold, coverage, connectivity, background, ignore_label):
        """The arguments of `region_metrics`, checked before anything reaches the library."""
        thr, cov = iou_threshold_fraction(iou_threshold), coverage_fraction(coverage)
        _common.connectivity(connectivity)
        background = _common.integer("background", background, 0, 255)
        if ignore_label is None:
            ignore_label = -1
        elif not _common.is_integer(ignore_label, 0, 255) or int(ignore_label) == background:
            raise ValueError(f"ignore_label must be None or an integer in 0..255 other than the background, got {ignore_label!r}")
        ignore_label = int(ignore_label)
        if classes is None:
            classes = [c for c in range(self.num_classes) if c not in (background, ignore_label)]
        classes = self._label_values(classes)
        if len(set(classes)) != len(classes) or background in classes or ignore_label in classes:
            raise ValueError(f"classes must be distinct and hold neither the background {background} nor the ignore label, "
                             f"got {classes}")
        return classes, thr, cov, background, ignore_label

    def region_metrics(self, pred: torch.Tensor, gt: torch.Tensor, classes: Optional[Sequence[int]] = None,
                       iou_threshold=0.5, coverage=0.5, connectivity: int = 4, background: int = 0, ignore_label=None,
                       return_matches: bool = False) -> List[dict]:
        """Per image: dict(per_class={class: the dict of `matches_from_stats`}, pq=, sq=, rq=, precision=, recall=, f1=,
        found_rate=, confirmed_rate=, mean_matched_iou= the nan-aware means over the classes, stats= the int64 [K, 8] behind
        them for `pool_region_stats`).  A predicted region and a true one of a class are matched when their IoU exceeds
        iou_threshold (0.5 <= t < 1, at most three decimals); a true region is found, a predicted one confirmed, when
        `coverage` of it or more lies on the other map's pixels of its class.  classes=None: range(num_classes) without the
        background.  ignore_label: ground-truth pixels of this value are void (see include/vitseg.h).
        return_matches: every dict also holds matches={"gt": int32 [kg, 9], "pred": int32 [kp, 9]}: `region_boxes`' seven
        fields in its (class, first) order for the regions of `classes` (of pred: those with a counted pixel), then `match`
        (the partner's row in the other list, -1 if none) and `covered` (its pixels on the other map's class)."""
        if not isinstance(pred, torch.Tensor) or pred.dtype != torch.uint8 or pred.dim() != 3:
            raise ValueError(f"pred must be a uint8 tensor [n, H, W], got {getattr(pred, 'dtype', type(pred).__name__)}")
        classes, thr, cov, background, ignore_label = self._region_arguments(classes, iou_threshold, coverage, connectivity,
                                                                            background, ignore_label)
        res = self.region_match_stats(pred, gt, classes, thr, cov, connectivity, background, ignore_label,
                                      return_info=return_matches)
        stats = (res[0] if return_matches else res).cpu().numpy()
        out = [dict(per_class=dict(zip(classes, row)), stats=stats[i], **_class_means(row, REGION_KEYS))
               for i, row in enumerate(matches_from_stats(stats))]
        if return_matches:
            from .regions import region_boxes
            _, pinfo, ginfo, g = res
            if ignore_label >= 0:
                g = torch.where(g == ignore_label, torch.full_like(g, background), g)
            sides = {"pred": (region_boxes(pred.to(self.device), background=background, connectivity=connectivity),
                              pinfo.cpu().numpy()),
                     "gt": (region_boxes(g, background=background, connectivity=connectivity), ginfo.cpu().numpy())}
            for i, d in enumerate(out):
                tabs, rows = {}, {}
                for name, (recs, info) in sides.items():
                    flat = info[i].reshape(-1, 2)
                    rec = recs[i][np.isin(recs[i][:, 0], classes)]
                    rec = rec[flat[rec[:, 6], 0] != -2]          # predicted regions without a counted pixel
                    rows[name] = {int(f): r for r, f in enumerate(rec[:, 6])}
                    tabs[name] = np.concatenate([rec, flat[rec[:, 6]]], axis=1).astype(np.int32).reshape(-1, 9)
                for name, other in (("pred", "gt"), ("gt", "pred")):
                    for r in tabs[name]:
                        r[7] = rows[other][int(r[7])] if r[7] >= 0 else -1
                d["matches"] = tabs
        return out

    def region_props(self, pred: torch.Tensor, gt: Optional[torch.Tensor] = None, skeleton_classes=None,
                     connectivity: int = 4, background: int = 0, pixel_size: float = 1.0, route: str = "auto") -> List[dict]:
        """Per image: dict(pred=[one dict per region of the prediction], gt=[the same for the ground truth, when given]) --
        the dicts of regions.props_from_records (position, size, axes, orientation, perimeter, frame contact and, for
        `skeleton_classes` (None: none; "all"; or label values), the region's own skeleton length and widths), in
        `region_boxes`' (class, first) order, lengths in units of `pixel_size`.  A ground truth of another size is
        nearest-resized to the prediction first, as `distance_stats` does.  One regions.region_props call per map."""
        from . import regions as _regions
        if not isinstance(pred, torch.Tensor) or pred.dtype != torch.uint8 or pred.dim() != 3:
            raise ValueError(f"pred must be a uint8 tensor [n, H, W], got {getattr(pred, 'dtype', type(pred).__name__)}")
        maps = {"pred": pred.to(self.device).contiguous()} if gt is None else \
            dict(zip(("pred", "gt"), self._device_pair(pred, gt)))
        out = [dict() for _ in range(pred.shape[0])]
        for name, m in maps.items():
            recs = _regions.region_props(m, skeleton_classes=skeleton_classes, background=background,
                                         connectivity=connectivity, route=route)
            for d, r in zip(out, recs):
                d[name] = _regions.props_from_records(r, pixel_size)
        return out

    def crack_graph(self, pred: torch.Tensor, classes: Sequence[int], pixel_size: float = 1.0, route: str = "auto",
                    simplify=None) -> List[dict]:
        """Per image: {class: dict(nodes=, branches=, points=, table=, summary=)} for the label values in `classes` -- the
        centre-line graph of the skeleton of {pred == class} (centerlines.trace: the int32 / int64 rows and the point lists),
        `centerlines.branch_table`'s dict per branch and `centerlines.summary`, lengths in units of `pixel_size`.  The
        prediction alone is read: uint8 [n, H, W].  `simplify`: a tolerance in pixels, the polylines thinned on the device
        (centerlines.trace); lengths and widths stay those of the full branches."""
        from . import centerlines as _cl
        if not isinstance(pred, torch.Tensor) or pred.dtype != torch.uint8 or pred.dim() != 3:
            raise ValueError(f"pred must be a uint8 tensor [n, H, W], got {getattr(pred, 'dtype', type(pred).__name__)}")
        if classes is None:
            raise ValueError("classes must be a sequence of label values")
        _common.pixel_size(pixel_size)
        if simplify is not None:
            from .simplify import tol2_q8
            tol2_q8(simplify)
        out = []
        for per_class in _cl.trace(pred.to(self.device), classes=classes, route=route, simplify=simplify):
            out.append({c: dict(nodes=nd, branches=br, points=pts, table=_cl.branch_table(br, pixel_size, pts),
                                summary=_cl.summary(nd, br, pixel_size)) for c, (nd, br, pts) in per_class.items()})
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
    _common.write_csv(path, CSV_COLUMNS, rows)


def distance_csv_row(model_info: Sequence, batch_num: int, image_idx: int, mode: str, percentile, m: dict) -> list:
    """One row of <model>_distance_metrics.csv from one image's dict of `Evaluator.distance_metrics`; Per_Class holds
    class:paed:hausdorff:hd_percentile:assd for every class present in either map, joined by "|"."""
    per = "|".join(f"{c}:{r['paed']:.6g}:{r['hausdorff']:.6g}:{r['hd_percentile']:.6g}:{r['assd']:.6g}"
                   for c, r in m["per_class"].items() if r["n"] or r["m"])
    return [model_info[0], model_info[1], batch_num, image_idx, mode, percentile, m["paed"], m["hausdorff"],
            m["hd_percentile"], m["assd"], per]


def crack_csv_row(model_info: Sequence, batch_num: int, image_idx: int, m: dict) -> list:
    """One row of <model>_crack_metrics.csv from one image's dict of `Evaluator.crack_metrics`; Per_Class holds
    class:cldice:length_gt:length_pred:mean_width_gt:mean_width_pred for every class present in either map, joined by "|"."""
    per = "|".join(f"{c}:{r['cldice']:.6g}:{r['length_gt']}:{r['length_pred']}:{r['mean_width_gt']:.6g}:{r['mean_width_pred']:.6g}"
                   for c, r in m["per_class"].items() if r["n"] or r["m"])
    return [model_info[0], model_info[1], batch_num, image_idx, m["cldice"], m["cl_precision"], m["cl_sensitivity"],
            m["length_gt"], m["length_pred"], m["mean_width_gt"], m["mean_width_pred"], per]


def region_csv_row(model_info: Sequence, batch_num, image_idx, cls: int, iou_threshold, coverage, m: dict) -> list:
    """One row of <model>_region_metrics.csv from one class's dict of `matches_from_stats`; batch_num "pooled" and an empty
    image_idx mark a row of the integers summed over all images."""
    return [model_info[0], model_info[1], batch_num, image_idx, cls, iou_threshold, coverage, m["n_gt"], m["n_pred"], m["tp"],
            m["fp"], m["fn"], m["gt_found"], m["pred_confirmed"], m["sum_q"], m["sum_i"], m["sum_u"], m["pq"], m["sq"], m["rq"],
            m["precision"], m["recall"], m["f1"], m["found_rate"], m["confirmed_rate"], m["mean_matched_iou"]]
