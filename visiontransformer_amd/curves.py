"""Crack-benchmark curves on the device: the precision-recall counts of one class' probability map over all thresholds, with a
pixel tolerance, and from them ODS, OIS and AP.

The crack benchmarks (CrackTree, CrackForest, DeepCrack) lead with the curve of the probability map, scored with a tolerance: a
predicted crack pixel within a few pixels of a true one is not an error.  The reference logs precision and recall at the fixed
0.5 cut (model/PAED/classes.py:308-330, 587-606).  One launch of `vitseg_pr_counts` (csrc/curves.hip, include/vitseg_curves.h)
re-generates every pixel's 16-bit score q of class `cls` from the low-res head output [n, C, g, g] -- `confidence.confidence_map`
under a mask that states `cls` everywhere, bit for bit --, dilates it by the Euclidean disc of the tolerance inside LDS and
returns per image and bin (q * bins) >> 16 the int64 row
  (pred: valid pixels, hit: those within the tolerance of a true pixel, found: true pixels by the best score within the tolerance).
Threshold k means "positive iff bin >= k", i.e. confidence_map(..., quantised=True) >= ceil(k 65536 / bins).  The ratios are
host arithmetic on the integers, pooled by addition first: `curve_from_counts`, `ods`, `ois`, `ap`, `summary`.  The usual host
answer is a scipy.ndimage grey dilation and a distance transform per image and three bincounts.
"""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from . import _common, _ext, _lib
from . import confidence as _conf
from . import simplify as _simplify

COUNT_FIELDS = ("pred", "hit", "found")
MAX_BINS = 1024          # include/vitseg_curves.h VITSEG_CURVES_MAX_BINS
MAX_TOLERANCE = 16.0     # pixels: tol2 at most VITSEG_CURVES_MAX_TOL2 = 256
Q_ONE = _conf.Q_ONE
CSV_COLUMNS = ["Model_ID", "Model_Name", "Class", "Bins", "Tolerance", "Row", "Threshold", "Predicted", "Hit", "Found", "N_GT",
               "Precision", "Recall", "F"]


def _symbol(name: str):
    return _ext.ext_symbol("curves", name)


def tolerance_to_tol2(tolerance) -> int:
    """floor(tolerance^2) for a tolerance of 0..16 pixels, the square formed as `simplify.tol2_q8` forms it (in 1/256 px^2,
    rounded: sqrt(5) gives 5, not 4).  ValueError for anything but a finite real number in range."""
    q8 = _simplify.tol2_q8(tolerance)   # refuses what is no finite number of pixels
    if float(tolerance) > MAX_TOLERANCE:
        raise ValueError(f"the curve tolerance must be in 0..{MAX_TOLERANCE:g} pixels, got {tolerance!r}")
    return q8 >> 8


def threshold_q(k: int, bins: int) -> int:
    """The smallest q whose bin (q * bins) >> 16 is at least k: ceil(k 65536 / bins)."""
    return -((-int(k) << 16) // int(bins))


def check_options(cls, bins, tolerance, ignore_label=None) -> int:
    """The argument checks of `pr_counts` that need no tensor; returns tol2."""
    _common.integer("cls", cls, 0, 254)
    _common.integer("bins", bins, 1, MAX_BINS)
    if ignore_label is not None and not _common.is_integer(ignore_label, 0, 255):
        raise ValueError(f"ignore_label must be None or an integer in 0..255, got {ignore_label!r}")
    return tolerance_to_tol2(tolerance)


def _checked(lowres, gt, kind, cls):
    """confidence._checked with the ground truth in the mask's place and the class among lowres' planes; returns (lowres [n, C,
    g, g], gt [n, S, S], single)."""
    if kind not in _conf.KINDS:
        raise ValueError(f"kind must be one of {sorted(_conf.KINDS)}, got {kind!r}")
    if isinstance(gt, np.ndarray):
        gt = torch.from_numpy(gt)
    if not isinstance(gt, torch.Tensor) or gt.dtype != torch.uint8 or gt.dim() not in (2, 3):
        raise ValueError("gt must be a uint8 tensor [n, S, S] or [S, S]")
    if isinstance(lowres, torch.Tensor) and lowres.dim() in (3, 4) and int(cls) >= int(lowres.shape[-3]):
        raise ValueError(f"cls must be one of the {int(lowres.shape[-3])} classes of lowres, got {cls!r}")
    return _conf._checked(lowres, gt, kind)   # (the shapes it names as the mask's are gt's)


@torch.no_grad()
def pr_counts(lowres, gt, cls: int = 1, bins: int = 256, tolerance=0, ignore_label: Optional[int] = None, kind: str = "prob"):
    """The counts of class `cls` under the low-res head output `lowres` (fp32 device tensor [n, C, g, g] or [C, g, g]; g == S:
    full-size logits as they stand) against the ground truth `gt` (uint8 [n, S, S] or [S, S]): int64 numpy [n, bins, 3] ([bins,
    3] for a single image), per image and bin (q * bins) >> 16 the (pred, hit, found) of the module's head.  `tolerance` is in
    pixels, 0..16: a pixel pair counts as near when dy^2 + dx^2 <= floor(tolerance^2); 0 is the plain pixel curve.  Pixels with
    gt == ignore_label are void: they are neither predicted nor true and lend no score to a true pixel nearby.  Pool images by
    adding the arrays.  One launch; there is no CPU fallback."""
    tol2 = check_options(cls, bins, tolerance, ignore_label)
    lowres, gt, single = _checked(lowres, gt, kind, cls)
    n, C, g, _ = (int(d) for d in lowres.shape)
    S = int(gt.shape[-1])
    counts = torch.empty((n, int(bins), 3), dtype=torch.int64, device=lowres.device)
    with torch.cuda.device(lowres.device):
        nbytes = _symbol("vitseg_pr_counts_scratch_bytes")(n, S, tol2)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=lowres.device) if nbytes else None
        _lib.check(_symbol("vitseg_pr_counts")(
            lowres.data_ptr(), gt.data_ptr(), n, C, g, S, int(cls), _conf.KINDS[kind], int(bins), tol2,
            -1 if ignore_label is None else int(ignore_label), counts.data_ptr(), None if scratch is None else scratch.data_ptr(),
            nbytes, torch.cuda.current_stream().cuda_stream))
    out = counts.cpu().numpy()
    return out[0] if single else out


# ---- host arithmetic on the integers ----

def _images(counts) -> np.ndarray:
    """counts as int64 [images, bins, 3]"""
    c = np.asarray(counts)
    if c.ndim < 2 or c.shape[-1] != len(COUNT_FIELDS) or c.shape[-2] < 1 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"counts must be an integer array [..., bins, {len(COUNT_FIELDS)}], got {c.dtype} {c.shape}")
    c = c.reshape(-1, c.shape[-2], 3).astype(np.int64)
    if (c < 0).any():
        raise ValueError("counts must not be negative")
    return c


def _curve(c: np.ndarray) -> dict:
    """The curve of one [bins, 3] table; every ratio from Python integers."""
    T = c.shape[0]
    cum = np.cumsum(c[::-1], axis=0)[::-1]   # threshold k: the bins k ..
    n_gt = int(c[:, 2].sum())
    nan = float("nan")
    out = {"threshold": [], "predicted": [], "hit": [], "found": [], "n_gt": n_gt, "precision": [], "recall": [], "f": []}
    for k in range(T):
        pred, hit, found = (int(v) for v in cum[k])
        p = hit / pred if pred else nan
        r = found / n_gt if n_gt else nan
        f = 2.0 * p * r / (p + r) if pred and n_gt and hit + found else 0.0
        out["threshold"].append(threshold_q(k, T) / Q_ONE)
        for name, v in (("predicted", pred), ("hit", hit), ("found", found), ("precision", p), ("recall", r), ("f", f)):
            out[name].append(v)
    return out


def curve_from_counts(counts) -> dict:
    """The curve of a table int64 [bins, 3], or of several [..., bins, 3] pooled by integer addition BEFORE the ratios are taken:
    per threshold k (positive iff bin >= k) the lists "threshold" (= ceil(k 65536 / bins) / 65535), "predicted", "hit", "found",
    "precision" = hit / predicted (nan where nothing is predicted), "recall" = found / n_gt (nan when n_gt = 0) and
    "f" = 2 P R / (P + R), 0 where nothing is predicted or P + R = 0; "n_gt": the true pixels."""
    return _curve(_images(counts).sum(axis=0))


def _best(curve: dict):
    f = curve["f"]
    k = max(range(len(f)), key=lambda i: (f[i], -i))   # the smallest k among equals
    return f[k], k


def ods(counts) -> dict:
    """Optimal data-set scale: the best F of the pooled counts at ONE threshold for all images, the smallest k among equals:
    {"f", "k", "threshold", "precision", "recall"}."""
    cur = curve_from_counts(counts)
    f, k = _best(cur)
    return {"f": f, "k": k, "threshold": cur["threshold"][k], "precision": cur["precision"][k], "recall": cur["recall"][k]}


def ois(counts) -> float:
    """Optimal image scale: the mean over the images with true pixels of each image's own best F; nan if there are none."""
    best = [_best(cur)[0] for cur in (_curve(c) for c in _images(counts)) if cur["n_gt"] > 0]
    return sum(best) / len(best) if best else float("nan")


def ap(counts) -> float:
    """Average precision of the pooled counts: sum_k (R_k - R_(k+1)) P_k with R_bins = 0, over the k with predictions; nan when
    there is no true pixel."""
    cur = curve_from_counts(counts)
    if cur["n_gt"] == 0:
        return float("nan")
    rec = cur["recall"] + [0.0]
    return sum((rec[k] - rec[k + 1]) * cur["precision"][k] for k in range(len(cur["f"])) if cur["predicted"][k])


def summary(counts) -> dict:
    """{"ods": ods(counts), "ois": ois(counts), "ap": ap(counts)}"""
    return {"ods": ods(counts), "ois": ois(counts), "ap": ap(counts)}


# ---- the evaluation scripts' file ----

def csv_rows(model_info, counts, cls: int, tolerance) -> List[list]:
    """The rows of <model>_pr_curve.csv from the per-image counts int64 [images, bins, 3]: one per threshold of the pooled
    counts, then the rows ODS (its threshold, precision, recall and F), OIS and AP (the value under F)."""
    c = _images(counts)
    bins = c.shape[1]
    cur = curve_from_counts(c)
    head = [model_info[0], model_info[1], cls, bins, tolerance]
    rows = [head + [k, cur["threshold"][k], cur["predicted"][k], cur["hit"][k], cur["found"][k], cur["n_gt"], cur["precision"][k],
                    cur["recall"][k], cur["f"][k]] for k in range(bins)]
    s = summary(c)
    o = s["ods"]
    rows.append(head + ["ODS", o["threshold"], cur["predicted"][o["k"]], cur["hit"][o["k"]], cur["found"][o["k"]], cur["n_gt"],
                        o["precision"], o["recall"], o["f"]])
    rows.append(head + ["OIS", "", "", "", "", cur["n_gt"], "", "", s["ois"]])
    rows.append(head + ["AP", "", "", "", "", cur["n_gt"], "", "", s["ap"]])
    return rows


__all__ = ["pr_counts", "curve_from_counts", "ods", "ois", "ap", "summary", "tolerance_to_tol2", "threshold_q", "check_options",
           "csv_rows", "COUNT_FIELDS", "CSV_COLUMNS", "MAX_BINS", "MAX_TOLERANCE"]
