"""What the reference's train / evaluation scripts share (model/CE/*.py, model/PAED/*.py), for the thin drivers under
model/: batches (the reference's dataset VisionChallenge/ is private, so synthetic tensors unless --data points at a
torch.save'd dict), checkpoint discovery with the reference's rule, and the per-image evaluation loop + CSV.
"""
from __future__ import annotations

import os
import re
import time
from typing import List, Optional

import torch

from . import clean, curves, reports, synth
from . import decide as _decide
from . import simplify as _simplify
from .metrics import Evaluator, csv_row, write_metrics_csv
from .tta import parse_sizes


def checkpoint_epoch(path: str) -> Optional[int]:
    m = re.search(r"epoch=(\d+)", path)
    return int(m.group(1)) if m else None


def get_latest_checkpoint(version_n: int, base_path: str) -> Optional[str]:
    """The checkpoint with the largest epoch number among logs/vit-model/version_<n>/checkpoints/epoch=E-step=S.ckpt,
    None (with a message) when the directory or any checkpoint is missing -- the rule of the reference's helper
    (model/CE/datasetTestViTmodel.py:38-54, also used by model/PAED/ViTscriptTest.py)."""
    ckpt_dir = os.path.join(base_path, "logs", "vit-model", f"version_{version_n}", "checkpoints")
    if not os.path.isdir(ckpt_dir):
        print(f"no checkpoint directory: {ckpt_dir}")
        return None
    by_epoch = {}
    for name in sorted(os.listdir(ckpt_dir)):
        epoch = checkpoint_epoch(name) if name.endswith(".ckpt") else None
        if epoch is not None:
            by_epoch[epoch] = name
    if not by_epoch:
        print(f"no epoch=<E>-step=<S>.ckpt file in {ckpt_dir}")
        return None
    path = os.path.join(ckpt_dir, by_epoch[max(by_epoch)])
    print(f"latest checkpoint: {path}")
    return path


def add_ce_loss_arguments(ap) -> None:
    """The loss options of the CE training scripts: the arguments of nn.CrossEntropyLoss the reference leaves at their
    defaults (model/CE/classes.py:268)."""
    ap.add_argument("--ignore-index", type=int, default=None,
                    help="label whose pixels do not count in the loss (255 for void / border pixels, -100 for torch's default)")
    ap.add_argument("--class-weights", default=None, help="comma-separated weight per class: w0,w1,...")
    ap.add_argument("--label-smoothing", type=float, default=0.0)
    ap.add_argument("--dice-weight", type=float, default=0.0,
                    help="train on CE + this many times the soft Dice loss of the softmax probabilities (0: CE alone)")
    ap.add_argument("--dice-smooth", type=float, default=1e-6)
    ap.add_argument("--dice-no-background", action="store_true", help="leave class 0 out of the Dice mean")
    ap.add_argument("--focal-gamma", type=float, default=0.0, help="focal loss: damp each pixel's CE by (1 - p_y)^gamma (0: off)")
    ap.add_argument("--ohem-thresh", type=float, default=None,
                    help="OHEM: average over the pixels whose true-class probability lies under this value (0.7 in mmsegmentation)")
    ap.add_argument("--ohem-min-kept", type=int, default=0, help="OHEM: never fewer than this many of the hardest pixels of a batch")
    ap.add_argument("--ohem-keep-fraction", type=float, default=0.0,
                    help="OHEM: never fewer than this fraction of the valid pixels of a batch")
    ap.add_argument("--cldice-weight", type=float, default=0.0,
                    help="add this many times the soft-clDice loss (centre-line Dice on soft skeletons; 0: off)")
    ap.add_argument("--cldice-classes", default=None, help="comma-separated classes the clDice term counts (default: all but 0)")
    ap.add_argument("--cldice-iters", type=int, default=3, help="rounds of min / max pooling of the soft skeleton")
    ap.add_argument("--cldice-smooth", type=float, default=1.0)
    ap.add_argument("--lovasz-weight", type=float, default=0.0,
                    help="add this many times the Lovasz-Softmax loss (the surrogate of the class IoU; 0: off)")
    ap.add_argument("--lovasz-classes", default=None, help="comma-separated classes the Lovasz term counts (default: all)")
    ap.add_argument("--lovasz-per-image", action="store_true", help="sort and average the Lovasz term per image, not over the batch")


def ce_loss_options(a) -> dict:
    """Keyword arguments for LightningViTModel from the flags of `add_ce_loss_arguments` (empty: the plain loss)."""
    kw = {}
    if a.ignore_index is not None:
        kw["ignore_index"] = a.ignore_index
    if a.class_weights:
        try:
            kw["class_weight"] = [float(v) for v in a.class_weights.split(",")]
        except ValueError:
            raise ValueError(f"--class-weights expects comma-separated numbers, got {a.class_weights!r}") from None
    if a.label_smoothing:
        kw["label_smoothing"] = a.label_smoothing
    if getattr(a, "dice_weight", 0.0):
        kw.update(dice_weight=a.dice_weight, dice_smooth=a.dice_smooth, dice_include_background=not a.dice_no_background)
    if getattr(a, "focal_gamma", 0.0):
        kw["focal_gamma"] = a.focal_gamma
    if getattr(a, "ohem_thresh", None) is not None:
        kw["ohem_thresh"] = a.ohem_thresh
    if getattr(a, "ohem_min_kept", 0):
        kw["ohem_min_kept"] = a.ohem_min_kept
    if getattr(a, "ohem_keep_fraction", 0.0):
        kw["ohem_keep_fraction"] = a.ohem_keep_fraction
    if getattr(a, "cldice_weight", 0.0):
        kw.update(cldice_weight=a.cldice_weight, cldice_iters=a.cldice_iters, cldice_smooth=a.cldice_smooth)
        if a.cldice_classes:
            try:
                kw["cldice_classes"] = [int(v) for v in a.cldice_classes.split(",")]
            except ValueError:
                raise ValueError(f"--cldice-classes expects comma-separated class indices, got {a.cldice_classes!r}") from None
    if getattr(a, "lovasz_weight", 0.0):
        kw.update(lovasz_weight=a.lovasz_weight, lovasz_per_image=bool(a.lovasz_per_image))
        if a.lovasz_classes:
            try:
                kw["lovasz_classes"] = [int(v) for v in a.lovasz_classes.split(",")]
            except ValueError:
                raise ValueError(f"--lovasz-classes expects comma-separated class indices, got {a.lovasz_classes!r}") from None
    return kw


_AUGMENT_PRESETS = {
    "flip": dict(hflip=0.5, vflip=0.5, rot90=True),
    "geom": dict(hflip=0.5, vflip=0.5, rot90=True, rotate=15.0, scale=(0.8, 1.25), translate=0.1),
    "full": dict(hflip=0.5, vflip=0.5, rot90=True, rotate=15.0, scale=(0.8, 1.25), translate=0.1, brightness=0.2,
                 contrast=0.2, saturation=0.2),
}


def add_augment_arguments(ap) -> None:
    """The augmentation options of the training scripts (augment.Augmenter): a preset and overrides of its ranges."""
    ap.add_argument("--augment", choices=["none", "flip", "geom", "full"], default="none",
                    help="none: the pixels as they are (the reference); flip: flips + quarter turns; geom: + rotation, scale "
                         "and translate jitter; full: + brightness / contrast / saturation jitter")
    ap.add_argument("--aug-rotate", type=float, default=None, help="degrees: the angle is uniform in [-v, v]")
    ap.add_argument("--aug-scale", default=None, help="LO,HI: the zoom factor is uniform in [LO, HI]")
    ap.add_argument("--aug-translate", type=float, default=None, help="fraction of the frame, uniform in [-v, v] per axis")
    ap.add_argument("--aug-brightness", type=float, default=None)
    ap.add_argument("--aug-contrast", type=float, default=None)
    ap.add_argument("--aug-saturation", type=float, default=None)
    ap.add_argument("--aug-seed", type=int, default=0)


def augmenter_from_args(a, cfg, device):
    """The Augmenter the flags of `add_augment_arguments` describe for a model of configuration `cfg`, or None for
    `--augment none`.  With `--ignore-index` the out-of-frame pixels carry that label and do not count in the loss
    (border "constant"); otherwise the frame's edge is repeated (border "edge")."""
    if a.augment == "none":
        return None
    from .augment import Augmenter
    kw = dict(_AUGMENT_PRESETS[a.augment])
    for name in ("rotate", "translate", "brightness", "contrast", "saturation"):
        v = getattr(a, "aug_" + name)
        if v is not None:
            kw[name] = v
    if a.aug_scale is not None:
        try:
            lo, hi = (float(v) for v in a.aug_scale.split(","))
        except ValueError:
            raise ValueError(f"--aug-scale expects LO,HI, got {a.aug_scale!r}") from None
        kw["scale"] = (lo, hi)
    ignore = getattr(a, "ignore_index", None)
    if ignore is not None:
        kw.update(border="constant", fill_label=ignore)
    return Augmenter(cfg.image_size, device=device, seed=a.aug_seed, **kw)


def add_optim_arguments(ap) -> None:
    """The optimiser options of the training scripts (optim.arena_groups, optim.FusedAdam, optim.warmup_cosine)."""
    ap.add_argument("--layer-decay", type=float, default=None,
                    help="layer-wise learning-rate decay in (0, 1]: the head trains at the full rate, every layer below at this "
                         "factor times the rate of the one above, the embeddings lowest")
    ap.add_argument("--no-decay", nargs="?", const="default", default=None, metavar="LIST|default",
                    help="no weight decay on these tensors: comma-separated among bias,norm,cls,pos (default: all four)")
    ap.add_argument("--freeze", default=None, metavar="embeddings|backbone|K",
                    help="do not train the embeddings, everything but the head, or the embeddings and the first K layers")
    ap.add_argument("--head-lr-mult", type=float, default=None, help="the head's learning rate is this many times the base rate")
    ap.add_argument("--max-grad-norm", type=float, default=None, help="clip the global L2 norm of the gradient to this")
    ap.add_argument("--skip-nonfinite", action="store_true", help="skip an optimiser step whose gradient norm is inf or NaN")
    ap.add_argument("--ema-decay", type=float, default=None,
                    help="keep an exponential moving average of the weights with this decay; validation and ema_state_dict use it")
    ap.add_argument("--weight-decay", type=float, default=None, help="AdamW's decoupled weight decay (FusedAdamW)")
    ap.add_argument("--warmup-steps", type=int, default=None,
                    help="optimiser steps of linear warm-up, followed by a cosine decay over the rest of the run")


def optim_options(a, total_steps=None) -> dict:
    """Keyword arguments for LightningViTModel / PAEDTrainer from the flags of `add_optim_arguments` (empty: the reference's
    optimiser).  `total_steps`: the optimiser steps of the run, passed on with --warmup-steps."""
    kw = {}
    if a.layer_decay is not None:
        kw["layer_decay"] = a.layer_decay
    if a.no_decay is not None:
        kw["no_decay"] = "default" if a.no_decay == "default" else tuple(t.strip() for t in a.no_decay.split(",") if t.strip())
    if a.freeze is not None:
        kw["freeze"] = int(a.freeze) if a.freeze.lstrip("-").isdigit() else a.freeze
    if a.head_lr_mult is not None:
        kw["head_lr_mult"] = a.head_lr_mult
    if a.max_grad_norm is not None:
        kw["max_grad_norm"] = a.max_grad_norm
    if a.skip_nonfinite:
        kw["skip_nonfinite"] = True
    if a.ema_decay is not None:
        kw["ema_decay"] = a.ema_decay
    if a.weight_decay is not None:
        kw["weight_decay"] = a.weight_decay
    if a.warmup_steps is not None:
        kw["warmup_steps"] = a.warmup_steps
        if total_steps is not None:
            kw["total_steps"] = int(total_steps)
    return kw


def optimizer_steps(epochs: int, batches_per_epoch: int, accumulate_grad_batches: int) -> int:
    """The optimiser steps `trainer.fit` takes: one per accumulation window, the epoch's incomplete last window included."""
    return int(epochs) * -(-int(batches_per_epoch) // int(accumulate_grad_batches))


def set_total_steps(model, epochs: int, batches_per_epoch: int, accumulate_grad_batches: int) -> None:
    """Tells a module built with --warmup-steps how long the run is, once its batches are known (before trainer.fit)."""
    if "warmup_steps" in model.optim_options:
        model.optim_options["total_steps"] = optimizer_steps(epochs, batches_per_epoch, accumulate_grad_batches)


def ce_batches(cfg, n_images: int, batch_size: int, data: Optional[str] = None, seed: int = 0, first: int = 0):
    """[(images [b,3,S,S] float, masks [b,256,256] long)]: StructuralDamageDataset items (model/CE/classes.py:60-89)."""
    if data:
        blob = torch.load(data)
        xs, ys = blob["images"].float(), blob["masks"].long()
    else:
        xs = torch.from_numpy(synth.make_images(cfg, n_images, seed=seed, first_image=first))
        ys = torch.from_numpy(synth.make_targets(cfg, n_images, seed=seed, first_image=first))
    return [(xs[i:i + batch_size], ys[i:i + batch_size]) for i in range(0, xs.shape[0], batch_size)]


def paed_binary_batches(cfg, n_images: int, batch_size: int, data: Optional[str] = None, seed: int = 0, sdf_size: int = 224,
                        sdf: str = "standin"):
    """[(images, masks [b,1,h,w] float 0/1, sdf_ext [b,h,w], sdf_int [b,h,w])]: the binary PAED dataset's items
    (model/PAED/classes.py:60-88: mask resized to 224 NEAREST and binarised, SDFs computed from it).  A `data` blob holds
    "images" and either "masks", "sdf_ext", "sdf_int" or the decoded 'L' masks "raw_masks" (uint8 [n, H, W]), whose targets
    Preprocessor.paed_binary_targets computes on the device.  Synthetic masks get smooth stand-in SDFs (`sdf="standin"`)
    or their exact ones from sdf.compute_sdf (`sdf="exact"`)."""
    if sdf not in ("standin", "exact"):
        raise ValueError(f'sdf must be "standin" or "exact", got {sdf!r}')
    if data:
        blob = torch.load(data)
        xs = blob["images"].float()
        if "sdf_ext" not in blob and "raw_masks" in blob:
            from .preprocess import Preprocessor
            dev = f"cuda:{torch.cuda.current_device()}"
            ms, se, si = Preprocessor(cfg.image_size, device=dev).paed_binary_targets(blob["raw_masks"], size=sdf_size)
        else:
            ms, se, si = blob["masks"].float(), blob["sdf_ext"].float(), blob["sdf_int"].float()
    else:
        xs = torch.from_numpy(synth.make_images(cfg, n_images, seed=seed))
        g = torch.Generator().manual_seed(seed + 17)
        # blobs: threshold a smooth random field; the stand-in "SDFs" are smooth non-negative maps of the same size
        field = torch.nn.functional.avg_pool2d(torch.rand(n_images, 1, sdf_size + 30, sdf_size + 30, generator=g), 31, 1)
        ms = (field > field.mean()).float()
        if sdf == "exact":
            from .sdf import compute_sdf
            se, si = compute_sdf(ms[:, 0].to(torch.uint8), device=f"cuda:{torch.cuda.current_device()}")
        else:
            se = (field[:, 0] - field.amin()).clamp_min(0) * 40 * (1 - ms[:, 0])
            si = (field.amax() - field[:, 0]).clamp_min(0) * 40 * ms[:, 0]
    out = []
    for i in range(0, xs.shape[0], batch_size):
        out.append((xs[i:i + batch_size], ms[i:i + batch_size], se[i:i + batch_size], si[i:i + batch_size]))
    return out


def run_validation(model, batches, device) -> dict:
    """trainer.validate / trainer.test of the reference scripts: validation_step over the loader, mean of what it logs."""
    model.eval()
    acc: dict = {}
    for i, batch in enumerate(batches):
        model.validation_step(tuple(t.to(device) for t in batch), i)
        for k, v in model.logged.items():
            if k.startswith("val"):
                acc.setdefault(k, []).append(v.detach().float().reshape(()) if torch.is_tensor(v) else torch.tensor(float(v)))
    return {k: float(torch.stack([t.to("cpu") for t in v]).mean()) for k, v in acc.items()}


def _stem(csv_path: str) -> str:
    """What every file of one evaluation starts with: the metrics file's path without "_metrics.csv" (or its extension)."""
    return csv_path[:-len("_metrics.csv")] if csv_path.endswith("_metrics.csv") else os.path.splitext(csv_path)[0]


def _parse_classes(flag: str, text: Optional[str]):
    """The value of a class-list flag: None (flag absent), "all", or a comma-separated list of label values."""
    if text is None or text == "all":
        return text
    try:
        return [int(t) for t in text.split(",") if t.strip()]
    except ValueError:
        raise ValueError(f'{flag} takes "all" or comma-separated label values, got {text!r}') from None


def parse_props_classes(text: Optional[str]):
    return _parse_classes("--region-props", text)


def add_confidence_arguments(ap) -> None:
    """--region-scores / --score-kind / --score-low / --calibration of the evaluation scripts."""
    ap.add_argument("--region-scores", action="store_true",
                    help="also write <model>_region_scores.csv: one row per predicted region with its confidence score (mean, "
                         "minimum, share of low pixels); with --region-metrics also its matched flag and one pooled AP row per "
                         "class; regions by --region-connectivity")
    ap.add_argument("--score-kind", default="prob", choices=["prob", "margin"],
                    help="a pixel's score: the sigmoid of its class, or its lead over the best other class")
    ap.add_argument("--score-low", type=float, default=0.5, help="pixels scoring below this count as low (0..1)")
    ap.add_argument("--calibration", nargs="?", const=16, type=int, metavar="BINS",
                    help="also write <model>_calibration.csv: the reliability table pooled over all images (default 16 bins, "
                         "1..256) and the expected calibration error")


def confidence_options(ap, a) -> dict:
    """The keywords of `evaluate_to_csv` from the parsed flags; refused when arguments are parsed (ap.error): a score flag
    with --tta, --score-low outside 0..1, BINS outside 1..256."""
    on = a.region_scores or a.calibration is not None
    if on and getattr(a, "tta", None):
        ap.error("--region-scores / --calibration cannot be combined with --tta: the scores are those of one forward")
    if not 0.0 <= a.score_low <= 1.0:
        ap.error(f"--score-low must lie in 0..1, got {a.score_low}")
    if a.calibration is not None and not 1 <= a.calibration <= 256:
        ap.error(f"--calibration takes 1..256 bins, got {a.calibration}")
    return dict(region_scores=a.region_scores, score_kind=a.score_kind, score_low=a.score_low, calibration_bins=a.calibration)


def add_polygon_arguments(ap) -> None:
    """--region-polygons of the evaluation scripts."""
    ap.add_argument("--region-polygons", action="store_true",
                    help="also write <model>_region_polygons.geojson: the outline of every predicted region as a polygon with "
                         "holes, coordinates in units of --pixel-size; regions by --region-connectivity, on the mask that "
                         "--min-area, --fill-holes and --tta produce")


def polygon_options(a, metrics_csv_path: str) -> dict:
    """The keywords of `evaluate_to_csv` from the parsed flags: none without --region-polygons, else `polygons_path`, the
    .geojson file beside the metrics file."""
    return dict(polygons_path=_stem(metrics_csv_path) + "_region_polygons.geojson") if a.region_polygons else {}


def add_crack_graph_arguments(ap) -> None:
    """--crack-graph of the evaluation scripts."""
    ap.add_argument("--crack-graph", nargs="?", const="all", metavar="CLASSES",
                    help="also write <model>_crack_graph.geojson and <model>_crack_branches.csv: the centre-lines of the listed "
                         'classes (comma-separated label values, or "all": every class but the background 0) as a graph -- one '
                         "LineString / one row per branch with its length, widths and ends, then a summary row per image and "
                         "class; lengths and coordinates in units of --pixel-size, on the mask that --min-area, --fill-holes and "
                         "--tta produce")


def crack_graph_options(a, metrics_csv_path: str) -> dict:
    """The keywords of `evaluate_to_csv` from the parsed flags: none without --crack-graph, else the classes (True for "all")
    and the two files beside the metrics file."""
    if a.crack_graph is None:
        return {}
    classes = _parse_classes("--crack-graph", a.crack_graph)
    stem = _stem(metrics_csv_path)
    return dict(crack_graph_classes=True if classes == "all" else classes, crack_graph_path=stem + "_crack_graph.geojson",
                crack_branches_csv_path=stem + "_crack_branches.csv")


def add_curve_arguments(ap) -> None:
    """--pr-curve / --pr-bins / --pr-tolerance of the evaluation scripts (--score-kind is the confidence flags')."""
    ap.add_argument("--pr-curve", nargs="?", const=1, type=int, metavar="CLASS",
                    help="also write <model>_pr_curve.csv: the precision-recall curve of CLASS' score map (default 1) over all "
                         "thresholds, pooled over all images, then the rows ODS, OIS and AP; the score is --score-kind's")
    ap.add_argument("--pr-bins", type=int, default=256, help="thresholds of the curve (1..1024)")
    ap.add_argument("--pr-tolerance", type=float, default=0.0,
                    help="a predicted pixel within this many pixels of a true one is no error, and a true pixel is found by a "
                         "prediction as near (0..16; the crack benchmarks use 2 to 5; 0: the plain pixel curve)")


def curve_options(ap, a) -> dict:
    """The keywords of `evaluate_to_csv` from the parsed flags: none without --pr-curve; refused when arguments are parsed
    (ap.error): the flag with --tta, a class, bin count or tolerance `curves.check_options` refuses."""
    if a.pr_curve is None:
        return {}
    try:
        reports.check_scoring(getattr(a, "tta", None), a.score_kind, a.score_low)
        curves.check_options(a.pr_curve, a.pr_bins, a.pr_tolerance)
    except ValueError as e:
        ap.error(f"--pr-curve: {e}")
    return dict(pr_curve=a.pr_curve, pr_bins=a.pr_bins, pr_tolerance=a.pr_tolerance)


def threshold_options(ap, a) -> dict:
    """The keywords of `evaluate_to_csv` from the parsed flags: none without --threshold; refused when arguments are parsed
    (ap.error): another threshold flag without --threshold, the flags with --tta, thresholds `decide.check_options` refuses (a
    low one above the high one among them) and a class the model lacks."""
    if a.threshold is None:
        if a.threshold_low is not None or a.threshold_over_argmax:
            ap.error("--threshold-low / --threshold-over-argmax need --threshold")
        return {}
    if getattr(a, "tta", None):
        ap.error("--threshold cannot be combined with --tta: the scores are those of one forward")
    try:   # (both scripts have --num-classes; a parser without it leaves the class to evaluate_to_csv)
        _decide.check_model_options(getattr(a, "num_classes", 255), a.threshold_class, a.threshold, a.threshold_low,
                                    a.threshold_connectivity, a.score_kind)
    except ValueError as e:
        ap.error(f"--threshold: {e}")
    return dict(threshold=a.threshold, threshold_low=a.threshold_low, threshold_class=a.threshold_class,
                threshold_connectivity=a.threshold_connectivity, threshold_over_argmax=a.threshold_over_argmax)


def add_evaluation_arguments(ap) -> None:
    """Every flag the two evaluation scripts (model/CE/datasetTestViTmodel.py, model/PAED/ViTscriptTest.py) share."""
    ap.add_argument("--distance-metrics", nargs="?", const="sets", choices=["sets", "borders"],
                    help="also write <model>_distance_metrics.csv: PAED, Hausdorff, HD95 and ASSD per image, between the "
                         "pixel sets of each class (sets, the default) or between their borders")
    ap.add_argument("--crack-metrics", action="store_true",
                    help="also write <model>_crack_metrics.csv: centre-line Dice, crack length and width per image, from the "
                         "Zhang-Suen skeletons of every class but the background 0")
    ap.add_argument("--region-metrics", action="store_true",
                    help="also write <model>_region_metrics.csv: regions found, missed and raised falsely, PQ / SQ / RQ and the "
                         "coverage hit rates per image and class but the background 0, then pooled over all images")
    ap.add_argument("--region-iou", type=float, default=0.5, help="a predicted and a true region match above this IoU (0.5 <= t < 1)")
    ap.add_argument("--region-coverage", type=float, default=0.5, help="a region is found / confirmed from this covered fraction on")
    ap.add_argument("--region-connectivity", type=int, default=4, choices=[4, 8])
    ap.add_argument("--region-props", nargs="?", const="all", metavar="C0,C1,...|all",
                    help="also write <model>_region_props.csv: one row per region of the prediction and of the ground truth "
                         "(position, size, axes, orientation, perimeter, frame contact) and, for the listed classes (default: "
                         "all present but the background 0), the region's own skeleton length and widths; regions by "
                         "--region-connectivity")
    ap.add_argument("--pixel-size", type=float, default=1.0, help="side of a pixel: the unit of the lengths in <model>_region_props.csv and <model>_crack_branches.csv and of the "
                         "coordinates in <model>_region_polygons.geojson and <model>_crack_graph.geojson")
    ap.add_argument("--tta", help='test-time augmentation: "hflip", "flip" or "d4" -- the mask is merged from flipped / '
                                  "quarter-turned views (default: one look)")
    ap.add_argument("--tta-sizes", help="comma-separated sides the views are resampled to, e.g. 160,224 (default: the image size)")
    ap.add_argument("--tta-merge", default="logits", choices=["logits", "probs"], help="mean of the views' logits or of their sigmoids")
    clean.add_arguments(ap)
    add_confidence_arguments(ap)
    add_polygon_arguments(ap)
    add_crack_graph_arguments(ap)
    add_curve_arguments(ap)
    _decide.add_arguments(ap)
    ap.add_argument("--simplify", type=float, metavar="TOL",
                    help="thin the rings of --region-polygons and the polylines of --crack-graph on the device before they are "
                         "written (Douglas-Peucker, tolerance TOL in pixels; ends, ring starts and areas are kept); the features "
                         "gain simplify_tolerance and vertices_full")


def evaluation_options(ap, a, csv_path: str) -> dict:
    """The keywords of `evaluate_to_csv` from the flags of `add_evaluation_arguments`, for the metrics file `csv_path`;
    `confidence_options`' refusals go through ap.error, and so does --simplify without --region-polygons or --crack-graph or
    with a tolerance `simplify.tol2_q8` refuses.  `simplify_tolerance` is in the dict only when the flag is given."""
    thin = {}
    if getattr(a, "simplify", None) is not None:
        if not a.region_polygons and a.crack_graph is None:
            ap.error("--simplify thins the geometry of --region-polygons and --crack-graph: give one of them")
        try:
            _simplify.tol2_q8(a.simplify)
        except ValueError as e:
            ap.error(f"--simplify: {e}")
        thin = dict(simplify_tolerance=a.simplify)
    return dict(**thin, distance_mode=a.distance_metrics, crack_classes=True if a.crack_metrics else None,
                tta=a.tta, tta_sizes=parse_sizes(a.tta_sizes), tta_merge=a.tta_merge,
                region_classes=True if a.region_metrics else None, region_iou=a.region_iou, region_coverage=a.region_coverage,
                region_connectivity=a.region_connectivity, props_classes=parse_props_classes(a.region_props),
                props_pixel_size=a.pixel_size, **clean.arguments(a), **confidence_options(ap, a),
                **polygon_options(a, csv_path), **crack_graph_options(a, csv_path), **curve_options(ap, a),
                **threshold_options(ap, a))


def evaluate_to_csv(model, batches, model_info, csv_path: str, num_classes: int, num_batches: int, device,
                    distance_mode: Optional[str] = None, distance_csv_path: Optional[str] = None, percentile=95,
                    crack_classes=None, crack_csv_path: Optional[str] = None, tta=None, tta_sizes=None, tta_merge: str = "logits",
                    min_area: int = 0, fill_holes: bool = False, max_hole_area: int = 0, region_classes=None,
                    region_csv_path: Optional[str] = None, region_iou=0.5, region_coverage=0.5, region_connectivity: int = 4,
                    props_classes=None, props_csv_path: Optional[str] = None, props_pixel_size: float = 1.0,
                    region_scores: bool = False, score_kind: str = "prob", score_low: float = 0.5,
                    calibration_bins: Optional[int] = None, scores_csv_path: Optional[str] = None,
                    calibration_csv_path: Optional[str] = None, polygons_path: Optional[str] = None, crack_graph_classes=None,
                    crack_graph_path: Optional[str] = None, crack_branches_csv_path: Optional[str] = None,
                    simplify_tolerance=None, pr_curve: Optional[int] = None, pr_bins: int = 256, pr_tolerance=0,
                    pr_curve_csv_path: Optional[str] = None, threshold=None, threshold_low=None, threshold_class: int = 1,
                    threshold_connectivity: int = 4, threshold_over_argmax: bool = False) -> List[list]:
    """The per-image loop of datasetTestViTmodel.py:163-227 / ViTscriptTest.py:160-227: model.eval(), logits.sigmoid(),
    argmax over the class dim, ground truth NEAREST-resized to the prediction, accuracy / mean IoU / mean Dice / class
    sets per image, one CSV row each with the batch's average time per image; returns those rows.  Predictions and class
    statistics stay on the GPU (fused sigmoid -> argmax mask, vitseg_eval_counts).  Every option is validated before the
    model is touched.  The other keywords add files beside the first, which stays as it is; its class in `reports` describes
    each group, a *_path defaults to <csv_path minus "_metrics.csv"> + the report's suffix, a class list may be True (all but 0):
      tta, tta_sizes, tta_merge               every file scores the merged mask of `predict_mask_tta` (default: one look)
      min_area, fill_holes, max_hole_area     every file scores the mask cleaned by clean.clean_mask, inside the time per image
      region_connectivity, props_pixel_size   the regions, and the unit of length, of every report below that has them
      distance_mode, percentile               reports.Distance
      crack_classes                           reports.Crack
      region_classes, region_iou, region_coverage   reports.RegionMetrics
      region_scores, score_kind, score_low    reports.RegionScores (ValueError with tta)
      calibration_bins, score_kind            reports.Calibration (ValueError with tta)
      props_classes (also "all")              reports.RegionProps
      polygons_path                           reports.Outlines
      crack_graph_classes                     reports.CrackGraph
      simplify_tolerance                      the rings / polylines of the two above thinned on the device (pixels; ValueError
                                              without either)
      pr_curve, pr_bins, pr_tolerance, score_kind   reports.PRCurve of class pr_curve (ValueError with tta)
      threshold, threshold_low, threshold_class, threshold_connectivity, threshold_over_argmax, score_kind
                                              every file scores the mask of `predict_threshold` (decide.threshold_mask: class
                                              threshold_class kept where its score reaches `threshold`, with hysteresis down to
                                              `threshold_low`), decided inside the time per image, before the clean-up
                                              (ValueError with tta, or for a class the model lacks)"""
    if simplify_tolerance is not None and polygons_path is None and crack_graph_classes is None:
        raise ValueError("simplify_tolerance needs polygons_path or crack_graph_classes: it thins their geometry")
    min_area, fill_holes, max_hole_area = clean.check_options(min_area, fill_holes, max_hole_area)
    if region_scores or calibration_bins is not None or pr_curve is not None:
        reports.check_scoring(tta, score_kind, score_low)
    crack_classes, region_classes, props_classes, crack_graph_classes = (
        reports.every_class_but_0(c, num_classes) for c in (crack_classes, region_classes, props_classes, crack_graph_classes))
    regions = reports.RegionMetrics(model_info, region_classes, region_iou, region_coverage, bool(region_scores),
                                    region_csv_path) if region_classes else None
    active = [   # in the order of their device calls per batch
        reports.Distance(distance_mode, percentile, distance_csv_path) if distance_mode is not None else None,
        reports.Crack(crack_csv_path, crack_classes) if crack_classes else None,
        regions,
        reports.RegionScores(model_info, score_kind, score_low, regions, scores_csv_path) if region_scores else None,
        reports.Calibration(model_info, calibration_bins, score_kind, calibration_csv_path) if calibration_bins is not None else None,
        reports.RegionProps(props_csv_path, props_classes) if props_classes is not None else None,
        reports.Outlines(polygons_path, simplify_tolerance) if polygons_path is not None else None,
        reports.CrackGraph(crack_graph_classes, crack_graph_path, crack_branches_csv_path,
                           simplify_tolerance) if crack_graph_classes is not None else None,
        reports.PRCurve(model_info, pr_curve, pr_bins, pr_tolerance, score_kind, pr_curve_csv_path) if pr_curve is not None else None,
    ]
    active = [r for r in active if r is not None]
    seg = getattr(model, "model", model)
    if pr_curve is not None and pr_curve >= seg.cfg.num_classes:
        raise ValueError(f"pr_curve must be one of the model's {seg.cfg.num_classes} classes, got {pr_curve}")
    if threshold is None and threshold_low is not None:
        raise ValueError("threshold_low needs threshold")
    if threshold is not None:
        if tta is not None:
            raise ValueError("threshold with tta is not supported: the scores are those of one forward")
        _decide.check_model_options(seg.cfg.num_classes, threshold_class, threshold, threshold_low, threshold_connectivity,
                                    score_kind)
    ev = Evaluator(num_classes, device)
    rows = []
    model.eval()
    for bn, batch in enumerate(batches):
        if bn >= num_batches:
            break
        x, gt = batch[0].to(device), batch[1]
        lowres = None
        torch.cuda.synchronize()
        t0 = time.time()
        with torch.no_grad():
            if tta is not None:
                mask = seg.predict_mask_tta(x, tta=tta, sizes=tta_sizes, merge=tta_merge)
            elif threshold is not None:
                lowres, mask = seg._lowres_and_threshold(x, threshold_class, threshold, threshold_low, threshold_connectivity,
                                                         score_kind, threshold_over_argmax)
            elif any(r.needs_lowres for r in active):
                lowres, mask = seg._lowres_and_mask(x)
            else:
                mask = seg.predict_mask(x)
            if clean.active(min_area, fill_holes):
                mask = clean.clean_mask(mask, min_area=min_area, fill_holes=fill_holes, max_hole_area=max_hole_area)
        torch.cuda.synchronize()
        per_image = (time.time() - t0) / len(x)
        gt = gt.reshape(gt.shape[0], gt.shape[-2], gt.shape[-1])
        for idx, m in enumerate(ev.evaluate(mask, gt)):
            rows.append(csv_row(model_info, bn, idx, m, per_image))
        for r in active:
            r.add(reports.Batch(bn, mask, gt, lowres, ev, model_info, region_connectivity, props_pixel_size))
    os.makedirs(os.path.dirname(os.path.abspath(csv_path)), exist_ok=True)
    write_metrics_csv(csv_path, rows)
    for r in active:
        r.write(_stem(csv_path))
    return rows


