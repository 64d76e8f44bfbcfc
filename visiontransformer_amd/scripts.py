"""What the reference's train / evaluation scripts share (model/CE/*.py, model/PAED/*.py), for the thin drivers under
model/: batches (the reference's dataset VisionChallenge/ is private, so synthetic tensors unless --data points at a
torch.save'd dict), checkpoint discovery with the reference's rule, and the per-image evaluation loop + CSV.
"""
from __future__ import annotations

import json
import os
import re
import time
from typing import List, Optional

import numpy as np
import torch

from . import synth
from .metrics import (Evaluator, crack_csv_row, csv_row, distance_csv_row, matches_from_stats, pool_region_stats,
                      region_csv_row, write_crack_csv, write_distance_csv, write_metrics_csv, write_region_csv)
from .regions import props_csv_row, write_props_csv


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


def parse_props_classes(text: Optional[str]):
    """The value of --region-props: None (flag absent), "all", or a comma-separated list of label values."""
    if text is None or text == "all":
        return text
    try:
        return [int(t) for t in text.split(",") if t.strip()]
    except ValueError:
        raise ValueError(f'--region-props takes "all" or comma-separated label values, got {text!r}') from None


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
    if not a.region_polygons:
        return {}
    stem = metrics_csv_path[:-len("_metrics.csv")] if metrics_csv_path.endswith("_metrics.csv") else os.path.splitext(metrics_csv_path)[0]
    return dict(polygons_path=stem + "_region_polygons.geojson")


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
    if a.crack_graph == "all":
        classes = True
    else:
        try:
            classes = [int(t) for t in a.crack_graph.split(",") if t.strip()]
        except ValueError:
            raise ValueError(f'--crack-graph takes "all" or comma-separated label values, got {a.crack_graph!r}') from None
    stem = metrics_csv_path[:-len("_metrics.csv")] if metrics_csv_path.endswith("_metrics.csv") else os.path.splitext(metrics_csv_path)[0]
    return dict(crack_graph_classes=classes, crack_graph_path=stem + "_crack_graph.geojson",
                crack_branches_csv_path=stem + "_crack_branches.csv")


def evaluate_to_csv(model, batches, model_info, csv_path: str, num_classes: int, num_batches: int, device,
                    distance_mode: Optional[str] = None, distance_csv_path: Optional[str] = None,
                    percentile=95, crack_classes=None, crack_csv_path: Optional[str] = None, tta=None, tta_sizes=None,
                    tta_merge: str = "logits", min_area: int = 0, fill_holes: bool = False,
                    max_hole_area: int = 0, region_classes=None, region_csv_path: Optional[str] = None, region_iou=0.5,
                    region_coverage=0.5, region_connectivity: int = 4, props_classes=None,
                    props_csv_path: Optional[str] = None, props_pixel_size: float = 1.0, region_scores: bool = False,
                    score_kind: str = "prob", score_low: float = 0.5, calibration_bins: Optional[int] = None,
                    scores_csv_path: Optional[str] = None, calibration_csv_path: Optional[str] = None,
                    polygons_path: Optional[str] = None, crack_graph_classes=None, crack_graph_path: Optional[str] = None,
                    crack_branches_csv_path: Optional[str] = None) -> List[list]:
    """The per-image loop of datasetTestViTmodel.py:163-227 / ViTscriptTest.py:160-227: model.eval(), logits.sigmoid(),
    argmax over the class dim, ground truth NEAREST-resized to the prediction, accuracy / mean IoU / mean Dice / class
    sets per image, one CSV row each with the batch's average time per image.  Predictions and class statistics stay on
    the GPU (fused sigmoid -> argmax mask, vitseg_eval_counts).  distance_mode "sets" / "borders": the boundary distances of
    every image (Evaluator.distance_metrics: PAED, Hausdorff, its percentile, ASSD) go to a second file, distance_csv_path
    (default: <csv_path minus "_metrics.csv">_distance_metrics.csv); the first file is the same with and without it.
    crack_classes (a list of label values, or True for every class but 0): clDice, crack length and width of every image
    (Evaluator.crack_metrics) go to crack_csv_path (default: ..._crack_metrics.csv), again beside the unchanged first file.
    tta (default None: one look): a test-time-augmentation preset or op sequence; every file then scores the merged mask of
    `predict_mask_tta` (views at tta_sizes, default the batch's own size, merged by tta_merge).
    min_area / fill_holes / max_hole_area (defaults: off): every file scores the mask cleaned on the device by
    clean.clean_mask (regions below min_area pixels to class 0, then enclosed holes of at most max_hole_area pixels filled);
    the clean-up is part of the time per image.
    region_classes (a list of label values, or True for every class but 0): the region-level detection statistics of every
    image and class (Evaluator.region_metrics at region_iou / region_coverage / region_connectivity) go to region_csv_path
    (default: ..._region_metrics.csv), followed by one row per class of the integers pooled over all images.
    props_classes (None: off; a list of label values, "all", or True for every class but 0 -- the classes whose regions also get
    their own skeleton length and widths; an empty list measures shape alone): one row per region of the prediction and of the
    ground truth (Evaluator.region_props at region_connectivity, lengths in units of props_pixel_size) goes to props_csv_path
    (default: ..._region_props.csv), with a Source column pred / gt.
    region_scores (default off): one row per predicted region -- class, first, area, score, score_min, low_fraction
    (confidence.region_scores with score_kind / score_low at region_connectivity, on the cleaned mask when the clean-up is
    on) -- goes to scores_csv_path (default: ..._region_scores.csv).  With region_classes the row also holds the region's
    `matched` flag, joined on `first` to Evaluator.region_metrics(return_matches=True), and one pooled AP row per class
    follows (confidence.average_precision over all images' regions of the class against the pooled n_gt).
    calibration_bins (None: off): the reliability table pooled over all images (confidence.calibration_hist of the mask against
    the resized ground truth, the integers added before any ratio) and its ECE go to calibration_csv_path (default:
    ..._calibration.csv).  Either makes the forward keep its low-res head output (one encoder pass, predict_mask's mask bit
    for bit); with tta they raise ValueError: scoring merged views is not built.
    polygons_path (None: off): the outlines of every predicted region of the (cleaned, merged) mask
    (polygons.region_polygons at region_connectivity, coordinates in units of props_pixel_size) go to that file as one GeoJSON
    FeatureCollection, each feature carrying its image as image_id "<batch>/<index>" and its batch_num / image_idx.
    crack_graph_classes (None: off; a list of label values, or True for every class but 0): the centre-line graph of each class
    of the (cleaned, merged) mask (Evaluator.crack_graph, lengths and coordinates in units of props_pixel_size) goes to
    crack_graph_path (default: ..._crack_graph.geojson) as one FeatureCollection of LineStrings, tagged like the outlines, and
    to crack_branches_csv_path (default: ..._crack_branches.csv): one row per branch, then a summary row per image and class."""
    from . import clean as _clean
    from . import confidence as _conf
    min_area, fill_holes, max_hole_area = _clean.check_options(min_area, fill_holes, max_hole_area)
    scoring = bool(region_scores) or calibration_bins is not None
    if scoring:
        if tta is not None:
            raise ValueError("region_scores / calibration_bins with tta are not supported: the scores are those of one forward")
        if score_kind not in _conf.KINDS:
            raise ValueError(f"score_kind must be one of {sorted(_conf.KINDS)}, got {score_kind!r}")
        _conf.low_to_q(score_low)
        if calibration_bins is not None and (isinstance(calibration_bins, bool) or not isinstance(calibration_bins, int)
                                             or not 1 <= calibration_bins <= _conf.MAX_BINS):
            raise ValueError(f"calibration_bins must be None or an integer in 1..{_conf.MAX_BINS}, got {calibration_bins!r}")
    seg = getattr(model, "model", model)
    ev = Evaluator(num_classes, device)
    rows, drows, crows, rrows, rstats, prows = [], [], [], [], [], []
    srows, ranked, pooled_hist = [], {}, None
    features = []
    if props_classes is True:
        props_classes = list(range(1, num_classes))
    if crack_classes is True:
        crack_classes = list(range(1, num_classes))
    if region_classes is True:
        region_classes = list(range(1, num_classes))
    if crack_graph_classes is True:
        crack_graph_classes = list(range(1, num_classes))
    if crack_graph_classes is not None:
        from . import centerlines as _cl
        crack_graph_classes = _cl.check_options(crack_graph_classes)
        lines, brows = [], []
    model.eval()
    for bn, batch in enumerate(batches):
        if bn >= num_batches:
            break
        x, gt = batch[0].to(device), batch[1]
        torch.cuda.synchronize()
        t0 = time.time()
        with torch.no_grad():
            if tta is not None:
                mask = seg.predict_mask_tta(x, tta=tta, sizes=tta_sizes, merge=tta_merge)
            elif scoring:
                lowres, mask = seg._lowres_and_mask(x)
            else:
                mask = seg.predict_mask(x)
            if _clean.active(min_area, fill_holes):
                mask = _clean.clean_mask(mask, min_area=min_area, fill_holes=fill_holes, max_hole_area=max_hole_area)
        torch.cuda.synchronize()
        per_image = (time.time() - t0) / len(x)
        gt = gt.reshape(gt.shape[0], gt.shape[-2], gt.shape[-1])
        for idx, m in enumerate(ev.evaluate(mask, gt)):
            rows.append(csv_row(model_info, bn, idx, m, per_image))
        if distance_mode is not None:
            for idx, m in enumerate(ev.distance_metrics(mask, gt, mode=distance_mode, percentile=percentile)):
                drows.append(distance_csv_row(model_info, bn, idx, distance_mode, percentile, m))
        if crack_classes:
            for idx, m in enumerate(ev.crack_metrics(mask, gt, classes=crack_classes)):
                crows.append(crack_csv_row(model_info, bn, idx, m))
        matched = None   # per image {(class, first): the predicted region has a partner}
        if region_classes:
            extra = dict(return_matches=True) if region_scores else {}
            found = ev.region_metrics(mask, gt, classes=region_classes, iou_threshold=region_iou, coverage=region_coverage,
                                      connectivity=region_connectivity, **extra)
            for idx, m in enumerate(found):
                rstats.append(m["stats"])
                for c, r in m["per_class"].items():
                    rrows.append(region_csv_row(model_info, bn, idx, c, region_iou, region_coverage, r))
            if region_scores:
                matched = [{(int(r[0]), int(r[6])): int(r[7]) >= 0 for r in m["matches"]["pred"]} for m in found]
        if region_scores:
            recs, srow = _conf.region_scores(lowres, mask, kind=score_kind, low=score_low, connectivity=region_connectivity)
            for idx, (rec, row) in enumerate(zip(recs, srow)):
                for r, d in enumerate(_conf.region_dicts(rec, row)):
                    flag = "" if matched is None else matched[idx].get((d["class"], d["first"]), "")
                    if flag != "":
                        ranked.setdefault(d["class"], []).append((d["score"], flag))
                    srows.append([model_info[0], model_info[1], bn, idx, r, d["class"], d["first"], d["area"], d["score"],
                                  d["score_min"], d["low_fraction"], "" if flag == "" else int(flag), "", ""])
        if calibration_bins is not None:
            h = _conf.calibration_hist(lowres, mask, ev.resized_gt(gt, mask), bins=calibration_bins, kind=score_kind)
            pooled_hist = h.sum(axis=0) if pooled_hist is None else pooled_hist + h.sum(axis=0)
        if props_classes is not None:
            for idx, m in enumerate(ev.region_props(mask, gt, skeleton_classes=props_classes, connectivity=region_connectivity,
                                                    pixel_size=props_pixel_size)):
                for source in ("pred", "gt"):
                    for r, d in enumerate(m[source]):
                        prows.append(props_csv_row(source, model_info, bn, idx, r, d))
        if polygons_path is not None:
            from . import polygons as _poly
            for idx, (rec, rings) in enumerate(_poly.region_polygons(mask, connectivity=region_connectivity)):
                for f in _poly.polygons_to_geojson(rec, rings, pixel_size=props_pixel_size, image_id=f"{bn}/{idx}")["features"]:
                    f["properties"].update(model_id=model_info[0], model_name=model_info[1], batch_num=bn, image_idx=idx)
                    features.append(f)
        if crack_graph_classes is not None:
            for idx, per_class in enumerate(ev.crack_graph(mask, crack_graph_classes, pixel_size=props_pixel_size)):
                for c, g in per_class.items():
                    found = _cl.centerlines_to_geojson(g["branches"], g["points"], pixel_size=props_pixel_size,
                                                       image_id=f"{bn}/{idx}", class_id=c)["features"]
                    for f in found:
                        f["properties"].update(model_id=model_info[0], model_name=model_info[1], batch_num=bn, image_idx=idx)
                    lines += found
                    brows += _cl.csv_rows(model_info, bn, idx, c, g["table"], g["summary"])
    os.makedirs(os.path.dirname(os.path.abspath(csv_path)), exist_ok=True)
    write_metrics_csv(csv_path, rows)
    stem = csv_path[:-len("_metrics.csv")] if csv_path.endswith("_metrics.csv") else os.path.splitext(csv_path)[0]
    if distance_mode is not None:
        if distance_csv_path is None:
            distance_csv_path = stem + "_distance_metrics.csv"
        write_distance_csv(distance_csv_path, drows)
    if crack_classes:
        write_crack_csv(crack_csv_path or stem + "_crack_metrics.csv", crows)
    if region_classes:
        if rstats:
            for c, r in zip(region_classes, matches_from_stats(pool_region_stats(rstats))):
                rrows.append(region_csv_row(model_info, "pooled", "", c, region_iou, region_coverage, r))
        write_region_csv(region_csv_path or stem + "_region_metrics.csv", rrows)
    if props_classes is not None:
        write_props_csv(props_csv_path or stem + "_region_props.csv", prows)
    if region_scores:
        if region_classes and rstats:
            n_gt = pool_region_stats(rstats)[:, 0]
            for c, k in zip(region_classes, n_gt):
                det = ranked.get(c, [])
                ap = _conf.average_precision([s for s, _ in det], [f for _, f in det], int(k))
                srows.append([model_info[0], model_info[1], "pooled", "", "", c, "", "", "", "", "", "", ap, int(k)])
        _conf.write_csv(scores_csv_path or stem + "_region_scores.csv", _conf.SCORES_CSV_COLUMNS, srows)
    if calibration_bins is not None:
        _conf.write_csv(calibration_csv_path or stem + "_calibration.csv", _conf.CALIBRATION_CSV_COLUMNS,
                        _conf.calibration_csv_rows(model_info, pooled_hist, calibration_bins))
    if polygons_path is not None:
        with open(polygons_path, "w") as f:
            json.dump({"type": "FeatureCollection", "features": features}, f)
    if crack_graph_classes is not None:
        with open(crack_graph_path or stem + "_crack_graph.geojson", "w") as f:
            json.dump({"type": "FeatureCollection", "features": lines}, f)
        _cl.write_csv(crack_branches_csv_path or stem + "_crack_branches.csv", brows)
    return rows
