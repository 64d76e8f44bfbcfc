"""`predict()` -- the worker-side call the reference's job dispatcher expects but does not contain.

The reference only ships the single-image script model/CE/testViTModel.py:92-126 (PIL -> Resize ->
ToTensor -> model.eval() -> logits.sigmoid() -> argmax) and a Django view that POSTs the image to an
external orchestrator (backend/core/views.py:97-114).  `predict()` is that script's inference body
as a function: image in, uint8 class-index mask out, computed by libvitseg on the MI355X (the
sigmoid->argmax is fused into the decoder-tail kernel).
"""
from __future__ import annotations

import io
import os
from typing import Optional, Union

import numpy as np
import torch

from .lightning import LightningViTModel
from .model import ViTSegmentationModel

# the nine (patch, hidden, layers, heads) configurations of the reference (testViTModel.py:73-83)
CONFIGURATIONS = {
    0: (16, 768, 12, 12), 1: (16, 512, 8, 8), 2: (16, 1024, 16, 16),
    3: (8, 512, 8, 8), 4: (8, 768, 12, 12), 5: (8, 1024, 16, 16),
    6: (4, 512, 8, 8), 7: (4, 768, 12, 12), 8: (4, 1024, 16, 16),
}


def load_model(model_id_or_config, num_classes: int, checkpoint: Optional[str] = None, *, image_size: int = 224,
               precision: str = "fp32", device="cuda:0", serve_size: Optional[int] = None) -> LightningViTModel:
    """Builds `LightningViTModel` for a reference configuration ID (or a (P, D, L, A) tuple) and loads a
    Lightning checkpoint `{'state_dict': ...}` if given (testViTModel.py:109-119).  `image_size` is the checkpoint's
    (its position table); `serve_size` (default: the same) the side `predict` resizes images to -- when the two differ
    the forward resamples the position table to the served grid (interpolate_pos_encoding)."""
    P, D, L, A = CONFIGURATIONS[model_id_or_config] if isinstance(model_id_or_config, int) else model_id_or_config
    model = LightningViTModel(num_classes, P, D, L, A, image_size=image_size, precision=precision, device=device)
    if checkpoint is not None:
        ck = torch.load(checkpoint, map_location="cpu")
        model.load_state_dict(ck["state_dict"] if "state_dict" in ck else ck)
    model.serve_size = int(serve_size) if serve_size is not None else None
    return model.eval()


def decode(image) -> np.ndarray:
    """PIL image / path / encoded bytes -> uint8 RGB [H, W, 3] (`Image.open(...).convert('RGB')`, classes.py:72)."""
    from PIL import Image
    if isinstance(image, (bytes, bytearray)):
        image = Image.open(io.BytesIO(image))
    elif isinstance(image, (str, os.PathLike)):
        image = Image.open(image)
    if isinstance(image, np.ndarray):
        return np.ascontiguousarray(image, dtype=np.uint8)
    return np.array(image.convert("RGB"), dtype=np.uint8)   # a writable copy (torch.from_numpy wants one)


_PRE = {}


def preprocess(image, size: int, device="cuda:0") -> torch.Tensor:
    """image -> float32 [1, 3, size, size] in [0, 1] on `device`: transforms.Resize((S, S)) [Pillow's antialiased
    bilinear] + ToTensor (testViTModel.py:92-97), computed by libvitseg bit-exactly (preprocess.Preprocessor); only the
    decoded bytes are uploaded."""
    from .preprocess import Preprocessor
    key = (int(size), str(device))
    if key not in _PRE:
        _PRE[key] = Preprocessor(size, device)
    return _PRE[key].images(torch.from_numpy(decode(image)))


def predict(image, model: Union[LightningViTModel, ViTSegmentationModel], *, index_to_color=None,
            return_logits: bool = False, serve_size: Optional[int] = None, return_boxes: bool = False,
            sliding: bool = False, stride: Optional[int] = None, weights: str = "linear", tta=None, tta_sizes=None,
            tta_merge: str = "logits", min_area: int = 0, fill_holes: bool = False, max_hole_area: int = 0,
            return_props: bool = False, props_classes=None, pixel_size: float = 1.0, return_scores: bool = False,
            return_confidence: bool = False, score_kind: str = "prob", low: float = 0.5, return_polygons: bool = False,
            return_centerlines: bool = False, centerline_classes=None, simplify=None, threshold=None, threshold_low=None,
            threshold_class: int = 1, threshold_connectivity: int = 4, threshold_kind: str = "prob",
            threshold_over_argmax: bool = False):
    """uint8 class-index mask [S, S] (numpy) for one image; optionally also an RGB rendering
    `index_to_color[mask]` (testViTModel.py:139-143) and/or the fp32 logits [C, S, S].  S = `serve_size`, else the
    one `load_model` was given, else the model's image size; another size than the model's runs with the position table
    resampled to it (interpolate_pos_encoding).  `return_boxes`: also, last, the reference's "Predicted Regions with
    Boxes" as {class: [(y_min, x_min, y_max, x_max), ...]} for every class present but 0 (testViTModel.py:171-185; the
    4-connected regions of regions.region_boxes, computed on the device).
    `sliding`: the image is NOT resized: its decoded bytes are uploaded and S x S windows `stride` apart run at the image's
    own resolution, blended with `weights` (ViTSegmentationModel.predict_mask_windowed); the mask is [H, W], the logits
    [C, H, W].  An image with a side shorter than S raises ValueError.
    `tta` (default None: one look, as before): test-time augmentation, a preset ("hflip", "flip", "d4", "none") or a
    sequence of ops 0..7; the image is resized to S as usual and the mask is `predict_mask_tta`'s -- the views at the sides
    `tta_sizes` (default (S,)) merged by `tta_merge` ("logits" or "probs"); `return_logits` then returns the merged fp32
    [C, S, S] (probabilities for "probs").  With `sliding` it raises ValueError: TTA inside sliding windows is not built.
    `min_area` / `fill_holes` / `max_hole_area` (defaults: off): the mask, its colour rendering and its boxes are those of
    the mask cleaned on the device by clean.clean_mask (regions below `min_area` pixels to class 0, then enclosed holes of
    at most `max_hole_area` pixels filled), after whichever route made it; the logits are not touched.
    `return_props`: also, last of all, one dict per region of the (cleaned) mask in `region_boxes`' order -- position, size,
    axes, orientation, perimeter, frame contact and, for the classes in `props_classes` (None: none; "all"; or label values),
    the region's own skeleton length and widths (regions.region_props + regions.props_from_records), lengths in units of
    `pixel_size`.
    `return_scores` / `return_confidence` (appended last, in this order): one dict per region of the (cleaned) mask in
    `region_boxes`' order -- class, first, area, score (the mean of its pixels' p), score_min, low_fraction (the share of its
    pixels with p below `low`) -- and the fp32 [S, S] map of p (confidence.region_scores / confidence_map; `score_kind`
    "prob": the sigmoid of the class the mask states, "margin": its lead over the best other class).  The scores are
    re-generated on the device from the low-res head output of the same forward.  With `sliding` or `tta` they raise
    ValueError before anything runs: scoring blended views is not built.
    `return_polygons`: also, last of all, the pair (records, polygons) of polygons.region_polygons for the (cleaned) mask: the
    int32 [k, 7] records of its regions and, per region, its outline as rings of (y, x) pixel corners, the outer ring first,
    then the holes.  It reads the mask alone, so it goes with `sliding` and `tta`.
    `return_centerlines`: also, last of all, the dict class -> (nodes, branches, points) of centerlines.trace for the label
    values `centerline_classes` (required) of the (cleaned) mask: the centre-line graph of each class's skeleton.  It reads the
    mask alone as well.
    `simplify`: a tolerance in pixels for the outlines and the centre-lines (None: as they are traced): both are thinned on
    the device before they are copied back (simplify.simplify_device).  ValueError without `return_polygons` or
    `return_centerlines`.
    `threshold` (default None: the argmax, as before): class `threshold_class` is decided by its score instead
    (ViTSegmentationModel.predict_threshold): a pixel is kept when its score (`threshold_kind`) reaches `threshold`, with
    `threshold_low` also when it reaches that and is `threshold_connectivity`-connected through such pixels to one that reaches
    `threshold`; the others become 0 or, with `threshold_over_argmax`, keep the argmax mask's class.  The mask, its colour
    rendering, boxes, props, scores, polygons and centre-lines are those of the decided mask; the clean-up runs after it.  With
    `sliding` or `tta` it raises ValueError before anything runs: those paths keep no single low-res map."""
    from . import clean as _clean
    _clean.check_options(min_area, fill_holes, max_hole_area)
    if simplify is not None:
        from .simplify import tol2_q8
        tol2_q8(simplify)
        if not (return_polygons or return_centerlines):
            raise ValueError("simplify needs return_polygons or return_centerlines: it thins their geometry")
    if return_centerlines:
        from . import centerlines as _centerlines
        if centerline_classes is None:
            raise ValueError("return_centerlines needs centerline_classes, a sequence of label values")
        _centerlines.check_options(centerline_classes)
    scoring = bool(return_scores or return_confidence)
    if scoring:
        from . import confidence as _conf
        if sliding or tta is not None:
            raise ValueError("return_scores / return_confidence with sliding=True or tta= is not supported: the scores are "
                             "those of one forward of the resized image")
        if score_kind not in _conf.KINDS:
            raise ValueError(f"score_kind must be one of {sorted(_conf.KINDS)}, got {score_kind!r}")
        _conf.low_to_q(low)
    deciding = threshold is not None
    if deciding or threshold_low is not None:
        from . import decide as _decide
        if sliding or tta is not None:
            raise ValueError("threshold with sliding=True or tta= is not supported: the scores are those of one forward of the "
                             "resized image")
        if not deciding:
            raise ValueError("threshold_low needs threshold")
    seg = model.model if isinstance(model, LightningViTModel) else model
    if deciding:
        decide_args = (threshold_class, threshold, threshold_low, threshold_connectivity, threshold_kind)
        value = _decide.check_model_options(seg.cfg.num_classes, *decide_args)
    S = serve_size if serve_size is not None else getattr(model, "serve_size", None)
    S = seg.cfg.image_size if S is None else int(S)
    if tta is not None and sliding:
        raise ValueError("tta with sliding=True is not supported: test-time augmentation runs on the resized image")
    if tta is not None:
        x = preprocess(image, S, seg.arena.device)
        out = seg.predict_mask_tta(x, tta=tta, sizes=tta_sizes, merge=tta_merge, return_merged=return_logits)
    elif sliding:
        img = torch.from_numpy(decode(image))
        if img.dim() != 3 or min(img.shape[0], img.shape[1]) < S:
            raise ValueError(f"sliding-window prediction needs an image of at least {S}x{S}, got "
                             f"{tuple(img.shape[:2])[0]}x{tuple(img.shape[:2])[1]}")
        out = seg.predict_mask_windowed(img[None].to(seg.arena.device), stride=stride, weights=weights, window_size=S,
                                        return_logits=return_logits)
    elif deciding and not return_logits:   # one encoder pass that keeps the low-res head output
        x = preprocess(image, S, seg.arena.device)
        with torch.no_grad():
            lowres, out = seg._lowres_and_threshold(x, *decide_args, bool(threshold_over_argmax), S != seg.cfg.image_size)
    elif scoring and not return_logits:   # one encoder pass that keeps the low-res head output; predict_mask's mask
        x = preprocess(image, S, seg.arena.device)
        with torch.no_grad():
            lowres, out = seg._lowres_and_mask(x, S != seg.cfg.image_size)
    else:
        x = preprocess(image, S, seg.arena.device)
        out = seg.predict_mask(x, return_logits=return_logits, interpolate_pos_encoding=S != seg.cfg.image_size)
        if scoring or deciding:
            lowres = out[1]   # the full-size logits are there already: scored as they stand (g == S)
        if deciding:
            out = (_decide.threshold_mask(lowres, threshold_class, threshold, threshold_low, threshold_connectivity, threshold_kind,
                                          base=out[0] if threshold_over_argmax else None, value=value, size=S), out[1])
    mask_dev = (out[0] if return_logits else out)[0]
    if _clean.active(min_area, fill_holes):
        mask_dev = _clean.clean_mask(mask_dev, min_area=min_area, fill_holes=fill_holes, max_hole_area=max_hole_area)
    boxes = None
    if return_boxes:
        from .regions import boxes_by_class, region_boxes
        boxes = boxes_by_class(region_boxes(mask_dev))
    props = None
    if return_props:
        from .regions import props_from_records, region_props
        props = props_from_records(region_props(mask_dev, skeleton_classes=props_classes), pixel_size)
    region_scores = conf_map = None
    if return_scores:
        region_scores = _conf.region_dicts(*_conf.region_scores(lowres[0], mask_dev, kind=score_kind, low=low))
    if return_confidence:
        conf_map = _conf.confidence_map(lowres[0], mask_dev, kind=score_kind).cpu().numpy()
    polygons = None
    if return_polygons:
        from .polygons import region_polygons
        polygons = region_polygons(mask_dev, simplify=simplify)
    graph = None
    if return_centerlines:
        graph = _centerlines.trace(mask_dev, classes=centerline_classes, simplify=simplify)
    mask = mask_dev.cpu().numpy()
    res = [mask]
    if index_to_color is not None:
        res.append(np.asarray(index_to_color, dtype=np.uint8)[mask])
    if return_logits:
        res.append(out[1][0].cpu().numpy())
    if return_boxes:
        res.append(boxes)
    if return_props:
        res.append(props)
    if return_scores:
        res.append(region_scores)
    if return_confidence:
        res.append(conf_map)
    if return_polygons:
        res.append(polygons)
    if return_centerlines:
        res.append(graph)
    return res[0] if len(res) == 1 else tuple(res)
