"""The optional outputs of the dataset evaluation (`scripts.evaluate_to_csv`): one report per file, or pair of files, beside
<model>_metrics.csv.  A report's constructor takes and validates its own options, `add(batch)` appends the rows of one batch
-- after the timed forward, never inside it -- and `write(stem)` writes its file to the path given, else to stem + suffix.
Every report scores the mask the evaluation hands it: cleaned and merged from augmented views when those options are on."""
from __future__ import annotations

import json
from collections import namedtuple
from typing import Optional, Sequence

import numpy as np

from . import centerlines, confidence, curves, polygons
from .simplify import tol2_q8
from ._common import write_csv
from .metrics import (CRACK_CSV_COLUMNS, DISTANCE_CSV_COLUMNS, REGION_CSV_COLUMNS, crack_csv_row, distance_csv_row,
                      matches_from_stats, pool_region_stats, region_csv_row)
from .regions import PROPS_CSV_COLUMNS, props_csv_row


# What a report sees of one batch: its number, the mask (uint8 [n, S, S] on the device), the ground truth as [n, H, W], the
# low-res head output (None unless a report `needs_lowres`), then what the run shares: region_connectivity, props_pixel_size.
# The reports that end on pooled rows are also built with model_info: they write it whether or not a batch came.
Batch = namedtuple("Batch", "bn mask gt lowres ev model_info connectivity pixel_size")


def every_class_but_0(classes, num_classes: int):
    """`classes` as given, except True: the label values 1..num_classes - 1."""
    return list(range(1, num_classes)) if classes is True else classes


def check_scoring(tta, score_kind, score_low) -> None:
    """What the confidence reports and the curve refuse: the scores are those of one forward, scoring merged views is not built."""
    if tta is not None:
        raise ValueError("region_scores / calibration_bins / pr_curve with tta are not supported: the scores are those of one "
                         "forward")
    if score_kind not in confidence.KINDS:
        raise ValueError(f"score_kind must be one of {sorted(confidence.KINDS)}, got {score_kind!r}")
    confidence.low_to_q(score_low)


def _feature_collection(path: str, features: list) -> None:
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "features": features}, f)


def _tagged(features: list, b: Batch, idx: int) -> list:
    for f in features:
        f["properties"].update(model_id=b.model_info[0], model_name=b.model_info[1], batch_num=b.bn, image_idx=idx)
    return features


class Report:
    """One CSV file of `columns`; a subclass sets `suffix` and fills `rows` in `add`.  `classes`: the label values of a report
    that has them, True already expanded."""
    needs_lowres = False   # the forward keeps its low-res head output (one encoder pass, predict_mask's mask bit for bit)
    suffix = columns = None

    def __init__(self, path: Optional[str] = None, classes=None):
        self.path, self.classes, self.rows = path, classes, []

    def write(self, stem: str) -> None:
        write_csv(self.path or stem + self.suffix, self.columns, self.rows)


class Distance(Report):
    """distance_mode "sets" / "borders": the boundary distances of every image (Evaluator.distance_metrics: PAED, Hausdorff,
    its percentile, ASSD)."""
    suffix, columns = "_distance_metrics.csv", DISTANCE_CSV_COLUMNS

    def __init__(self, mode: str, percentile=95, path=None):
        super().__init__(path)
        self.mode, self.percentile = mode, percentile

    def add(self, b: Batch) -> None:
        for idx, m in enumerate(b.ev.distance_metrics(b.mask, b.gt, mode=self.mode, percentile=self.percentile)):
            self.rows.append(distance_csv_row(b.model_info, b.bn, idx, self.mode, self.percentile, m))


class Crack(Report):
    """crack_classes: clDice, crack length and width of every image (Evaluator.crack_metrics)."""
    suffix, columns = "_crack_metrics.csv", CRACK_CSV_COLUMNS

    def add(self, b: Batch) -> None:
        for idx, m in enumerate(b.ev.crack_metrics(b.mask, b.gt, classes=self.classes)):
            self.rows.append(crack_csv_row(b.model_info, b.bn, idx, m))


class RegionMetrics(Report):
    """region_classes: the region-level detection statistics of every image and class (Evaluator.region_metrics at region_iou /
    region_coverage / region_connectivity), followed by one row per class of the integers pooled over all images.
    keep_matches (the scores report is on): `matched` holds, per image of the last batch, {(class, first): the predicted region
    has a partner}."""
    suffix, columns = "_region_metrics.csv", REGION_CSV_COLUMNS

    def __init__(self, model_info: Sequence, classes, iou=0.5, coverage=0.5, keep_matches: bool = False, path=None):
        super().__init__(path, classes)
        self.model_info, self.iou, self.coverage, self.keep_matches = model_info, iou, coverage, keep_matches
        self.stats, self.matched = [], None

    def add(self, b: Batch) -> None:
        found = b.ev.region_metrics(b.mask, b.gt, classes=self.classes, iou_threshold=self.iou, coverage=self.coverage,
                                    connectivity=b.connectivity, return_matches=self.keep_matches)
        for idx, m in enumerate(found):
            self.stats.append(m["stats"])
            for c, r in m["per_class"].items():
                self.rows.append(region_csv_row(b.model_info, b.bn, idx, c, self.iou, self.coverage, r))
        if self.keep_matches:
            self.matched = [{(int(r[0]), int(r[6])): int(r[7]) >= 0 for r in m["matches"]["pred"]} for m in found]

    def write(self, stem: str) -> None:
        if self.stats:
            for c, r in zip(self.classes, matches_from_stats(pool_region_stats(self.stats))):
                self.rows.append(region_csv_row(self.model_info, "pooled", "", c, self.iou, self.coverage, r))
        super().write(stem)


class RegionScores(Report):
    """region_scores: one row per predicted region -- class, first, area, score, score_min, low_fraction
    (confidence.region_scores with score_kind / score_low at region_connectivity).  With the region-metrics report (`regions`,
    else None) the row also holds the region's `matched` flag, joined on (class, first) to
    Evaluator.region_metrics(return_matches=True), and one pooled AP row per class follows (confidence.average_precision over
    all images' regions of the class against the pooled n_gt)."""
    needs_lowres = True
    suffix, columns = "_region_scores.csv", confidence.SCORES_CSV_COLUMNS

    def __init__(self, model_info: Sequence, kind="prob", low=0.5, regions: Optional[RegionMetrics] = None, path=None):
        super().__init__(path)
        self.model_info, self.kind, self.low, self.regions, self.ranked = model_info, kind, low, regions, {}

    def add(self, b: Batch) -> None:
        matched = None if self.regions is None else self.regions.matched   # of this batch: region metrics run first
        recs, srow = confidence.region_scores(b.lowres, b.mask, kind=self.kind, low=self.low, connectivity=b.connectivity)
        for idx, (rec, row) in enumerate(zip(recs, srow)):
            for r, d in enumerate(confidence.region_dicts(rec, row)):
                flag = "" if matched is None else matched[idx].get((d["class"], d["first"]), "")
                if flag != "":
                    self.ranked.setdefault(d["class"], []).append((d["score"], flag))
                self.rows.append([b.model_info[0], b.model_info[1], b.bn, idx, r, d["class"], d["first"], d["area"], d["score"],
                                  d["score_min"], d["low_fraction"], "" if flag == "" else int(flag), "", ""])

    def write(self, stem: str) -> None:
        if self.regions is not None and self.regions.stats:
            for c, k in zip(self.regions.classes, pool_region_stats(self.regions.stats)[:, 0]):
                det = self.ranked.get(c, [])
                ap = confidence.average_precision([s for s, _ in det], [f for _, f in det], int(k))
                self.rows.append([self.model_info[0], self.model_info[1], "pooled", "", "", c, "", "", "", "", "", "", ap, int(k)])
        super().write(stem)


class Calibration(Report):
    """calibration_bins: the reliability table pooled over all images (confidence.calibration_hist of the mask against the
    resized ground truth, the integers added before any ratio) and its ECE."""
    needs_lowres = True
    suffix, columns = "_calibration.csv", confidence.CALIBRATION_CSV_COLUMNS

    def __init__(self, model_info: Sequence, bins: int, kind: str = "prob", path=None):
        super().__init__(path)
        if isinstance(bins, bool) or not isinstance(bins, int) or not 1 <= bins <= confidence.MAX_BINS:   # no numpy integer
            raise ValueError(f"calibration_bins must be None or an integer in 1..{confidence.MAX_BINS}, got {bins!r}")
        self.model_info, self.bins, self.kind, self.hist = model_info, bins, kind, None

    def add(self, b: Batch) -> None:
        h = confidence.calibration_hist(b.lowres, b.mask, b.ev.resized_gt(b.gt, b.mask), bins=self.bins, kind=self.kind)
        self.hist = h.sum(axis=0) if self.hist is None else self.hist + h.sum(axis=0)

    def write(self, stem: str) -> None:
        self.rows = confidence.calibration_csv_rows(self.model_info, self.hist, self.bins)
        super().write(stem)


class PRCurve(Report):
    """pr_curve: the precision-recall curve of one class' score map over all thresholds (curves.pr_counts of the low-res head
    output against the resized ground truth, at `bins` thresholds and a tolerance in pixels), the integers of all images added
    before any ratio: one row per threshold, then the rows ODS, OIS and AP.  It scores the probability map, not the mask."""
    needs_lowres = True
    suffix, columns = "_pr_curve.csv", curves.CSV_COLUMNS

    def __init__(self, model_info: Sequence, cls: int = 1, bins: int = 256, tolerance=0, kind: str = "prob", path=None):
        super().__init__(path)
        curves.check_options(cls, bins, tolerance)
        self.model_info, self.cls, self.bins, self.tolerance, self.kind, self.counts = model_info, cls, bins, tolerance, kind, []

    def add(self, b: Batch) -> None:
        self.counts.append(curves.pr_counts(b.lowres, b.ev.resized_gt(b.gt, b.mask), cls=self.cls, bins=self.bins,
                                            tolerance=self.tolerance, kind=self.kind))

    def write(self, stem: str) -> None:
        counts = np.concatenate(self.counts) if self.counts else np.zeros((0, self.bins, 3), np.int64)
        self.rows = curves.csv_rows(self.model_info, counts, self.cls, self.tolerance)
        super().write(stem)


class RegionProps(Report):
    """props_classes (a list of label values or "all": the classes whose regions also get their own skeleton length and widths;
    an empty list measures shape alone): one row per region of the prediction and of the ground truth (Evaluator.region_props
    at region_connectivity, lengths in units of props_pixel_size), with a Source column pred / gt."""
    suffix, columns = "_region_props.csv", PROPS_CSV_COLUMNS

    def add(self, b: Batch) -> None:
        for idx, m in enumerate(b.ev.region_props(b.mask, b.gt, skeleton_classes=self.classes, connectivity=b.connectivity,
                                                  pixel_size=b.pixel_size)):
            for source in ("pred", "gt"):
                for r, d in enumerate(m[source]):
                    self.rows.append(props_csv_row(source, b.model_info, b.bn, idx, r, d))


class Outlines(Report):
    """polygons_path: the outlines of every predicted region (polygons.region_polygons at region_connectivity, coordinates in
    units of props_pixel_size) as one GeoJSON FeatureCollection, each feature carrying its image as image_id "<batch>/<index>"
    and its batch_num / image_idx.  `simplify`: a tolerance in pixels, the rings thinned on the device; the features then also
    carry simplify_tolerance and vertices_full."""

    def __init__(self, path=None, simplify=None):
        super().__init__(path)
        if simplify is not None:
            tol2_q8(simplify)
        self.simplify = simplify

    def add(self, b: Batch) -> None:
        for idx, (rec, rings) in enumerate(polygons.region_polygons(b.mask, connectivity=b.connectivity, simplify=self.simplify)):
            found = polygons.polygons_to_geojson(rec, rings, pixel_size=b.pixel_size, image_id=f"{b.bn}/{idx}")["features"]
            self.rows += _tagged(found, b, idx)

    def write(self, stem: str) -> None:
        _feature_collection(self.path, self.rows)


class CrackGraph(Report):
    """crack_graph_classes: the centre-line graph of each class (Evaluator.crack_graph, lengths and coordinates in units of
    props_pixel_size) as one FeatureCollection of LineStrings, tagged like the outlines, and as a CSV file: one row per branch,
    then a summary row per image and class.  `simplify`: a tolerance in pixels, the polylines thinned on the device; the
    features then also carry simplify_tolerance and vertices_full, the CSV rows the kept point count."""
    suffix, columns = "_crack_branches.csv", centerlines.CSV_COLUMNS

    def __init__(self, classes, graph_path=None, path=None, simplify=None):
        super().__init__(path, centerlines.check_options(classes))
        if simplify is not None:
            tol2_q8(simplify)
        self.graph_path, self.lines, self.simplify = graph_path, [], simplify

    def add(self, b: Batch) -> None:
        kw = {} if self.simplify is None else dict(simplify=self.simplify)
        for idx, per_class in enumerate(b.ev.crack_graph(b.mask, self.classes, pixel_size=b.pixel_size, **kw)):
            for c, g in per_class.items():
                found = centerlines.centerlines_to_geojson(g["branches"], g["points"], pixel_size=b.pixel_size,
                                                           image_id=f"{b.bn}/{idx}", class_id=c)["features"]
                self.lines += _tagged(found, b, idx)
                self.rows += centerlines.csv_rows(b.model_info, b.bn, idx, c, g["table"], g["summary"])

    def write(self, stem: str) -> None:
        _feature_collection(self.graph_path or stem + "_crack_graph.geojson", self.lines)
        super().write(stem)
