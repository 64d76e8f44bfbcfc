"""GPU (-m gpu): the dataset evaluation's reports (scripts.evaluate_to_csv over reports.*) on a tiny model, two batches of two
224 x 224 images: every file is the same whether its report runs alone or beside all the others, the region-metrics file holds
Evaluator.region_metrics' rows and the pooled ones, test-time augmentation reaches every file, and the Evaluator's methods
resize a smaller ground truth exactly as `resized_gt` does.  Everything compared is an integer or host arithmetic on integers:
the comparisons are exact."""
import csv
import os

import numpy as np
import pytest
import torch

from visiontransformer_amd import clean, metrics, scripts, synth
from visiontransformer_amd.model import ViTSegmentationModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INFO = (7, "ID7P16H192A3", 16, 192, 1, 3)
SHARED = dict(min_area=4, fill_holes=True, region_connectivity=8, props_pixel_size=0.5)   # what every report sees
_CACHE = {}


def _setup():
    """(model, batches, per batch (cleaned mask, ground truth [n, H, W])), built once"""
    if not _CACHE:
        model = ViTSegmentationModel(3, 16, 192, 1, 3, image_size=224, device=DEV).eval()
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(model.cfg, seed=3).items()})
        batches = scripts.ce_batches(model.cfg, 4, 2, seed=3)
        seen = []
        for x, gt in batches:
            with torch.no_grad():
                mask = clean.clean_mask(model.predict_mask(x.to(DEV)), min_area=4, fill_holes=True)
            seen.append((mask, gt.reshape(gt.shape[0], gt.shape[-2], gt.shape[-1])))
        _CACHE.update(model=model, batches=batches, seen=seen)
    return _CACHE["model"], _CACHE["batches"], _CACHE["seen"]


def _run(directory, **kw):
    model, batches, _ = _setup()
    return scripts.evaluate_to_csv(model, batches, INFO, str(directory / "m_metrics.csv"), 3, 2, DEV, **kw)


def _content(path):
    """The file's bytes; of the metrics file its rows without column 11, the time per image"""
    if os.path.basename(path) == "m_metrics.csv":
        return [r[:11] + r[12:] for r in csv.reader(open(path, newline=""))]
    with open(path, "rb") as f:
        return f.read()


def _text(rows):
    return [[str(v) for v in r] for r in rows]


def test_every_file_is_the_same_alone_and_beside_the_others(tmp_path):
    scores = dict(region_scores=True, score_kind="margin", score_low=0.6)
    region = dict(region_classes=True, region_iou=0.6)
    alone = {
        "distance": dict(distance_mode="borders"),
        "crack": dict(crack_classes=True),
        "region": region,
        "scores": dict(**scores, **region),       # the matched flags and the AP rows come from the region metrics
        "calibration": dict(calibration_bins=8, score_kind="margin"),
        "props": dict(props_classes=[1, 2]),
        "outlines": dict(polygons_path=str(tmp_path / "outlines" / "m_region_polygons.geojson")),
        "graph": dict(crack_graph_classes=[1, 2]),
    }
    combined = {k: v for kw in alone.values() for k, v in kw.items()}
    combined["polygons_path"] = str(tmp_path / "all" / "m_region_polygons.geojson")
    _run(tmp_path / "all", **combined, **SHARED)
    names = sorted(os.listdir(tmp_path / "all"))
    assert names == ["m_calibration.csv", "m_crack_branches.csv", "m_crack_graph.geojson", "m_crack_metrics.csv",
                     "m_distance_metrics.csv", "m_metrics.csv", "m_region_metrics.csv", "m_region_polygons.geojson",
                     "m_region_props.csv", "m_region_scores.csv"]
    written = set()
    for name, kw in alone.items():
        _run(tmp_path / name, **kw, **SHARED)
        found = sorted(os.listdir(tmp_path / name))
        assert "m_metrics.csv" in found and 2 <= len(found) <= 3, (name, found)
        for f in found:
            assert _content(tmp_path / name / f) == _content(tmp_path / "all" / f), (name, f)
        written.update(found)
    assert sorted(written) == names
    assert len(_content(tmp_path / "all" / "m_metrics.csv")) == 1 + 4
    assert os.path.getsize(tmp_path / "all" / "m_region_scores.csv") > 200   # regions were found: the files are not headers alone


def test_region_metrics_file_holds_the_rows_per_image_and_the_pooled_rows(tmp_path):
    _, _, seen = _setup()
    _run(tmp_path, region_classes=True, region_iou=0.6, region_coverage=0.4, **SHARED)
    got = list(csv.reader(open(tmp_path / "m_region_metrics.csv", newline="")))
    assert got[0] == metrics.REGION_CSV_COLUMNS
    ev = metrics.Evaluator(3, DEV)
    want, stats = [], []
    for bn, (mask, gt) in enumerate(seen):
        for idx, m in enumerate(ev.region_metrics(mask, gt, classes=[1, 2], iou_threshold=0.6, coverage=0.4, connectivity=8)):
            stats.append(m["stats"])
            want += [metrics.region_csv_row(INFO, bn, idx, c, 0.6, 0.4, r) for c, r in m["per_class"].items()]
    assert len(want) == 2 * 2 * 2 and sum(int(s[:, 1].sum()) for s in stats) > 0      # some predicted regions at all
    pooled = metrics.matches_from_stats(metrics.pool_region_stats(stats))
    want += [metrics.region_csv_row(INFO, "pooled", "", c, 0.6, 0.4, r) for c, r in zip((1, 2), pooled)]
    assert got[1:] == _text(want)


def test_tta_reaches_the_metrics_and_the_distance_file(tmp_path):
    model, batches, _ = _setup()
    rows = _run(tmp_path, tta="hflip", distance_mode="sets")
    assert sorted(os.listdir(tmp_path)) == ["m_distance_metrics.csv", "m_metrics.csv"]
    ev = metrics.Evaluator(3, DEV)
    want, dwant, differ = [], [], 0
    for bn, (x, gt) in enumerate(batches):
        gt = gt.reshape(gt.shape[0], gt.shape[-2], gt.shape[-1])
        with torch.no_grad():
            mask = model.predict_mask_tta(x.to(DEV), tta="hflip")
            differ += int((mask != model.predict_mask(x.to(DEV))).sum())
        want += [metrics.csv_row(INFO, bn, idx, m, 0.0) for idx, m in enumerate(ev.evaluate(mask, gt))]
        dwant += [metrics.distance_csv_row(INFO, bn, idx, "sets", 95, m)
                  for idx, m in enumerate(ev.distance_metrics(mask, gt, mode="sets", percentile=95))]
    assert differ > 0                                   # the merged mask is not the plain one: the comparison can tell them apart
    strip = lambda rs: [list(r[:11]) + list(r[12:]) for r in rs]
    np.testing.assert_equal(strip(rows), strip(want))   # nan-aware: a class mean may be nan
    assert _content(tmp_path / "m_metrics.csv")[1:] == _text(strip(want))
    got = list(csv.reader(open(tmp_path / "m_distance_metrics.csv", newline="")))
    assert got[0] == metrics.DISTANCE_CSV_COLUMNS and got[1:] == _text(dwant)


def test_evaluator_resizes_a_smaller_ground_truth_as_resized_gt_does():
    model, _, seen = _setup()
    pred = seen[0][0]
    small = torch.from_numpy(synth.make_targets(model.cfg, 2, seed=11, size=112))
    assert tuple(pred.shape) == (2, 224, 224) and tuple(small.shape) == (2, 112, 112) and len(torch.unique(small)) == 3
    ev = metrics.Evaluator(3, DEV)
    g = ev.resized_gt(small, pred)
    idx = torch.arange(224) // 2                        # Pillow's NEAREST at a factor of two: floor((i + 0.5) / 2)
    assert g.dtype == torch.uint8 and torch.equal(g.cpu(), small[:, idx][:, :, idx].to(torch.uint8))
    assert ev.resized_gt(g, pred) is g                  # the sizes agree: the tensor itself
    for a, b in zip(ev.distance_stats(pred, small, [0, 1, 2], 1, 19, 20), ev.distance_stats(pred, g, [0, 1, 2], 1, 19, 20)):
        assert a.dtype == b.dtype and torch.equal(a, b)
    for a, b in zip(ev.skeleton_stats(pred, small, [1, 2]), ev.skeleton_stats(pred, g, [1, 2])):
        assert a.dtype == b.dtype and torch.equal(a, b)
    a = ev.region_match_stats(pred, small, [1, 2], (3, 5), (1, 2), 8, return_info=True)
    b = ev.region_match_stats(pred, g, [1, 2], (3, 5), (1, 2), 8, return_info=True)
    assert all(torch.equal(s, t) for s, t in zip(a, b)) and int(a[0][:, :, 0].sum()) > 0      # some true regions at all
    pa = ev.region_props(pred, small, skeleton_classes=[1, 2], connectivity=8, pixel_size=0.5)
    pb = ev.region_props(pred, g, skeleton_classes=[1, 2], connectivity=8, pixel_size=0.5)
    np.testing.assert_equal(pa, pb)
    assert all(len(d["gt"]) > 0 for d in pa)
