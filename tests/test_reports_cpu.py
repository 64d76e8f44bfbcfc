"""CPU: the flag table of the two evaluation scripts (scripts.add_evaluation_arguments / evaluation_options) and the argument
checks that regions, clean, polygons, centerlines and metrics share (_common): which values each caller takes and refuses."""
import argparse

import numpy as np
import pytest

from visiontransformer_amd import centerlines, clean, metrics, polygons, regions, scripts

CSV = "out/ID1/ID1_metrics.csv"


def _options(argv):
    ap = argparse.ArgumentParser()
    scripts.add_evaluation_arguments(ap)
    return scripts.evaluation_options(ap, ap.parse_args(argv), CSV)


def test_evaluation_options_without_a_flag_and_with_every_flag():
    assert _options([]) == dict(
        distance_mode=None, crack_classes=None, tta=None, tta_sizes=None, tta_merge="logits", region_classes=None,
        region_iou=0.5, region_coverage=0.5, region_connectivity=4, props_classes=None, props_pixel_size=1.0, min_area=0,
        fill_holes=False, max_hole_area=0, region_scores=False, score_kind="prob", score_low=0.5, calibration_bins=None)
    every = ["--distance-metrics", "borders", "--crack-metrics", "--region-metrics", "--region-iou", "0.6", "--region-coverage",
             "0.4", "--region-connectivity", "8", "--region-props", "2,1", "--pixel-size", "0.25", "--min-area", "8",
             "--fill-holes", "--max-hole-area", "64", "--region-polygons", "--crack-graph", "1,2"]
    shared = dict(
        distance_mode="borders", crack_classes=True, region_classes=True, region_iou=0.6, region_coverage=0.4,
        region_connectivity=8, props_classes=[2, 1], props_pixel_size=0.25, min_area=8, fill_holes=True, max_hole_area=64,
        polygons_path="out/ID1/ID1_region_polygons.geojson", crack_graph_classes=[1, 2],
        crack_graph_path="out/ID1/ID1_crack_graph.geojson", crack_branches_csv_path="out/ID1/ID1_crack_branches.csv")
    # the confidence flags and --tta exclude each other: every flag is set in one of the two command lines
    assert _options(every + ["--region-scores", "--score-kind", "margin", "--score-low", "0.7", "--calibration", "32"]) == dict(
        shared, tta=None, tta_sizes=None, tta_merge="logits", region_scores=True, score_kind="margin", score_low=0.7,
        calibration_bins=32)
    assert _options(every + ["--tta", "flip", "--tta-sizes", "160,224", "--tta-merge", "probs"]) == dict(
        shared, tta="flip", tta_sizes=(160, 224), tta_merge="probs", region_scores=False, score_kind="prob", score_low=0.5,
        calibration_bins=None)
    assert _options(["--distance-metrics", "--region-props", "--calibration", "--crack-graph"]) == dict(
        _options([]), distance_mode="sets", props_classes="all", calibration_bins=16, crack_graph_classes=True,
        crack_graph_path="out/ID1/ID1_crack_graph.geojson", crack_branches_csv_path="out/ID1/ID1_crack_branches.csv")
    for argv in (["--region-scores", "--tta", "hflip"], ["--calibration", "0"], ["--score-low", "1.5"], ["--min-area", "-1"],
                 ["--region-connectivity", "6"], ["--tta-merge", "max"]):
        with pytest.raises(SystemExit):
            _options(argv)


def _takes(call, good, bad):
    for v in good:
        call(v)
    for v in bad:
        with pytest.raises(ValueError):
            call(v)


def test_shared_argument_checks_take_and_refuse_what_each_caller_did():
    m = np.zeros((4, 4), np.uint8)
    ev = metrics.Evaluator(3, device="cpu")
    region_args = lambda **kw: ev._region_arguments(**{**dict(classes=None, iou_threshold=0.5, coverage=0.5, connectivity=4,
                                                              background=0, ignore_label=None), **kw})
    ints, no_ints = [0, 255, np.int64(3), np.uint8(7)], [True, False, 256, -2, 1.0, "0", None, np.float32(1)]
    # the background: -1 means "none" for the regions and the outlines; the clean-up and the matching need one
    _takes(lambda v: regions._checked(m, v, 4), ints + [-1, np.int32(-1)], no_ints)
    _takes(lambda v: clean.check_options(background=v), ints, no_ints + [-1])
    _takes(lambda v: region_args(background=v, classes=[9]), ints, no_ints + [-1])
    _takes(lambda v: region_args(ignore_label=v, classes=[9]), [None, 5, 255, np.uint8(7)], no_ints[:-3] + [0, -1, "0"])
    # connectivity
    for call in (lambda v: regions._checked(m, 0, v), lambda v: clean.check_options(connectivity=v),
                 lambda v: region_args(connectivity=v)):
        _takes(call, [4, 8, np.int64(8)], [6, 0, 1, "4", None])
    # the clean-up's counts
    for name in ("min_area", "max_hole_area"):
        _takes(lambda v: clean.check_options(**{name: v}), [0, 1, np.int64(3), (1 << 31) - 1], [-1, 1 << 31, True, 1.5, "3", None])
    # sequences of label values: distinct everywhere; the matching coerces with int(), the others take integers alone
    _takes(lambda v: regions._checked_props(m, v, 0, 4, "auto"), [None, "all", [], [1, 2], (3,), [np.int64(3), np.uint8(255)]],
           ["some", [True], [1.5], [256], [-1], [1, 1], [0], [0, 1]])
    with pytest.raises(ValueError):
        regions._checked_props(m, [2], 2, 4, "auto")          # the background among the classes
    assert regions._checked_props(m, [0, np.int64(1)], -1, 4, "auto")[2] == [0, 1]
    _takes(centerlines.check_options, [None, [0], [1, np.uint8(2)], (255,)], [[], "12", b"1", [True], [256], [-1], [1, 1], [1.0]])
    assert centerlines.check_options([np.int64(2), 1]) == [2, 1]
    _takes(lambda v: region_args(classes=v), [None, [1, 2], [1.0, 2], [True, 2], [np.int64(255)]], [[], [256], [-1], [1, 1], [0]])
    assert region_args(classes=[True, 2.0])[0] == [1, 2] and region_args(background=2, ignore_label=4)[0] == [0, 1]
    # pixel_size: positive and finite, whatever float() takes
    for call in (lambda v: regions.props_from_records(np.zeros((0, 20), np.int64), v),
                 lambda v: polygons.polygons_to_geojson(np.zeros((0, 7), np.int32), [], pixel_size=v),
                 lambda v: centerlines.branch_table(np.zeros((0, 9), np.int64), v),
                 lambda v: centerlines.summary(np.zeros((0, 4), np.int32), np.zeros((0, 9), np.int64), v)):
        _takes(call, [1, 0.5, np.float32(2), "2", True], [0, -1, float("nan"), float("inf"), float("-inf"), "x"])
