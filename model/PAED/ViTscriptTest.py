#!/usr/bin/env python3
"""PAED evaluation -- MI355X counterpart of the reference's model/PAED/ViTscriptTest.py:110-227: per configuration ID,
PAEDTrainer(P16, H512, L8, A8) (:126), latest checkpoint of logs/vit-model/version_<ID>, `num_batches` test batches:
model.eval(), logits.sigmoid(), argmax over the class dim (:184-193), per-image accuracy / IoU / Dice / class sets and
the time per image into test/<model>/<model>_metrics.csv.

    python model/PAED/ViTscriptTest.py --ids 0 --num-batches 3
"""
import argparse
import os

import torch

from classes import PAEDTrainer
from visiontransformer_amd import clean, scripts
from visiontransformer_amd.predict import CONFIGURATIONS
from visiontransformer_amd.tta import parse_sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, nargs="*", default=[0])
    ap.add_argument("--num-classes", type=int, default=1)       # ViTscript.py:27
    ap.add_argument("--patch-size", type=int, default=16)
    ap.add_argument("--hidden-size", type=int, default=512)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--heads", type=int, default=8)
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--batch-size", type=int, default=4)
    ap.add_argument("--num-batches", type=int, default=10)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--data")
    ap.add_argument("--out", default="test")
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
    scripts.add_confidence_arguments(ap)
    scripts.add_polygon_arguments(ap)
    scripts.add_crack_graph_arguments(ap)
    a = ap.parse_args()
    confidence = scripts.confidence_options(ap, a)
    dev = "cuda:0"
    cwd = os.getcwd()
    for vid in a.ids:
        P, D, L, A = CONFIGURATIONS.get(vid, (a.patch_size, a.hidden_size, a.layers, a.heads))
        print(f"Testing Version {vid}: Patch Size {P}, Hidden Size {D}, Hidden Layers {L}, Attention Heads {A}")
        # the reference builds the SAME architecture for every ID here (:126) and names the outputs after the grid entry
        model = PAEDTrainer(a.num_classes, a.patch_size, a.hidden_size, a.layers, a.heads, image_size=a.image_size,
                            precision=a.precision, device=dev)
        ck = scripts.get_latest_checkpoint(vid, cwd)
        if ck:
            model.load_state_dict(torch.load(ck, map_location="cpu")["state_dict"])
        name = f"ID{vid}P{P}H{D}A{A}"
        batches = scripts.paed_binary_batches(model.model.cfg, a.num_batches * a.batch_size, a.batch_size, a.data, seed=5)
        csv_path = os.path.join(cwd, a.out, name, f"{name}_metrics.csv")
        rows = scripts.evaluate_to_csv(model, batches, (vid, name, P, D, L, A), csv_path,
                                       max(a.num_classes, 2), a.num_batches, dev,
                                       distance_mode=a.distance_metrics, crack_classes=True if a.crack_metrics else None,
                                       tta=a.tta, tta_sizes=parse_sizes(a.tta_sizes), tta_merge=a.tta_merge,
                                       region_classes=True if a.region_metrics else None, region_iou=a.region_iou,
                                       region_coverage=a.region_coverage, region_connectivity=a.region_connectivity,
                                       props_classes=scripts.parse_props_classes(a.region_props),
                                       props_pixel_size=a.pixel_size, **clean.arguments(a), **confidence,
                                       **scripts.polygon_options(a, csv_path), **scripts.crack_graph_options(a, csv_path))
        print(f"{name}: {len(rows)} images evaluated -> {os.path.join(a.out, name)}")


if __name__ == "__main__":
    main()
