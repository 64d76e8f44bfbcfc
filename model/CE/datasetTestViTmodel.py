#!/usr/bin/env python3
"""Dataset evaluation -- MI355X counterpart of the reference's model/CE/datasetTestViTmodel.py:107-227: for every
configuration ID, build LightningViTModel, load the latest checkpoint of logs/vit-model/version_<ID> (the reference
resumes the Lightning trainer on it; only the weights matter for the evaluation), run `num_batches` test batches and
write test/<model>/<model>_metrics.csv (per-image accuracy / mean IoU / mean Dice / class sets / time per image) --
the schema model/CE/compareModels.py:27-47 reads.  Plots are host-side reporting and not produced.

    python model/CE/datasetTestViTmodel.py --ids 1 --num-classes 17 --num-batches 3 [--data eval.pt]
"""
import argparse
import os

import torch

from classes import LightningViTModel
from visiontransformer_amd import clean, scripts
from visiontransformer_amd.predict import CONFIGURATIONS
from visiontransformer_amd.tta import parse_sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ids", type=int, nargs="*", default=sorted(CONFIGURATIONS))
    ap.add_argument("--num-classes", type=int, default=17)
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--batch-size", type=int, default=4)          # DataLoader(batch_size=4), :103
    ap.add_argument("--num-batches", type=int, default=10)        # :151
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
        P, D, L, A = CONFIGURATIONS[vid]
        print(f"Testing Version {vid}: Patch Size {P}, Hidden Size {D}, Hidden Layers {L}, Attention Heads {A}")
        model = LightningViTModel(a.num_classes, P, D, L, A, image_size=a.image_size, precision=a.precision, device=dev)
        ck = scripts.get_latest_checkpoint(vid, cwd)
        if ck:
            model.load_state_dict(torch.load(ck, map_location="cpu")["state_dict"])
        name = f"ID{vid}P{P}H{D}A{A}"
        batches = scripts.ce_batches(model.model.cfg, a.num_batches * a.batch_size, a.batch_size, a.data, seed=3)
        csv_path = os.path.join(cwd, a.out, name, f"{name}_metrics.csv")
        rows = scripts.evaluate_to_csv(model, batches, (vid, name, P, D, L, A), csv_path,
                                       a.num_classes, a.num_batches, dev,
                                       distance_mode=a.distance_metrics, crack_classes=True if a.crack_metrics else None,
                                       tta=a.tta, tta_sizes=parse_sizes(a.tta_sizes), tta_merge=a.tta_merge,
                                       region_classes=True if a.region_metrics else None, region_iou=a.region_iou,
                                       region_coverage=a.region_coverage, region_connectivity=a.region_connectivity,
                                       props_classes=scripts.parse_props_classes(a.region_props),
                                       props_pixel_size=a.pixel_size, **clean.arguments(a), **confidence,
                                       **scripts.polygon_options(a, csv_path), **scripts.crack_graph_options(a, csv_path))
        acc = sum(r[8] for r in rows) / max(len(rows), 1)
        print(f"{name}: {len(rows)} images, mean accuracy {acc:.2f} %, {rows[0][11] * 1e3:.2f} ms/image")


if __name__ == "__main__":
    main()
