#!/usr/bin/env python3
"""Byte-for-byte A/B of the files `scripts.evaluate_to_csv` writes, between two versions of the Python evaluation layer (the
device results are integers or single-rounded values and the host arithmetic is deterministic, so the files are too).  Run it
once on each side as a process of its own and diff the outputs:
    python tools/eval_files_digest.py > a.txt        # on the old tree
    python tools/eval_files_digest.py > b.txt        # on the new tree
A tiny model (3 classes, P16, D192, 1 layer, 3 heads at 224) with synthetic weights of a fixed seed scores two batches of two
synthetic images under two option sets: (a) every output but test-time augmentation, at non-default settings; (b) test-time
augmentation at two sizes with the distance and region files.  Per set: the sorted directory listing and the SHA-256 of every
file; of <model>_metrics.csv without column 11, the time per image.  The mean of that column over set (a) goes to stderr: it
is the one figure that may differ between two runs."""
import csv
import hashlib
import io
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visiontransformer_amd import scripts, synth  # noqa: E402
from visiontransformer_amd.model import ViTSegmentationModel  # noqa: E402

DEV = "cuda:0"
INFO = (7, "ID7P16H192A3", 16, 192, 1, 3)
TIME_COLUMN = 11


def option_sets(out_dir):
    return {
        "a": dict(distance_mode="borders", crack_classes=True, region_classes=True, region_iou=0.6, region_connectivity=8,
                  props_classes=[1, 2], props_pixel_size=0.5, region_scores=True, score_kind="margin", score_low=0.6,
                  calibration_bins=8, polygons_path=os.path.join(out_dir, "a", "m_region_polygons.geojson"),
                  crack_graph_classes=[1, 2], min_area=4, fill_holes=True),
        "b": dict(tta="flip", tta_sizes=(160, 224), distance_mode="sets", region_classes=True),
    }


def file_digest(path):
    with open(path, "rb") as f:
        data = f.read()
    if os.path.basename(path) == "m_metrics.csv":   # the first file alone holds a time
        rows = list(csv.reader(io.StringIO(data.decode(), newline="")))
        buf = io.StringIO(newline="")
        csv.writer(buf).writerows([r[:TIME_COLUMN] + r[TIME_COLUMN + 1:] for r in rows])
        data = buf.getvalue().encode()
    return hashlib.sha256(data).hexdigest()


def main():
    model = ViTSegmentationModel(3, 16, 192, 1, 3, image_size=224, device=DEV).eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(model.cfg, seed=3).items()})
    batches = scripts.ce_batches(model.cfg, 4, 2, seed=3)
    with tempfile.TemporaryDirectory() as out_dir:
        for name, kw in option_sets(out_dir).items():
            rows = scripts.evaluate_to_csv(model, batches, INFO, os.path.join(out_dir, name, "m_metrics.csv"), 3, 2, DEV, **kw)
            names = sorted(os.listdir(os.path.join(out_dir, name)))
            print(f"set {name}: {len(rows)} images, files {' '.join(names)}")
            for n in names:
                print(f"  {file_digest(os.path.join(out_dir, name, n))}  {n}")
            if name == "a":
                mean = sum(r[TIME_COLUMN] for r in rows) / len(rows)
                print(f"set a: mean Inference_Time {mean * 1e3:.3f} ms per image", file=sys.stderr)


if __name__ == "__main__":
    main()
