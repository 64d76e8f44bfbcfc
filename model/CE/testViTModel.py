#!/usr/bin/env python3
"""Single-image inference, the MI355X counterpart of the reference's model/CE/testViTModel.py:92-126.

    python model/CE/testViTModel.py IMAGE [--model-id 0] [--num-classes 17] [--checkpoint x.ckpt]
                                          [--image-size 224] [--precision fp32|bf16] [--out mask.png]
                                          [--boxes boxes.json] [--tta d4] [--tta-sizes 160,224] [--tta-merge probs]
                                          [--min-area 8] [--fill-holes] [--max-hole-area 64]

Without --checkpoint the weights are random (the reference's checkpoints are private)."""
import argparse

import numpy as np

from classes import LightningViTModel  # noqa: F401  (same import the reference script uses)
from visiontransformer_amd import clean
from visiontransformer_amd.predict import load_model, predict
from visiontransformer_amd.tta import parse_sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("image")
    ap.add_argument("--model-id", type=int, default=0, help="configuration ID 0..8 of the reference grid")
    ap.add_argument("--num-classes", type=int, default=17)
    ap.add_argument("--checkpoint")
    ap.add_argument("--image-size", type=int, default=224)
    ap.add_argument("--precision", default="fp32")
    ap.add_argument("--out")
    ap.add_argument("--boxes", help="write the predicted regions' boxes, {class: [[y_min, x_min, y_max, x_max], ...]} for "
                                    "every class present but 0 (the reference's boxes panel), to this JSON file")
    ap.add_argument("--tta", help='test-time augmentation: "hflip", "flip" or "d4" -- the mask is merged from flipped / '
                                  "quarter-turned views (default: one look)")
    ap.add_argument("--tta-sizes", help="comma-separated sides the views are resampled to, e.g. 160,224 (default: the image size)")
    ap.add_argument("--tta-merge", default="logits", choices=["logits", "probs"], help="mean of the views' logits or of their sigmoids")
    clean.add_arguments(ap)
    a = ap.parse_args()
    tta = dict(tta=a.tta, tta_sizes=parse_sizes(a.tta_sizes), tta_merge=a.tta_merge, **clean.arguments(a))
    model = load_model(a.model_id, a.num_classes, a.checkpoint, image_size=a.image_size, precision=a.precision)
    if a.boxes:
        import json
        mask, boxes = predict(a.image, model, return_boxes=True, **tta)
        with open(a.boxes, "w") as f:
            json.dump({str(c): [list(b) for b in bs] for c, bs in boxes.items()}, f)
    else:
        mask = predict(a.image, model, **tta)
    print("classes present:", np.unique(mask).tolist(), "mask shape:", mask.shape)
    if a.out:
        from PIL import Image
        Image.fromarray((mask.astype(np.float32) * (255.0 / max(a.num_classes - 1, 1))).astype(np.uint8)).save(a.out)


if __name__ == "__main__":
    main()
