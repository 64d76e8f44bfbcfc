#!/usr/bin/env python3
"""Writes tests/golden/workspace/workspace.npz: vitseg_train_workspace and vitseg_query_workspace in bytes for every
precision over a grid of configurations x batches -- workspace sizes are behaviour, a caller allocates by them.

The grid is the 160 configurations of tests/test_config_domain_cpu.py (inside check_config's domain, most of them odd) and the
named production shapes, each at the batches 1, 2, 3, 4, 8, 16, 32, 64: 160 x 8 x 2 = 2 560 training queries from the first part
alone.  A refused query is stored as 0.  Host arithmetic: needs the built library, no GPU (256 compute units are assumed without
one, as on an MI355X).  tests/test_splitk_cpu.py asserts the table; rewrite it only when a size is meant to change."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from visiontransformer_amd import _lib  # noqa: E402
from visiontransformer_amd.config import ViTSegConfig, vit_base16, vit_large16, vit_tiny16  # noqa: E402

BATCHES = (1, 2, 3, 4, 8, 16, 32, 64)
PRECISIONS = (_lib.F32, _lib.BF16, _lib.F16, _lib.F32X3)
FIELDS = ("num_classes", "patch_size", "hidden_size", "num_hidden_layers", "num_attention_heads", "image_size",
          "intermediate_size", "num_channels")


def configs():
    from test_config_domain_cpu import CASES
    named = [vit_tiny16(), vit_tiny16(3), vit_base16(), vit_base16(17, 224), vit_base16(2, 224), vit_large16(),
             ViTSegConfig(17, 8, 768, 12, 12, image_size=224), ViTSegConfig(2, 8, 512, 8, 8, image_size=224),
             ViTSegConfig(2, 16, 1024, 2, 16, image_size=224), ViTSegConfig(2, 16, 512, 12, 8, image_size=320)]
    return [c for c, _ in CASES] + named


def size(fn, cfg, batch, precision):
    try:
        return fn(cfg, batch, precision)
    except (ValueError, RuntimeError):
        return 0


def table(cfg_rows):
    train = np.zeros((len(cfg_rows), len(BATCHES), len(PRECISIONS)), dtype=np.uint64)
    query = np.zeros_like(train)
    for i, row in enumerate(cfg_rows):
        cfg = ViTSegConfig(**{k: int(v) for k, v in zip(FIELDS, row)})
        for j, b in enumerate(BATCHES):
            for k, p in enumerate(PRECISIONS):
                train[i, j, k] = size(_lib.train_workspace, cfg, b, p)
                query[i, j, k] = size(_lib.query_workspace, cfg, b, p)
    return train, query


def main():
    rows = np.array([[getattr(c, f) for f in FIELDS] for c in configs()], dtype=np.int32)
    train, query = table(rows)
    path = os.path.join(ROOT, "tests", "golden", "workspace", "workspace.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, configs=rows, batches=np.array(BATCHES, dtype=np.int32),
                        precisions=np.array(PRECISIONS, dtype=np.int32), train=train, query=query)
    print(f"{len(rows)} configs x {len(BATCHES)} batches x {len(PRECISIONS)} precisions: "
          f"{int((train > 0).sum())} training sizes, {int((query > 0).sum())} inference sizes")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
