"""Generates tests/golden/posinterp/*.npz: the REAL reference ViTSegmentationModel with its backbone called with
`interpolate_pos_encoding=True` (Hugging Face ViTEmbeddings.interpolate_pos_encoding), i.e. a model whose position table
has the 224x224 geometry (197 rows at P = 16) run on inputs of another size.

Same fixture kinds as oracle/make_golden.py (whose loader, sampler and stage hooks it imports): sampled stages, the full
low-res logits, sampled logits, the mask bits (+ fragile pixels), and for the training case the loss, sampled gradients
-- backbone.embeddings.position_embeddings among them, at its [1, 197, D] shape -- and the first Adam step.  Needs the
reference tree and `transformers`; nothing here runs on the product path.

    python tools/make_golden_posinterp.py       # rewrites tests/golden/posinterp/*.npz
"""
from __future__ import annotations

import dataclasses
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden import GRAD_KEYS, STAGES, hook_stages, load_reference_class, pack  # noqa: E402
from visiontransformer_amd import synth  # noqa: E402
from visiontransformer_amd.config import ViTSegConfig  # noqa: E402

OUT_DIR = os.path.join(ROOT, "tests", "golden", "posinterp")

# name -> (cfg = the checkpoint's geometry, input side, batch, weight seed, with_training)
CASES = {
    "tiny16_224to384_c2": (ViTSegConfig(2, 16, 192, 12, 3, image_size=224), 384, 2, 1, False),
    "tiny16_224to160_c2": (ViTSegConfig(2, 16, 192, 12, 3, image_size=224), 160, 1, 1, False),   # downsampling
    "base16_224to512_c2": (ViTSegConfig(2, 16, 768, 12, 12, image_size=224), 512, 1, 3, False),  # the headline size
    "p8_h512_224to320_c2": (ViTSegConfig(2, 8, 512, 2, 8, image_size=224), 320, 1, 4, False),    # grid 28 -> 40
    "base16w_l2_224to320_c2_train": (ViTSegConfig(2, 16, 768, 2, 12, image_size=224), 320, 2, 6, True),
}


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    os.makedirs(OUT_DIR, exist_ok=True)
    build = load_reference_class()
    import transformers
    for name, (cfg, S_in, B, wseed, train) in CASES.items():
        ref = build(cfg).eval()   # eval(): dropout off
        bb_forward = ref.backbone.forward
        ref.backbone.forward = lambda *a, **kw: bb_forward(*a, interpolate_pos_encoding=True, **kw)
        sd_np = synth.make_state_dict(cfg, seed=wseed)
        missing, unexpected = ref.load_state_dict({k: torch.from_numpy(v) for k, v in sd_np.items()}, strict=False)
        assert not unexpected, unexpected
        assert all(k.startswith("backbone.pooler.") for k in missing), missing
        cfg_in = dataclasses.replace(cfg, image_size=S_in)
        x = torch.from_numpy(synth.make_images(cfg_in, B, seed=0))
        stages = {}
        hooks = hook_stages(ref, stages)
        store = {"meta.versions": np.array([torch.__version__, transformers.__version__]),
                 "meta.cfg": np.array([cfg.num_classes, cfg.patch_size, cfg.hidden_size, cfg.num_hidden_layers,
                                       cfg.num_attention_heads, cfg.image_size, cfg.intermediate_size, B, wseed]),
                 "meta.head_gain": np.array([1.0]), "meta.image_in": np.array([S_in])}
        if train:
            y256 = torch.from_numpy(synth.make_targets(cfg, B, seed=0))
            # the targets resized to the input's size (LightningViTModel._resize_target, classes.py:273-285)
            y = F.interpolate(y256.unsqueeze(1).float(), size=(S_in, S_in), mode="nearest").squeeze(1).long()
            logits = ref(x)
            loss = nn.CrossEntropyLoss()(logits, y)
            loss.backward()
            store["train.target_resized"] = y.numpy().astype(np.uint8)
            store["train.loss"] = np.array([loss.item()], dtype=np.float64)
            named = dict(ref.named_parameters())
            for gk in GRAD_KEYS:
                gk = gk.format(last=cfg.num_hidden_layers - 1)
                pack(store, "grad." + gk, named[gk].grad)
            opt = torch.optim.Adam(ref.parameters(), lr=1e-5)   # configure_optimizers(), classes.py:296-297
            opt.step()
            for gk in GRAD_KEYS[:6] + ["backbone.embeddings.position_embeddings"]:
                gk = gk.format(last=cfg.num_hidden_layers - 1)
                pack(store, "adam1." + gk, named[gk].detach() - torch.from_numpy(sd_np[gk]).reshape(named[gk].shape))
        else:
            with torch.no_grad():
                logits = ref(x)
        for h in hooks:
            h.remove()
        for st in STAGES:
            pack(store, "stage." + st, stages[st])
        store["lowres_logits.full"] = stages["lowres_logits"].detach().numpy()
        pack(store, "logits", logits)
        with torch.no_grad():
            mask = logits.detach().sigmoid().argmax(dim=1).numpy().astype(np.uint8)   # testViTModel.py:122-126
            srt = logits.detach().sigmoid().sort(dim=1, descending=True).values
            margin_sig = (srt[:, 0] - srt[:, 1]).numpy()
            srt = logits.detach().sort(dim=1, descending=True).values
            margin = (srt[:, 0] - srt[:, 1]).numpy()
        store["mask.bits"] = np.packbits(mask.ravel())
        fragile = (margin < 1e-4) | (margin_sig == 0)
        store["mask.fragile_bits"] = np.packbits(fragile.ravel())
        store["mask.shape"] = np.array(mask.shape)
        path = os.path.join(OUT_DIR, name + ".npz")
        np.savez_compressed(path, **store)
        print(f"{name}: logits[{tuple(logits.shape)}] min-margin {margin.min():.3e} fragile {int(fragile.sum())} "
              f"size {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
