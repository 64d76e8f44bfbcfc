"""Shared helpers for the parity tests (golden loading, oracle wiring)."""
import os

import numpy as np
import torch

from visiontransformer_amd import synth
from visiontransformer_amd.config import ViTSegConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz"))

# bf16 training-step gradient gates for shallow models (<= 2 layers): per-tensor relative L2 error / cosine against the fp32
# or fp64 gradient of the same step; bf16 operands (2^-9) through 1-2 layers give <= 5.1e-2 / 0.9987
BF16_GRAD_REL, BF16_GRAD_COS = 0.10, 0.997


class Golden:
    def __init__(self, name):
        self.name = name
        self.z = np.load(os.path.join(GOLDEN, name + ".npz"))
        m = [int(v) for v in self.z["meta.cfg"]]
        self.cfg = ViTSegConfig(m[0], m[1], m[2], m[3], m[4], image_size=m[5], intermediate_size=m[6])
        self.batch, self.wseed = m[7], m[8]
        self.head_gain = float(self.z["meta.head_gain"][0])

    def state_dict_np(self):
        return synth.make_state_dict(self.cfg, seed=self.wseed, head_gain=self.head_gain)

    def state_dict(self, dtype=torch.float32):
        return {k: torch.from_numpy(v).to(dtype) for k, v in self.state_dict_np().items()}

    def images(self):
        return torch.from_numpy(synth.make_images(self.cfg, self.batch, seed=0))

    def targets(self):
        return torch.from_numpy(synth.make_targets(self.cfg, self.batch, seed=0))

    def has(self, key):
        return key + ".idx" in self.z.files

    def sampled(self, key):
        return self.z[key + ".idx"], self.z[key + ".val"], tuple(self.z[key + ".shape"])

    def max_abs_err(self, key, tensor):
        """max |tensor.flat[idx] - golden| and the golden's max-abs (for relative scale)."""
        idx, val, shape = self.sampled(key)
        assert tuple(tensor.shape) == shape, (key, tuple(tensor.shape), shape)
        a = tensor.detach().to(torch.float64).cpu().numpy().ravel()[idx]
        return float(np.abs(a - val.astype(np.float64)).max()), float(np.abs(val).max())

    def checksum_rel_err(self, key, tensor):
        a = tensor.detach().to(torch.float64).cpu().numpy().ravel()
        s = self.z[key + ".sum"]
        return abs(a.sum() - s[0]) / (np.sqrt(s[1] * a.size) + 1e-30)

    def mask(self):
        shape = tuple(self.z["mask.shape"])
        if "mask.bits" in self.z.files:
            n = int(np.prod(shape))
            return np.unpackbits(self.z["mask.bits"])[:n].reshape(shape)
        return self.z["mask.u8"]

    def fragile(self):
        shape = tuple(self.z["mask.shape"])
        n = int(np.prod(shape))
        return np.unpackbits(self.z["mask.fragile_bits"])[:n].reshape(shape).astype(bool)


def relu_flip_tokens(stages, cfg, thr=2e-6, limit=16):
    """Reference-layout token indices (CLS = 0) whose gradient one sign flip of a seg_head.0 ReLU can move: the head
    applies ReLU to ~10^6 pre-activations; one that lies within fp32 rounding of zero in the fp64 oracle may take the other
    branch on the GPU, which changes the gradient that flows into the 3x3 token neighbourhood of that unit.  Returns the
    union of those neighbourhoods (a handful of units at most -- asserted)."""
    z = stages["head_pre"].detach()
    near = (z.abs() < thr).nonzero()
    assert near.shape[0] <= limit, f"{near.shape[0]} head pre-activations within {thr} of zero"
    g = cfg.grid
    toks = set()
    for _, _, y, x in near.tolist():
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if 0 <= y + dy < g and 0 <= x + dx < g:
                    toks.add(1 + (y + dy) * g + (x + dx))
    return sorted(toks), int(near.shape[0])


def grad_check(cfg, arena_grad, leaf, precision, stages=None):
    from visiontransformer_amd.params import arena_views
    gv = arena_views(cfg, arena_grad)
    rel_gate, cos_gate = BF16_GRAD_REL, BF16_GRAD_COS
    worst, worst_cos, bad, worst_name = 0.0, 1.0, [], ""
    num, den = 0.0, 0.0
    exempt_rows, n_near = relu_flip_tokens(stages, cfg) if stages is not None else ([], 0)
    for k, r in leaf.items():
        if r.grad is None or "pooler" in k:
            continue
        A, Bg = gv[k].cpu().double(), r.grad.double()
        if precision == "fp32" and exempt_rows and k.endswith("position_embeddings"):
            # the only tensor indexed by token: leave out exactly the token rows next to a ReLU unit whose fp64
            # pre-activation is within fp32 rounding of zero (see relu_flip_tokens); everything else is compared
            keep = torch.ones(A.shape[1], dtype=torch.bool)
            keep[exempt_rows] = False
            A, Bg = A[:, keep], Bg[:, keep]
        a, b = A.flatten(), Bg.flatten()
        if b.norm() < 1e-7:
            if a.norm() >= 1e-4:
                bad.append((k, "zero-gradient tensor", float(a.norm())))
            continue
        rel = float((a - b).norm() / b.norm())
        num, den = num + float((a - b).pow(2).sum()), den + float(b.pow(2).sum())
        if rel > worst:
            worst, worst_name = rel, k
        if precision == "fp32":
            if rel >= 2e-4:
                bad.append((k, rel, float((a - b).abs().max() / b.abs().max())))
        else:       # bf16 operands (2^-9 relative) through the layer
            cos = float((a @ b) / (a.norm() * b.norm()))
            worst_cos = min(worst_cos, cos)
            if not (cos > cos_gate and rel < rel_gate):
                bad.append((k, rel, cos))
    whole = (num / max(den, 1e-300)) ** 0.5
    print(f"gradient check ({precision}): worst relative L2 {worst:.3e} ({worst_name}), worst cosine {worst_cos:.5f}, "
          f"whole gradient {whole:.3e}, "
          f"{n_near} head units within fp32 rounding of zero ({len(exempt_rows)} position-embedding rows set aside)")
    assert not bad, bad
    return worst, whole
