"""Fused Adam / AdamW over the flat parameter arena (one kernel launch per step), and what fine-tuning adds to them.

`FusedAdam(params, lr)` is `torch.optim.Adam(params, lr)` with default betas/eps, weight_decay 0, amsgrad off --
what `LightningViTModel.configure_optimizers` builds in the reference (model/CE/classes.py:296-297).  It refuses a
nonzero weight_decay: torch.optim.Adam adds L2 decay to the gradient (g += wd * p), which the kernel does not do.
`FusedAdamW` is `torch.optim.AdamW` (decoupled decay: p *= 1 - lr * wd in front of the update).

The arena is one tensor, so torch's parameter groups cannot describe it.  `arena_groups` describes it instead: every arena
tensor starts on a 64-float boundary, so a byte per 64-float chunk names the group of (lr_mult, wd_mult) its floats belong to
-- layer-wise learning-rate decay, no decay on biases / LayerNorm / cls / pos, frozen embeddings or backbone.  With `groups=`,
`max_grad_norm=`, `skip_nonfinite=` or `ema_decay=` the optimisers step through the entry points of include/vitseg_optim.h
(csrc/optim.hip): the squared-gradient partial sums (only when the step clips or may skip), one block that forms the norm,
the clip coefficient, the skip decision and the per-group step sizes on the device, and one pass over the arena with the
arithmetic of the plain kernel element for element, the EMA of the weights in the same pass.  Nothing in a step reads device
memory from the host.  Without the four arguments `step()` calls exactly what it called before.
"""
from __future__ import annotations

import contextlib
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib

CHUNK = 64          # include/vitseg_optim.h VITSEG_OPTIM_CHUNK: floats per chunk (csrc/plan.hpp ALIGN_F)
PARTIAL = 8192      # VITSEG_OPTIM_PARTIAL: floats per fp32 partial sum of the norm
MAX_GROUPS = 256    # VITSEG_OPTIM_MAX_GROUPS
STATE_WORDS = 8     # VITSEG_OPTIM_STATE_BYTES / 4
FLAG_NORM, FLAG_CLIP, FLAG_SKIP = 1, 2, 4   # VITSEG_OPTIM_NORM / _CLIP / _SKIP
# words of the device state (the float words are read through .view(torch.float32))
W_STEP, W_SKIPPED, W_NORM, W_COEF, W_BC1, W_RBC2, W_APPLIED = range(7)
NO_DECAY_KINDS = ("bias", "norm", "cls", "pos")

Row = namedtuple("Row", "name tensor layer offset numel lr_mult wd_mult group")   # numel: padded to whole chunks

# arena order (csrc/plan.hpp make_layout): (tensor id, name, kinds)
_PRE = [(_lib.T_CLS, "backbone.embeddings.cls_token", ("cls",)),
        (_lib.T_POS, "backbone.embeddings.position_embeddings", ("pos",)),
        (_lib.T_PATCH_W, "backbone.embeddings.patch_embeddings.projection.weight", ()),
        (_lib.T_PATCH_B, "backbone.embeddings.patch_embeddings.projection.bias", ("bias",))]
_LAYER = [(_lib.T_LN1_W, "layernorm_before.weight", ("norm",)), (_lib.T_LN1_B, "layernorm_before.bias", ("norm", "bias")),
          (_lib.T_WQKV, "attention.qkv.weight", ()), (_lib.T_BQKV, "attention.qkv.bias", ("bias",)),
          (_lib.T_WO, "attention.o_proj.weight", ()), (_lib.T_BO, "attention.o_proj.bias", ("bias",)),
          (_lib.T_LN2_W, "layernorm_after.weight", ("norm",)), (_lib.T_LN2_B, "layernorm_after.bias", ("norm", "bias")),
          (_lib.T_W1, "mlp.fc1.weight", ()), (_lib.T_B1, "mlp.fc1.bias", ("bias",)),
          (_lib.T_W2, "mlp.fc2.weight", ()), (_lib.T_B2, "mlp.fc2.bias", ("bias",))]
_POST = [(_lib.T_LNF_W, "backbone.layernorm.weight", ("norm",)), (_lib.T_LNF_B, "backbone.layernorm.bias", ("norm", "bias")),
         (_lib.T_HEAD0_W, "seg_head.0.weight", ()), (_lib.T_HEAD0_B, "seg_head.0.bias", ("bias",)),
         (_lib.T_HEAD2_W, "seg_head.2.weight", ()), (_lib.T_HEAD2_B, "seg_head.2.bias", ("bias",))]


def _symbol(name: str):
    from . import _ext
    return _ext.ext_symbol("optim", name)


class ArenaGroups:
    """The parameter groups of an arena: `rows` (one `Row` per arena tensor, in arena order), `table` (float32 [G, 2]: lr_mult,
    wd_mult of every group; lr_mult 0 is a frozen group), `chunk_map` (uint8 [n_floats / 64]: the group of every chunk) and
    `n_floats`.  Built by `arena_groups`, or directly from a table and a chunk map."""

    def __init__(self, table, chunk_map, rows=()):
        self.table = np.ascontiguousarray(np.asarray(table, dtype=np.float32).reshape(-1, 2))
        self.chunk_map = np.ascontiguousarray(np.asarray(chunk_map, dtype=np.uint8).reshape(-1))
        self.rows = list(rows)
        if not 1 <= len(self.table) <= MAX_GROUPS:
            raise ValueError(f"an arena takes 1..{MAX_GROUPS} parameter groups, got {len(self.table)}")
        if not np.all(np.isfinite(self.table)) or np.any(self.table < 0):
            raise ValueError("lr_mult and wd_mult must be finite and >= 0")
        if len(self.chunk_map) == 0 or int(self.chunk_map.max()) >= len(self.table):
            raise ValueError(f"the chunk map must be non-empty and name groups below {len(self.table)}")

    @property
    def n_floats(self) -> int:
        return CHUNK * len(self.chunk_map)

    @property
    def frozen(self) -> np.ndarray:
        """bool [n_chunks]: the chunks no step touches."""
        return self.table[self.chunk_map, 0] == 0

    def describe(self) -> str:
        """One line per group: its multipliers, floats and tensors (runs of layers abbreviated by their count)."""
        lines = [f"{len(self.table)} groups over {self.n_floats} floats ({len(self.chunk_map)} chunks of {CHUNK})"]
        counts = np.bincount(self.chunk_map, minlength=len(self.table)) * CHUNK
        for gi, (lm, wm) in enumerate(self.table):
            names = [r.name for r in self.rows if r.group == gi]
            shown = ", ".join(names[:3]) + (f", ... ({len(names)} tensors)" if len(names) > 3 else "")
            lines.append(f"  group {gi}: lr x {lm:.6g}{' (frozen)' if lm == 0 else ''}, weight decay x {wm:.6g}, {int(counts[gi])} floats"
                         + (f": {shown}" if names else ""))
        return "\n".join(lines)


def _freeze_depth(freeze, layers: int):
    """(deepest frozen depth id or -1, whether everything but seg_head is frozen)."""
    if freeze is None or (isinstance(freeze, (tuple, list)) and not freeze):
        return -1, False
    if freeze == "embeddings":
        return 0, False
    if freeze == "backbone":
        return layers, True
    if isinstance(freeze, (int, np.integer)) and not isinstance(freeze, (bool, np.bool_)) and 0 <= freeze <= layers:
        return int(freeze), False
    raise ValueError(f'freeze must be "embeddings", "backbone" or a number of layers 0..{layers}, got {freeze!r}')


def arena_groups(cfg, layer_decay: float = 1.0, no_decay=(), freeze=(), head_lr_mult: float = 1.0) -> ArenaGroups:
    """The groups of the arena of configuration `cfg`; host arithmetic on `_lib.param_offset` alone.
    Depth ids as BEiT / timm number them: cls, pos and the patch projection 0, layer i i + 1, the final LayerNorm and seg_head
    L + 1; lr_mult = layer_decay ** (L + 1 - depth), times `head_lr_mult` for seg_head.
    `no_decay`: a subset of {"bias", "norm", "cls", "pos"} (a name or a sequence), or "default" for all four: wd_mult 0 there.
    `freeze`: "embeddings", "backbone" (everything but seg_head) or an int k (embeddings and the first k layers): lr_mult 0.
    ValueError for an unknown name, layer_decay outside (0, 1], a negative head_lr_mult or more than 256 distinct groups."""
    if not (isinstance(layer_decay, (int, float)) and 0.0 < float(layer_decay) <= 1.0):
        raise ValueError(f"layer_decay must lie in (0, 1], got {layer_decay!r}")
    if not (isinstance(head_lr_mult, (int, float)) and math.isfinite(head_lr_mult) and head_lr_mult >= 0):
        raise ValueError(f"head_lr_mult must be finite and >= 0, got {head_lr_mult!r}")
    kinds = NO_DECAY_KINDS if no_decay == "default" else (no_decay,) if isinstance(no_decay, str) else tuple(no_decay or ())
    unknown = [k for k in kinds if k not in NO_DECAY_KINDS]
    if unknown:
        raise ValueError(f'no_decay takes "default" or names among {NO_DECAY_KINDS}, got {unknown[0]!r}')
    L = cfg.num_hidden_layers
    frozen_to, backbone = _freeze_depth(freeze, L)
    tensors = [(tid, name, k, 0, 0) for tid, name, k in _PRE]
    for i in range(L):
        tensors += [(tid, f"backbone.layers.{i}.{name}", k, i, i + 1) for tid, name, k in _LAYER]
    tensors += [(tid, name, k, 0, L + 1) for tid, name, k in _POST]
    total = _lib.param_count(cfg)
    offsets = [_lib.param_offset(cfg, tid, layer)[0] for tid, _, _, layer, _ in tensors] + [total]
    if sorted(offsets) != offsets or offsets[0] != 0 or any(o % CHUNK for o in offsets):
        raise RuntimeError("the arena is not laid out in forward order on 64-float boundaries")
    pairs, rows = {}, []
    chunk_map = np.empty(total // CHUNK, dtype=np.uint8)
    for (tid, name, k, layer, depth), off, end in zip(tensors, offsets[:-1], offsets[1:]):
        head = name.startswith("seg_head.")
        lr_mult = float(layer_decay) ** (L + 1 - depth) * (float(head_lr_mult) if head else 1.0)
        if depth <= frozen_to or (backbone and not head):
            lr_mult = 0.0
        wd_mult = 0.0 if any(kind in kinds for kind in k) else 1.0
        pair = (float(np.float32(lr_mult)), float(np.float32(wd_mult)))
        group = pairs.setdefault(pair, len(pairs))
        if group >= MAX_GROUPS:
            raise ValueError(f"more than {MAX_GROUPS} distinct (lr_mult, wd_mult) groups")
        chunk_map[off // CHUNK:end // CHUNK] = group
        rows.append(Row(name, tid, layer, off, end - off, pair[0], pair[1], group))
    return ArenaGroups(np.array(list(pairs), dtype=np.float32), chunk_map, rows)


def warmup_cosine(opt, warmup_steps: int, total_steps: int, min_lr_ratio: float = 0.0):
    """A `LambdaLR` to step once per optimiser step: the factor rises linearly from 0 to 1 over `warmup_steps` steps and falls
    along half a cosine to `min_lr_ratio` at `total_steps` (where it stays)."""
    warmup_steps, total_steps = int(warmup_steps), int(total_steps)
    if warmup_steps < 0 or total_steps < max(warmup_steps, 1) or not 0.0 <= min_lr_ratio <= 1.0:
        raise ValueError(f"warmup_cosine needs 0 <= warmup_steps <= total_steps, total_steps >= 1 and min_lr_ratio in 0..1, got "
                         f"{warmup_steps}, {total_steps}, {min_lr_ratio}")

    def factor(step):
        if step < warmup_steps:
            return step / warmup_steps
        t = min(1.0, (step - warmup_steps) / max(1, total_steps - warmup_steps))
        return min_lr_ratio + (1.0 - min_lr_ratio) * 0.5 * (1.0 + math.cos(math.pi * t))
    return torch.optim.lr_scheduler.LambdaLR(opt, factor)


class FusedAdam(torch.optim.Optimizer):
    _decoupled = False   # FusedAdamW: weight_decay is AdamW's decoupled decay

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, *, groups=None, max_grad_norm=None,
                 skip_nonfinite=False, ema_decay=None):
        """`weight_decay` must be 0 (ValueError otherwise): torch.optim.Adam's L2 form is not implemented; use FusedAdamW
        for decoupled decay.
        `groups`: the `ArenaGroups` of the (single) parameter; `lr` and `weight_decay` of the torch param group are multiplied
        by its lr_mult / wd_mult per chunk, so a torch scheduler acting on param_groups[0]["lr"] keeps working.
        `max_grad_norm`: torch.nn.utils.clip_grad_norm_(L2) of the scaled gradient (g * grad_scale) over the non-frozen chunks.
        `skip_nonfinite`: a step whose gradient norm is inf or NaN changes nothing but `skipped_steps`.
        `ema_decay` d in [0, 1): ema = d * ema + (1 - d) * p after every applied step, started from a copy of p.
        With all four at their defaults step() calls what it called without them; otherwise it takes the grouped route for the
        optimiser's lifetime (one parameter, a multiple of 64 floats)."""
        self._check_decay(weight_decay)
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"max_grad_norm must be positive, got {max_grad_norm!r}")
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must lie in [0, 1), got {ema_decay!r}")
        if groups is not None and not isinstance(groups, ArenaGroups):
            raise ValueError(f"groups must be an ArenaGroups (optim.arena_groups), got {type(groups).__name__}")
        self.groups = groups
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.grouped = groups is not None or max_grad_norm is not None or self.skip_nonfinite or ema_decay is not None
        self._dev = {}   # per parameter: the device copies of the table and the chunk map, the scratch
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _check_decay(self, weight_decay):
        if weight_decay != 0 and not self._decoupled:
            raise ValueError(f"FusedAdam(weight_decay={weight_decay}): torch.optim.Adam's L2 weight decay is not "
                             f"implemented; use FusedAdamW for AdamW's decoupled decay")

    def add_param_group(self, param_group):
        self._check_decay(param_group.get("weight_decay", self.defaults["weight_decay"]))
        super().add_param_group(param_group)

    # ---- the grouped route ----

    def _param(self):
        ps = [p for g in self.param_groups for p in g["params"]]
        if not self.grouped or len(ps) != 1:
            raise RuntimeError("groups, clipping, step skip and the EMA belong to an optimiser over the one arena parameter that "
                               "was built with one of groups=, max_grad_norm=, skip_nonfinite=, ema_decay=")
        return ps[0]

    def _device_side(self, p):
        """(table, chunk map, scratch, scratch bytes, n_groups) on p's device, built at the first use."""
        d = self._dev.get(p)
        if d is None or d[0].device != p.device:
            n = p.numel()
            groups = self.groups or ArenaGroups([[1.0, 1.0]], np.zeros(max(n // CHUNK, 1), dtype=np.uint8))
            if n % CHUNK or groups.n_floats != n:
                raise RuntimeError(f"the grouped optimiser needs a parameter of a multiple of {CHUNK} floats that its groups cover: "
                                   f"{n} floats, groups for {groups.n_floats}")
            _lib.check(_symbol("vitseg_optim_check_groups")(groups.table.ctypes.data, len(groups.table),
                                                            groups.chunk_map.ctypes.data, len(groups.chunk_map)))
            nbytes = _symbol("vitseg_optim_scratch_bytes")(n, len(groups.table))
            d = self._dev[p] = (torch.from_numpy(groups.table).to(p.device), torch.from_numpy(groups.chunk_map).to(p.device),
                                torch.empty(nbytes, dtype=torch.uint8, device=p.device), nbytes, len(groups.table))
        return d

    def _ensure_state(self, p):
        """state[p] with everything the route needs; a state from the plain route (or a loaded one) is completed: the device
        step count starts from the host's."""
        st = self.state[p]
        if "exp_avg" not in st:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p)
            st["exp_avg_sq"] = torch.zeros_like(p)
        if self.grouped:
            if "optim_state" not in st:
                # eight 4-byte words kept as float32 bits, so that Optimizer.load_state_dict's cast to the parameter's dtype
                # leaves them alone; the integer words are read through .view(torch.int32)
                words = torch.zeros(STATE_WORDS, dtype=torch.int32)
                words[W_STEP] = int(st["step"])
                st["optim_state"] = words.view(torch.float32).to(p.device)
            if self.ema_decay is not None and "ema" not in st:
                st["ema"] = p.detach().clone()
        return st

    def _grouped_step(self, p, group, grad_scale):
        if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()):
            raise RuntimeError("FusedAdam needs contiguous fp32 HIP tensors")
        st = self._ensure_state(p)
        table, cmap, scratch, nbytes, n_groups = self._device_side(p)
        st["step"] += 1   # calls of step(); the device state counts the applied and the skipped ones
        g = p.grad.contiguous()
        n, b1, b2 = p.numel(), group["betas"][0], group["betas"][1]
        flags = 0
        if self.max_grad_norm is not None or self.skip_nonfinite:
            flags = FLAG_NORM | (FLAG_CLIP if self.max_grad_norm is not None else 0) | (FLAG_SKIP if self.skip_nonfinite else 0)
        ema = st["ema"].data_ptr() if self.ema_decay is not None else None
        with torch.cuda.device(p.device):
            stream = torch.cuda.current_stream().cuda_stream
            if flags:
                _lib.check(_symbol("vitseg_optim_grad_norm")(g.data_ptr(), n, cmap.data_ptr(), table.data_ptr(), n_groups,
                                                             grad_scale, scratch.data_ptr(), nbytes, stream))
            _lib.check(_symbol("vitseg_optim_prepare")(st["optim_state"].data_ptr(), table.data_ptr(), n_groups, n, flags,
                                                       group["lr"], b1, b2, group.get("weight_decay", 0.0),
                                                       self.max_grad_norm or 0.0, scratch.data_ptr(), nbytes, stream))
            _lib.check(_symbol("vitseg_optim_step")(p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(),
                                                    st["exp_avg_sq"].data_ptr(), ema, n, cmap.data_ptr(),
                                                    st["optim_state"].data_ptr(), b1, b2, group["eps"], grad_scale,
                                                    self.ema_decay or 0.0, scratch.data_ptr(), nbytes, stream))

    @property
    def last_grad_norm(self) -> torch.Tensor:
        """Device scalar (no sync): the norm of the scaled gradient at the last step; 0 when the optimiser neither clips nor skips."""
        p = self._param()
        return self._ensure_state(p)["optim_state"][W_NORM]

    @property
    def last_clip_coef(self) -> torch.Tensor:
        """Device scalar: the last clip coefficient, 0 when the step was skipped."""
        p = self._param()
        return self._ensure_state(p)["optim_state"][W_COEF]

    @property
    def skipped_steps(self) -> torch.Tensor:
        """Device scalar (int32, no sync): the steps skipped so far."""
        p = self._param()
        return self._ensure_state(p)["optim_state"].view(torch.int32)[W_SKIPPED]

    @property
    def applied_steps(self) -> torch.Tensor:
        p = self._param()
        return self._ensure_state(p)["optim_state"].view(torch.int32)[W_STEP]

    def ema_params(self) -> torch.Tensor:
        """The EMA of the parameter (a copy of it before the first step); laid out as the arena."""
        p = self._param()
        if self.ema_decay is None:
            raise RuntimeError("this optimiser keeps no EMA (ema_decay=None)")
        return self._ensure_state(p)["ema"]

    @contextlib.contextmanager
    def swap_ema(self):
        """Inside the block the parameter holds the EMA weights and the EMA buffer the live ones; exchanged on the device, the
        parameter's version bumped both ways (the bf16 shadow of the arena follows)."""
        p, ema = self._param(), self.ema_params()

        def exchange():
            with torch.no_grad():
                tmp = p.detach().clone()
                p.copy_(ema)
                ema.copy_(tmp)
        exchange()
        try:
            yield ema
        finally:
            exchange()

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0):
        loss = closure() if closure is not None else None
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if self.grouped:
                    self._param()
                    self._grouped_step(p, group, grad_scale)
                    torch.autograd.graph.increment_version(p)
                    continue
                if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.numel() % 4 == 0):
                    raise RuntimeError("FusedAdam needs contiguous fp32 HIP tensors whose size is a multiple of 4")
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                st["step"] += 1
                g = p.grad.contiguous()
                with torch.cuda.device(p.device):
                    _lib.check(_lib.lib().vitseg_adamw_step(
                        p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel(),
                        group["lr"], group["betas"][0], group["betas"][1], group["eps"], group.get("weight_decay", 0.0),
                        st["step"], grad_scale, torch.cuda.current_stream().cuda_stream))
                # the update went through the raw pointer: bump the version counter (no kernel) so the bf16 shadow of
                # the arena and autograd's saved-tensor checks see the modification
                torch.autograd.graph.increment_version(p)
        return loss


class FusedAdamW(FusedAdam):
    """`torch.optim.AdamW(params, lr)` (default weight_decay 1e-2, decoupled: p *= 1 - lr * weight_decay in front of the
    update) over the flat arena in one launch per step: what `PAEDTrainer.configure_optimizers` builds in the reference
    (model/PAED/classes.py:536-548).  The keyword arguments are FusedAdam's."""
    _decoupled = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kw)


# ---- the keywords of the Lightning-style modules (lightning.py, paed.py) ----
OPTION_KEYS = ("layer_decay", "no_decay", "freeze", "head_lr_mult", "max_grad_norm", "skip_nonfinite", "ema_decay",
               "weight_decay", "warmup_steps", "total_steps")


def pop_options(kw: dict) -> dict:
    """Takes the optimiser keywords out of a module's **kw (what is left goes to ViTSegmentationModel) and checks them, so
    that a bad one fails when the module is built, not at the first step."""
    opts = {k: kw.pop(k) for k in OPTION_KEYS if k in kw}
    if opts.get("warmup_steps") is not None and int(opts["warmup_steps"]) < 0:
        raise ValueError(f"warmup_steps must not be negative, got {opts['warmup_steps']!r}")
    if opts.get("weight_decay") is not None and not float(opts["weight_decay"]) >= 0.0:
        raise ValueError(f"weight_decay must not be negative, got {opts['weight_decay']!r}")
    if opts.get("max_grad_norm") is not None and not float(opts["max_grad_norm"]) > 0.0:
        raise ValueError(f"max_grad_norm must be positive, got {opts['max_grad_norm']!r}")
    if opts.get("ema_decay") is not None and not 0.0 <= float(opts["ema_decay"]) < 1.0:
        raise ValueError(f"ema_decay must lie in [0, 1), got {opts['ema_decay']!r}")
    return opts


def configure(net, lr: float, opts: dict, decoupled: bool = False):
    """The optimiser `opts` (a dict of OPTION_KEYS) describe for the arena of `net` (a ViTSegmentationModel): FusedAdamW when
    `decoupled` or a weight_decay is given, else FusedAdam; groups from `arena_groups` when one of its four arguments is
    given.  Returns (optimiser, Lightning scheduler dict or None): with warmup_steps a `warmup_cosine` over total_steps, to be
    stepped after every optimiser step ("interval": "step")."""
    group_kw = {k: opts[k] for k in ("layer_decay", "no_decay", "freeze", "head_lr_mult") if opts.get(k) is not None}
    kw = dict(groups=arena_groups(net.cfg, **group_kw) if group_kw else None, max_grad_norm=opts.get("max_grad_norm"),
              skip_nonfinite=bool(opts.get("skip_nonfinite", False)), ema_decay=opts.get("ema_decay"))
    if decoupled or opts.get("weight_decay") is not None:
        wd = {} if opts.get("weight_decay") is None else dict(weight_decay=float(opts["weight_decay"]))
        opt = FusedAdamW(net.parameters(), lr=lr, **wd, **kw)
    else:
        opt = FusedAdam(net.parameters(), lr=lr, **kw)
    sched = None
    if opts.get("warmup_steps") is not None:
        if opts.get("total_steps") is None:
            raise ValueError("warmup_steps needs total_steps: the number of optimiser steps of the run")
        sched = {"scheduler": warmup_cosine(opt, opts["warmup_steps"], opts["total_steps"]), "interval": "step", "frequency": 1}
    return opt, sched


__all__ = ["FusedAdam", "FusedAdamW", "ArenaGroups", "Row", "arena_groups", "warmup_cosine", "pop_options", "configure",
           "OPTION_KEYS", "CHUNK", "PARTIAL", "MAX_GROUPS"]
