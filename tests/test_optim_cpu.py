"""CPU (-m "not gpu"): the fine-tuning optimiser's host side -- include/vitseg_optim.h against `_ext.EXT_LATER["optim"]`, the
argument checks of the entry points (they come before any launch), `optim.arena_groups`, `optim.warmup_cosine`, the flags of
the training scripts, the keywords of the Lightning-style modules, and tests/optim_ref.py against a hand-written AdamW."""
import argparse
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from optim_ref import GroupedReference
from test_binding_cpu import ROOT, parse_header, signature_errors
from visiontransformer_amd import _ext, _lib, optim, scripts
from visiontransformer_amd.config import ViTSegConfig

HEADER = os.path.join(ROOT, "include", "vitseg_optim.h")
NAMES = ["vitseg_optim_version", "vitseg_optim_scratch_bytes", "vitseg_optim_check_groups", "vitseg_optim_grad_norm",
         "vitseg_optim_prepare", "vitseg_optim_step"]
VITB = ViTSegConfig(2, 16, 768, 12, 12, image_size=512)
SMALLEST = ViTSegConfig(3, 16, 64, 2, 1, image_size=32)   # hidden 64, one head: the last tensor has 3 values, 61 of padding


def _table():
    return {name: (restype, list(argtypes)) for name, restype, argtypes in _ext.EXT_LATER["optim"][2]}


# ---- the family header and its table ----

def test_family_header_is_the_table_both_ways():
    decls, structs, enums, defines = parse_header(open(HEADER).read())
    assert _ext.EXT_LATER["optim"][:2] == ("vitseg_optim.h", "the fine-tuning optimiser")
    assert sorted(decls) == sorted(NAMES) == sorted(_table()) and not structs and not enums
    assert signature_errors(decls, _table()) == []
    assert defines == {"VITSEG_OPTIM_VERSION": 100, "VITSEG_OPTIM_CHUNK": optim.CHUNK, "VITSEG_OPTIM_PARTIAL": optim.PARTIAL,
                       "VITSEG_OPTIM_MAX_GROUPS": optim.MAX_GROUPS, "VITSEG_OPTIM_STATE_BYTES": 4 * optim.STATE_WORDS,
                       "VITSEG_OPTIM_NORM": optim.FLAG_NORM, "VITSEG_OPTIM_CLIP": optim.FLAG_CLIP,
                       "VITSEG_OPTIM_SKIP": optim.FLAG_SKIP}
    assert _ext.OPTIM_VERSION == 100 and _ext.EXT_VERSIONS["optim"] == ("vitseg_optim_version", 100)
    tab = _table()   # the comparison can fail
    tab["vitseg_optim_prepare"] = (C.c_int, tab["vitseg_optim_prepare"][1][:5] + [C.c_double] + tab["vitseg_optim_prepare"][1][6:])
    assert signature_errors(decls, tab) == ["vitseg_optim_prepare: argument 5: c_double for float"]


def test_family_leaves_the_first_header_alone():
    assert all("optim" not in name for name in _lib.EXPORTS)
    assert "vitseg_optim" not in open(os.path.join(ROOT, "include", "vitseg.h")).read()
    assert '#include "vitseg.h"' in open(HEADER).read()
    assert set(_ext.EXT_VERSIONS) == set(_ext.EXT_SIGNATURES) | set(_ext.EXT_FAMILIES) | set(_ext.EXT_LATER)
    l = C.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        assert hasattr(l, name), name
    assert _ext.ext_symbol("optim", "vitseg_optim_version")() == 100


def test_every_status_code_without_a_device():
    """The argument checks come before any launch: every address is a live host buffer that no call reaches."""
    size = _ext.ext_symbol("optim", "vitseg_optim_scratch_bytes")
    norm, prepare, step, groups = (_ext.ext_symbol("optim", "vitseg_optim_" + n) for n in ("grad_norm", "prepare", "step", "check_groups"))
    buf = (C.c_uint8 * 8192)()
    p = C.addressof(buf)
    need = size(128, 2)
    assert need == 256 + 256 * 16 and size(8192, 1) == need and size(8192 + 64, 1) == need and size(2049 * 64 * 128, 256) > need
    for bad in ((0, 1), (63, 1), (65, 1), (64, 0), (64, 257), (64, -1)):
        assert size(*bad) == 0, bad

    def call_norm(g=p, n=128, cmap=p, table=p, ng=2, scratch=p, nbytes=need):
        return norm(g, n, cmap, table, ng, 1.0, scratch, nbytes, None)

    def call_prepare(state=p, table=p, ng=2, n=128, flags=7, lr=1e-4, b1=0.9, b2=0.999, wd=1e-2, max_norm=1.0, scratch=p, nbytes=need):
        return prepare(state, table, ng, n, flags, lr, b1, b2, wd, max_norm, scratch, nbytes, None)

    def call_step(params=p, g=p, m=p, v=p, ema=None, n=128, cmap=p, state=p, b1=0.9, b2=0.999, eps=1e-8, d=0.0, scratch=p, nbytes=need):
        return step(params, g, m, v, ema, n, cmap, state, b1, b2, eps, 1.0, d, scratch, nbytes, None)
    nan = float("nan")
    for fn, cases in ((call_norm, (dict(g=None), dict(cmap=None), dict(table=None), dict(scratch=None), dict(n=0), dict(n=100),
                                   dict(ng=0), dict(ng=257))),
                      (call_prepare, (dict(state=None), dict(table=None), dict(scratch=None), dict(n=96), dict(ng=0), dict(ng=257),
                                      dict(flags=8), dict(flags=-1), dict(flags=2), dict(flags=4), dict(flags=6), dict(wd=-1e-3),
                                      dict(wd=nan), dict(lr=-1.0), dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=nan),
                                      dict(b1=1.0), dict(b2=-0.1))),
                      (call_step, (dict(params=None), dict(g=None), dict(m=None), dict(v=None), dict(cmap=None), dict(state=None),
                                   dict(scratch=None), dict(n=32), dict(n=0), dict(ema=p, d=1.0), dict(ema=p, d=-0.1),
                                   dict(ema=p, d=nan), dict(eps=-1.0), dict(b1=1.5)))):
        for kw in cases:
            assert fn(**kw) == _lib.EINVAL, (fn.__name__, kw)
            assert b"optim_" in _lib.lib().vitseg_last_error()
        assert fn(nbytes=need - 1) == _lib.EWORKSPACE, fn.__name__
    table = (C.c_float * 4)(1.0, 1.0, 0.0, 0.5)
    cmap = (C.c_uint8 * 3)(0, 1, 1)
    assert groups(table, 2, cmap, 3) == _lib.OK and groups(table, 2, None, 0) == _lib.OK
    for bad in ((-0.5, 1.0, 0.0, 0.5), (1.0, -1.0, 0.0, 0.5), (1.0, 1.0, nan, 0.5), (1.0, 1.0, 0.0, float("inf"))):
        assert groups((C.c_float * 4)(*bad), 2, cmap, 3) == _lib.EINVAL, bad
    assert groups(table, 1, cmap, 3) == _lib.EINVAL and groups(None, 2, cmap, 3) == _lib.EINVAL
    assert groups(table, 0, cmap, 3) == _lib.EINVAL and groups(table, 257, cmap, 3) == _lib.EINVAL
    assert bytes(buf) == bytes(8192)   # nothing was written


# ---- arena_groups ----

@pytest.mark.parametrize("cfg", [VITB, SMALLEST], ids=["vitb16_512", "smallest"])
def test_arena_groups_cover_every_chunk_once_with_the_depth_multipliers(cfg):
    L = cfg.num_hidden_layers
    total = _lib.param_count(cfg)
    g = optim.arena_groups(cfg, layer_decay=0.75, no_decay="default", head_lr_mult=2.0)
    assert len(g.chunk_map) * 64 == total == g.n_floats and g.chunk_map.dtype == np.uint8 and g.table.dtype == np.float32
    assert len(g.rows) == 4 + 12 * L + 6
    cover = np.zeros(total // 64, dtype=np.int64)
    for r in g.rows:
        off, n = _lib.param_offset(cfg, r.tensor, r.layer)
        assert r.offset == off and r.offset % 64 == 0 and r.numel % 64 == 0 and n <= r.numel < n + 64, r
        cover[r.offset // 64:(r.offset + r.numel) // 64] += 1
        assert (g.chunk_map[r.offset // 64:(r.offset + r.numel) // 64] == r.group).all(), r
        assert tuple(g.table[r.group]) == (np.float32(r.lr_mult), np.float32(r.wd_mult)), r
        depth = 0 if "embeddings" in r.name else L + 1 if not r.name.startswith("backbone.layers.") else r.layer + 1
        want = 0.75 ** (L + 1 - depth) * (2.0 if r.name.startswith("seg_head.") else 1.0)
        assert r.lr_mult == float(np.float32(want)), (r, want)
        plain = r.name.endswith(".weight") and "layernorm" not in r.name
        assert r.wd_mult == (1.0 if plain else 0.0), r
    assert (cover == 1).all()                                     # every chunk exactly once, padding included
    assert len({tuple(t) for t in g.table}) == len(g.table)       # equal pairs are merged
    last = g.rows[-1]
    assert last.name == "seg_head.2.bias" and last.offset + last.numel == total
    if cfg is SMALLEST:
        assert _lib.param_offset(cfg, last.tensor, 0)[1] == 3 and last.numel == 64   # 3 values, 61 floats of padding
    text = g.describe()
    assert f"{len(g.table)} groups over {total} floats" in text and "weight decay x 0" in text and len(text.splitlines()) == len(g.table) + 1


def test_arena_groups_spellings_of_no_decay_and_freeze():
    cfg, L = SMALLEST, SMALLEST.num_hidden_layers
    plain = optim.arena_groups(cfg)
    assert plain.table.tolist() == [[1.0, 1.0]] and not plain.chunk_map.any() and not plain.frozen.any()

    def no_decay_names(spec):
        return {r.name for r in optim.arena_groups(cfg, no_decay=spec).rows if r.wd_mult == 0.0}
    every = no_decay_names("default")
    assert every == no_decay_names(("bias", "norm", "cls", "pos")) == no_decay_names(["pos", "cls", "norm", "bias"])
    assert no_decay_names("cls") == {"backbone.embeddings.cls_token"} == no_decay_names(("cls",))
    assert no_decay_names("pos") == {"backbone.embeddings.position_embeddings"}
    assert no_decay_names("norm") == {n for n in every if "layernorm" in n} and len(no_decay_names("norm")) == 4 * L + 2
    assert no_decay_names("bias") == {n for n in every if n.endswith(".bias")}
    assert no_decay_names(()) == set() == no_decay_names(None)

    def frozen_names(spec):
        return {r.name for r in optim.arena_groups(cfg, freeze=spec, layer_decay=0.9).rows if r.lr_mult == 0.0}
    emb = frozen_names("embeddings")
    assert emb == {r.name for r in plain.rows if "embeddings" in r.name} and len(emb) == 4 and emb == frozen_names(0)
    assert frozen_names(1) == emb | {r.name for r in plain.rows if r.name.startswith("backbone.layers.0.")}
    assert frozen_names(L) == {r.name for r in plain.rows if "embeddings" in r.name or r.name.startswith("backbone.layers.")}
    assert frozen_names("backbone") == {r.name for r in plain.rows if not r.name.startswith("seg_head.")}
    assert frozen_names(()) == set() == frozen_names(None)
    g = optim.arena_groups(cfg, freeze="backbone")
    assert g.frozen.sum() * 64 == sum(r.numel for r in g.rows if not r.name.startswith("seg_head."))


def test_arena_groups_refusals():
    for kw in (dict(layer_decay=0.0), dict(layer_decay=1.5), dict(layer_decay=-0.5), dict(layer_decay=float("nan")),
               dict(layer_decay="0.5"), dict(no_decay="biases"), dict(no_decay=("bias", "head")), dict(freeze="head"),
               dict(freeze=SMALLEST.num_hidden_layers + 1), dict(freeze=-1), dict(freeze=True), dict(head_lr_mult=-1.0)):
        with pytest.raises(ValueError):
            optim.arena_groups(SMALLEST, **kw)
    deep = ViTSegConfig(2, 16, 64, 300, 1, image_size=32)          # 302 depths: more than 256 distinct multipliers
    with pytest.raises(ValueError, match="more than 256"):
        optim.arena_groups(deep, layer_decay=0.99)
    assert len(optim.arena_groups(deep).table) == 1
    with pytest.raises(ValueError):
        optim.ArenaGroups([[1.0, 1.0]], [0, 1])
    with pytest.raises(ValueError):
        optim.ArenaGroups([[-1.0, 1.0]], [0])


# ---- the optimiser's arguments, the scheduler, the flags ----

def test_optimizer_arguments_are_checked_when_it_is_built():
    p = torch.nn.Parameter(torch.zeros(128))
    for kw in (dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(groups=[[1, 1]])):
        with pytest.raises(ValueError):
            optim.FusedAdamW([p], **kw)
    with pytest.raises(ValueError, match="L2 weight decay"):
        optim.FusedAdam([p], weight_decay=1e-2, max_grad_norm=1.0)
    assert not optim.FusedAdamW([p]).grouped and not optim.FusedAdam([p], lr=1e-5).grouped
    for kw in (dict(groups=optim.ArenaGroups([[1, 1]], [0, 0])), dict(max_grad_norm=1.0), dict(skip_nonfinite=True), dict(ema_decay=0.0)):
        assert optim.FusedAdam([p], **kw).grouped, kw
    with pytest.raises(RuntimeError, match="keeps no EMA"):
        optim.FusedAdam([p], max_grad_norm=1.0).ema_params()
    with pytest.raises(RuntimeError, match="one arena parameter"):
        optim.FusedAdam([p]).last_grad_norm


def test_warmup_cosine_values():
    p = torch.nn.Parameter(torch.zeros(4))
    opt = torch.optim.SGD([p], lr=2.0)
    sched = optim.warmup_cosine(opt, warmup_steps=4, total_steps=12, min_lr_ratio=0.1)
    lrs = []
    for _ in range(14):
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    assert lrs[0] == 0.0 and lrs[2] == 1.0 and lrs[4] == 2.0                       # step 0, half way, `warmup`
    assert lrs[8] == pytest.approx(2.0 * (0.1 + 0.9 * 0.5)) and lrs[12] == pytest.approx(0.2) and lrs[13] == pytest.approx(0.2)
    assert all(a > b for a, b in zip(lrs[4:12], lrs[5:13]))
    assert optim.warmup_cosine(torch.optim.SGD([p], lr=1.0), 0, 5).get_last_lr() == [1.0]
    for bad in ((-1, 5, 0.0), (6, 5, 0.0), (0, 0, 0.0), (1, 5, 1.5)):
        with pytest.raises(ValueError):
            optim.warmup_cosine(opt, *bad)


def _flags(argv):
    ap = argparse.ArgumentParser()
    scripts.add_optim_arguments(ap)
    return ap.parse_args(argv)


def test_script_flags_map_to_the_keywords():
    assert scripts.optim_options(_flags([])) == {}
    a = _flags(["--layer-decay", "0.75", "--no-decay", "--freeze", "embeddings", "--head-lr-mult", "10", "--max-grad-norm", "1",
                "--skip-nonfinite", "--ema-decay", "0.999", "--weight-decay", "0.05", "--warmup-steps", "100"])
    want = dict(layer_decay=0.75, no_decay="default", freeze="embeddings", head_lr_mult=10.0, max_grad_norm=1.0,
                skip_nonfinite=True, ema_decay=0.999, weight_decay=0.05, warmup_steps=100)
    assert scripts.optim_options(a) == want and scripts.optim_options(a, total_steps=500) == dict(want, total_steps=500)
    assert set(want) | {"total_steps"} == set(optim.OPTION_KEYS)
    assert scripts.optim_options(_flags(["--no-decay", "bias,norm"])) == dict(no_decay=("bias", "norm"))
    assert scripts.optim_options(_flags(["--no-decay", "default"])) == dict(no_decay="default")
    assert scripts.optim_options(_flags(["--freeze", "3"])) == dict(freeze=3)
    assert scripts.optim_options(_flags(["--freeze", "backbone"])) == dict(freeze="backbone")
    assert scripts.optimizer_steps(3, 8, 4) == 6 and scripts.optimizer_steps(3, 9, 4) == 9 and scripts.optimizer_steps(2, 5, 1) == 10


def test_module_keywords_build_the_optimizer():
    from visiontransformer_amd import paed
    from visiontransformer_amd.lightning import LightningViTModel
    args = (3, 16, 64, 2, 1)
    lm = LightningViTModel(*args, image_size=32, device="cpu")
    opt = lm.configure_optimizers()
    assert lm.optim_options == {} and type(opt) is optim.FusedAdam and not opt.grouped and opt.param_groups[0]["lr"] == 1e-5
    lm = LightningViTModel(*args, image_size=32, device="cpu", layer_decay=0.75, no_decay="default", freeze="embeddings",
                           max_grad_norm=1.0)
    opt = lm.configure_optimizers()
    assert type(opt) is optim.FusedAdam and opt.grouped and opt.max_grad_norm == 1.0 and opt.ema_decay is None
    want = optim.arena_groups(lm.model.cfg, layer_decay=0.75, no_decay="default", freeze="embeddings")
    assert opt.groups.n_floats == lm.model.arena.numel() and (opt.groups.chunk_map == want.chunk_map).all()
    assert (opt.groups.table == want.table).all() and opt.groups.frozen.any()
    lm = LightningViTModel(*args, image_size=32, device="cpu", weight_decay=0.05, ema_decay=0.99, skip_nonfinite=True,
                           warmup_steps=2, total_steps=8)
    both = lm.configure_optimizers()
    opt, sched = both["optimizer"], both["lr_scheduler"]
    assert type(opt) is optim.FusedAdamW and opt.param_groups[0]["weight_decay"] == 0.05 and opt.ema_decay == 0.99 and opt.skip_nonfinite
    assert sched["interval"] == "step" and opt.param_groups[0]["lr"] == 0.0 and opt.groups is None
    lm.optim_options.pop("total_steps")
    with pytest.raises(ValueError, match="total_steps"):
        lm.configure_optimizers()
    scripts.set_total_steps(lm, 3, 8, 4)
    assert lm.optim_options["total_steps"] == 6
    for bad in (dict(max_grad_norm=0.0), dict(ema_decay=1.0), dict(weight_decay=-1.0), dict(warmup_steps=-1)):
        with pytest.raises(ValueError):
            LightningViTModel(*args, image_size=32, device="cpu", **bad)
    pm = paed.LightningViTModel(17, 16, 64, 2, 1, image_size=32, device="cpu", weight_decay=0.01)
    assert type(pm.configure_optimizers()) is optim.FusedAdamW
    assert type(paed.LightningViTModel(17, 16, 64, 2, 1, image_size=32, device="cpu").configure_optimizers()) is optim.FusedAdam
    pt = paed.PAEDTrainer(1, 16, 64, 2, 1, image_size=32, device="cpu")
    plain = pt.configure_optimizers()
    assert type(plain["optimizer"]) is optim.FusedAdamW and not plain["optimizer"].grouped
    assert isinstance(plain["lr_scheduler"]["scheduler"], torch.optim.lr_scheduler.ReduceLROnPlateau)
    pt = paed.PAEDTrainer(1, 16, 64, 2, 1, image_size=32, device="cpu", freeze=1, max_grad_norm=2.0)
    kept = pt.configure_optimizers()
    assert kept["optimizer"].grouped and kept["optimizer"].param_groups[0]["weight_decay"] == 1e-2
    assert isinstance(kept["lr_scheduler"]["scheduler"], torch.optim.lr_scheduler.ReduceLROnPlateau)
    pt = paed.PAEDTrainer(1, 16, 64, 2, 1, image_size=32, device="cpu", warmup_steps=1, total_steps=4)
    assert pt.configure_optimizers()["lr_scheduler"]["interval"] == "step"


# ---- the reference against a hand-written AdamW ----

def test_reference_equals_a_hand_written_adamw_in_fp64():
    """3 chunks: group 0 (1, 1), group 1 (0.5, 0), group 2 frozen; clipping on, EMA on, three steps with one skipped."""
    gen = torch.Generator().manual_seed(3)
    n, lr, wd, b1, b2, eps, d, max_norm = 192, 1e-2, 0.1, 0.9, 0.999, 1e-8, 0.9, 0.5
    p0 = torch.randn(n, generator=gen, dtype=torch.float64)
    table, cmap = [(1.0, 1.0), (0.5, 0.0), (0.0, 1.0)], [1, 2, 0]
    ref = GroupedReference(p0, cmap, table, lr, weight_decay=wd, betas=(b1, b2), eps=eps, max_grad_norm=max_norm,
                           skip_nonfinite=True, ema_decay=d)
    p, m, v, ema, t = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), p0.clone(), 0
    lr_e = torch.tensor([0.5] * 64 + [0.0] * 64 + [1.0] * 64, dtype=torch.float64) * lr
    wd_e = torch.tensor([0.0] * 64 + [1.0] * 64 + [1.0] * 64, dtype=torch.float64) * wd
    live = lr_e > 0
    for k in range(4):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * (3.0 if k < 2 else 0.01)
        g[100] = float("nan")                                   # in the frozen chunk: never counts
        if k == 1:
            g[5] = float("inf")
        applied = ref.step(g, grad_scale=0.5)
        gs = g * 0.5
        norm = gs[live].pow(2).sum().sqrt()
        if not math.isfinite(float(norm)):
            assert not applied and ref.skipped == 1
        else:
            assert applied
            coef = min(1.0, max_norm / (float(norm) + 1e-6))
            assert (coef < 1.0) == (k < 2)
            t += 1
            for i in range(n):
                if not live[i]:
                    continue
                gi = float(gs[i]) * coef
                m[i] = b1 * m[i] + (1 - b1) * gi
                v[i] = b2 * v[i] + (1 - b2) * gi * gi
                p[i] = p[i] * (1 - float(lr_e[i]) * float(wd_e[i]))
                p[i] = p[i] - float(lr_e[i]) / (1 - b1 ** t) * float(m[i]) / (math.sqrt(float(v[i])) / math.sqrt(1 - b2 ** t) + eps)
                ema[i] = d * ema[i] + (1 - d) * p[i]
        assert torch.allclose(ref.full_params(), p, rtol=1e-12, atol=1e-14)
        assert torch.allclose(ref.full_state("exp_avg"), m, rtol=1e-12, atol=1e-16)
        assert torch.allclose(ref.full_state("exp_avg_sq"), v, rtol=1e-12, atol=1e-18)
        assert torch.allclose(ref.ema, ema, rtol=1e-12, atol=1e-14)
    assert ref.steps == 3 and ref.skipped == 1 and torch.equal(ref.full_params()[64:128], p0[64:128])
    assert torch.equal(ref.live_mask(), live)
    ref.set_lr(0.0)
    before = ref.full_params()
    ref.step(torch.ones(n, dtype=torch.float64))
    assert torch.equal(ref.full_params(), before)               # lr 0: neither an update nor a decay
