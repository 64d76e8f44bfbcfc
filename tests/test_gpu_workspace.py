"""GPU (-m gpu): the whole-model entry points with every buffer guard-banded and the workspace poisoned.

vitseg_forward / vitseg_forward_train / vitseg_backward are called through the C ABI the way model._run, _forward_train and
_backward call them, but the workspace is exactly vitseg_query_workspace / vitseg_train_workspace bytes between two 0xFF
guards, and so are the logits, mask, gradients, loss and the inputs (x, the fp32 arena, the 16-bit / split shadow arena).
Each case runs twice, with the workspace pre-filled with 0x00 and with 0xFF bytes: the outputs must be finite and bitwise
identical (a read of a workspace byte no launch of the call wrote would tell the two apart), the guards intact (a write
past the end of any buffer, or a size formula that undercounts, lands in one) and the inputs bitwise unchanged."""
import ctypes as C

import pytest
import torch

from guard import check, guarded, snapshot, unchanged
from visiontransformer_amd import _lib, synth
from visiontransformer_amd.config import ViTSegConfig
from visiontransformer_amd.model import ViTSegmentationModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PREC = {"fp32": _lib.F32, "bf16": _lib.BF16, "fp16": _lib.F16, "fp32x3": _lib.F32X3}
CAST = {"bf16": ("vitseg_cast_params_bf16", torch.bfloat16), "fp16": ("vitseg_cast_params_f16", torch.float16),
        "fp32x3": ("vitseg_cast_params_split", torch.float32)}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _bits(t):
    return t.contiguous().view(-1).view(torch.uint8)


def _setup(cfg, precision, batch, seed=3):
    """Guarded x, fp32 arena and shadow arena (the shadow made by the cast entry point, as model._bf16_arena does)."""
    m = ViTSegmentationModel(cfg.num_classes, cfg.patch_size, cfg.hidden_size, cfg.num_hidden_layers,
                             cfg.num_attention_heads, image_size=cfg.image_size,
                             intermediate_size=cfg.intermediate_size, device=DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_state_dict(cfg, seed=seed, head_gain=4.0).items()})
    n = m.arena.numel()
    arena = guarded((n,), torch.float32, m.arena.detach(), name="arena")
    shadow = None
    if precision != "fp32":
        fn, dt = CAST[precision]
        shadow = guarded((n,), dt, "nan", name="shadow arena")
        _lib.check(getattr(_lib.lib(), fn)(arena.data_ptr(), shadow.data_ptr(), n, _stream()))
    x = guarded((batch, 3, cfg.image_size, cfg.image_size), torch.float32,
                torch.from_numpy(synth.make_images(cfg, batch, seed=seed)).to(DEV), name="x")
    torch.cuda.synchronize()
    check(arena, shadow)
    return x, arena, shadow


def _forward(cfg, precision, x, arena, shadow, fill):
    B, S, Cc = x.shape[0], cfg.image_size, cfg.num_classes
    ws = guarded(_lib.query_workspace(cfg, B, PREC[precision]), torch.uint8, fill, name="workspace")
    logits = guarded((B, Cc, S, S), torch.float32, "nan", name="logits")
    mask = guarded((B, S, S), torch.uint8, "nan", name="mask")
    snap = snapshot(x, arena, shadow)
    _lib.check(_lib.lib().vitseg_forward(C.byref(_lib.CConfig.from_config(cfg)), arena.data_ptr(), _ptr(shadow),
                                         x.data_ptr(), B, PREC[precision], logits.data_ptr(), mask.data_ptr(),
                                         ws.data_ptr(), ws.numel(), _stream()))
    torch.cuda.synchronize()
    check(x, arena, shadow, ws, logits, mask)
    unchanged(snap)
    return logits.clone(), mask.clone()


# (C, P, D, L, A, S, I): the smallest grids (S = 2 P), 17 classes, patch 8; a 1 x 1 grid (g1_p16), the generic patch
# gather (p12), 255 classes (c255) and I = 100 (the large route by I; fp32 formats only: the 16-bit ones need I % 64 == 0)
INFER_CFGS = {
    "c2_p16_s32": (2, 16, 64, 1, 1, 32, 128),
    "c17_p8_s16": (17, 8, 128, 2, 2, 16, 256),
    "c3_p16_s48": (3, 16, 128, 1, 2, 48, 256),
    "g1_p16": (3, 16, 128, 1, 2, 16, 256),
    "p12": (3, 12, 128, 1, 2, 96, 256),
    "c255": (255, 16, 64, 1, 1, 224, 256),
    "i100": (2, 16, 128, 1, 2, 64, 100),
}
OLD_CFGS = ("c2_p16_s32", "c17_p8_s16", "c3_p16_s48")   # (these keep their fp32x3 / small ids, which skip)
FORWARD_RUNS = [(n, p, r) for n in sorted(INFER_CFGS) for p in ("fp32", "bf16", "fp16", "fp32x3") for r in ("small", "large")
                if (n in OLD_CFGS or (p, r) != ("fp32x3", "small")) and (n != "i100" or (p in ("fp32", "fp32x3") and r == "large"))]


@pytest.mark.parametrize("name,precision,route", FORWARD_RUNS)
def test_forward_guarded_and_poisoned(name, precision, route):
    if precision == "fp32x3" and route == "small":
        pytest.skip("fp32x3 has no small-batch route")
    c = INFER_CFGS[name]
    cfg = ViTSegConfig(*c[:5], image_size=c[5], intermediate_size=c[6])
    batch = 2
    x, arena, shadow = _setup(cfg, precision, batch)
    with _lib.option("no_small", int(route == "large")):
        assert _lib.forward_route(cfg, batch, PREC[precision]) == route
        l0, m0 = _forward(cfg, precision, x, arena, shadow, "zero")
        l1, m1 = _forward(cfg, precision, x, arena, shadow, "nan")
    assert torch.isfinite(l0).all()
    assert int(m0.max()) < cfg.num_classes
    assert torch.equal(_bits(l0), _bits(l1)), "logits depend on the workspace's prior contents"
    assert torch.equal(m0, m1)


def test_forward_large_batch_conv_dma_guarded_and_poisoned():
    """The LDS-DMA head conv of the large-batch fp32 forward (switch conv_dma)."""
    cfg = ViTSegConfig(2, 16, 128, 1, 2, image_size=64, intermediate_size=256)
    x, arena, shadow = _setup(cfg, "fp32", 3)
    with _lib.option("no_small", 1), _lib.option("conv_dma", 1):
        l0, m0 = _forward(cfg, "fp32", x, arena, shadow, "zero")
        l1, m1 = _forward(cfg, "fp32", x, arena, shadow, "nan")
    with _lib.option("no_small", 1):
        l2, _ = _forward(cfg, "fp32", x, arena, shadow, "nan")
    assert torch.isfinite(l0).all()
    assert torch.equal(_bits(l0), _bits(l1)) and torch.equal(m0, m1)
    assert torch.equal(_bits(l0), _bits(l2))   # the switch is bit-identical


def _train_step(cfg, precision, x, arena, shadow, fill, drop, target=None, grad_logits=None):
    """forward_train (workspace poisoned right before it) + backward, every buffer guarded."""
    B, S, Cc = x.shape[0], cfg.image_size, cfg.num_classes
    pcfg = C.byref(_lib.CConfig.from_config(cfg))
    ws = guarded(_lib.train_workspace(cfg, B, PREC[precision]), torch.uint8, fill, name="train workspace")
    logits = guarded((B, Cc, S, S), torch.float32, "nan", name="logits")
    grads = guarded(arena.shape, torch.float32, "nan", name="grads")
    loss = guarded((1,), torch.float32, "nan", name="loss") if target is not None else None
    snap = snapshot(x, arena, shadow, target, grad_logits)
    L = _lib.lib()
    _lib.check(L.vitseg_forward_train(pcfg, arena.data_ptr(), _ptr(shadow), x.data_ptr(), B, PREC[precision], drop[0],
                                      drop[1], logits.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    _lib.check(L.vitseg_backward(pcfg, arena.data_ptr(), _ptr(shadow), x.data_ptr(), B, PREC[precision], drop[0], drop[1],
                                 _ptr(target), int(target is not None and target.dtype == torch.uint8), _ptr(grad_logits),
                                 grads.data_ptr(), _ptr(loss), 1.0, None, ws.data_ptr(), ws.numel(), _stream()))
    torch.cuda.synchronize()
    check(x, arena, shadow, target, grad_logits, ws, logits, grads, loss)
    unchanged(snap)
    assert torch.isfinite(logits).all() and torch.isfinite(grads).all()
    return logits.clone(), grads.clone(), (loss.clone() if loss is not None else None)


# (C, P, D, L, A, S, I, batch)
TRAIN_CFGS = {
    "c3_p16_s32": (3, 16, 64, 1, 1, 32, 128, 2),        # the smallest grid
    "c2_p32_s64_narrow": (2, 32, 64, 1, 1, 64, 128, 1),  # patch 32 with a narrow MLP: the patch-embedding slabs
    "c17_p8_s16": (17, 8, 128, 2, 2, 16, 256, 2),
    "g1_p16": (3, 16, 128, 1, 2, 16, 256, 2),            # a 1 x 1 token grid
    "p12": (3, 12, 128, 1, 2, 96, 256, 2),               # the generic patch gather / im2col
    "i100": (2, 16, 128, 1, 2, 64, 100, 2),              # the large route by I (fp32 only: bf16 needs I % 64 == 0)
}
TRAIN_RUNS = [(n, p, r) for n in sorted(TRAIN_CFGS) for p, r in (("fp32", "small"), ("fp32", "large"), ("bf16", None))
              if n != "i100" or (p, r) == ("fp32", "large")]


def _train_case(cfg, precision, B, dropout):
    """The three backward entries (uint8 targets, int64 targets, grad_logits) after a workspace poisoned with 0x00 and
    with 0xFF; returns the results of the 0xFF run after checking the two runs are bitwise the same."""
    S = cfg.image_size
    x, arena, shadow = _setup(cfg, precision, B)
    if precision == "fp32":
        shadow = None   # the fp32 training step takes no shadow arena
    g = torch.Generator().manual_seed(9)
    t64 = guarded((B, S, S), torch.int64, torch.randint(0, cfg.num_classes, (B, S, S), generator=g).to(DEV), name="target")
    t8 = guarded((B, S, S), torch.uint8, t64.to(torch.uint8), name="target u8")
    gl = guarded((B, cfg.num_classes, S, S), torch.float32,
                 (torch.randn(B, cfg.num_classes, S, S, generator=g) * 1e-3).to(DEV), name="grad_logits")
    drop = (dropout, 0x1234_5678_9ABC if dropout else 0)
    out = {}
    for fill in ("zero", "nan"):
        out[fill] = (_train_step(cfg, precision, x, arena, shadow, fill, drop, target=t8),
                     _train_step(cfg, precision, x, arena, shadow, fill, drop, target=t64),
                     _train_step(cfg, precision, x, arena, shadow, fill, drop, grad_logits=gl))
    for fill in ("zero", "nan"):
        (l8, g8, loss8), (l64, g64, loss64), (lp, gp, _) = out[fill]
        assert torch.isfinite(loss8).all()
        assert torch.equal(_bits(loss8), _bits(loss64)) and torch.equal(_bits(g8), _bits(g64)), "uint8 / int64 targets differ"
        assert torch.equal(_bits(l8), _bits(l64)) and torch.equal(_bits(l8), _bits(lp))
    for a, b in zip(out["zero"], out["nan"]):
        for u, v in zip(a, b):
            if u is not None:
                assert torch.equal(_bits(u), _bits(v)), "training results depend on the workspace's prior contents"
    return out["nan"]


# The training step's route is the fp32 forward's (small_applies(cfg, batch, VITSEG_F32) in vitseg_forward_train and
# vitseg_backward, the answer vitseg_forward_route gives for VITSEG_F32); the bf16 training step has one route.
@pytest.mark.parametrize("dropout", [0.0, 0.1])
@pytest.mark.parametrize("name,precision,route", TRAIN_RUNS)
def test_train_step_guarded_and_poisoned(name, precision, route, dropout):
    c = TRAIN_CFGS[name]
    cfg = ViTSegConfig(*c[:5], image_size=c[5], intermediate_size=c[6])
    with _lib.option("no_small", int(route == "large")):
        if route is not None:
            assert _lib.forward_route(cfg, c[7], _lib.F32) == route
        _train_case(cfg, precision, c[7], dropout)


def test_train_step_shared_dropout_words_guarded_and_poisoned():
    """bf16 training keeps packed attention-dropout words for sequences of a multiple of 128 patches, per layer or (option
    dropw_limit_mb 0) in one buffer regenerated per layer; both layouts guarded and poisoned, and bitwise the same."""
    cfg = ViTSegConfig(3, 8, 64, 2, 1, image_size=128, intermediate_size=128)   # 256 patches
    per_layer = _train_case(cfg, "bf16", 1, 0.1)
    with _lib.option("dropw_limit_mb", 0):
        shared = _train_case(cfg, "bf16", 1, 0.1)
    for a, b in zip(per_layer, shared):
        for u, v in zip(a, b):
            if u is not None:
                assert torch.equal(_bits(u), _bits(v))
