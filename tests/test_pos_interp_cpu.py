"""CPU: interpolated position embeddings (HF `interpolate_pos_encoding=True`) -- the C ABI's `*_at` entry points, the
Python surface's validation, and a numpy restatement of the bicubic resampling that sizes the GPU tests' tolerances.
No compute entry point runs here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from visiontransformer_amd import _lib
from visiontransformer_amd.config import ViTSegConfig
from visiontransformer_amd.lightning import LightningViTModel
from visiontransformer_amd.model import ViTSegmentationModel
from visiontransformer_amd.worker import parse_model_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["vitseg_query_workspace_at", "vitseg_workspace_offset_at", "vitseg_forward_at", "vitseg_train_workspace_at",
       "vitseg_forward_train_at", "vitseg_backward_at", "vitseg_pos_interp", "vitseg_pos_interp_bwd"]

CONFIGS = [ViTSegConfig(2, 16, 192, 12, 3, image_size=224), ViTSegConfig(2, 16, 768, 12, 12, image_size=512),
           ViTSegConfig(2, 8, 512, 2, 8, image_size=224), ViTSegConfig(17, 16, 768, 2, 12, image_size=224),
           ViTSegConfig(3, 4, 512, 1, 8, image_size=64)]


def _c(cfg):
    return ctypes.byref(_lib.CConfig.from_config(cfg))


def _up(n, a=256):
    return (n + a - 1) // a * a


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "vitseg.h")).read()
    declared = set(re.findall(r"\b(vitseg_[a-z0-9_]+)\s*\(", hdr))
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in _lib.AT_EXPORTS and name in _lib.EXPORTS, name
        assert hasattr(l, name), name
        assert _lib.at_symbol(name).argtypes, name
    assert _lib.lib().vitseg_version() == 110


def test_missing_symbol_asks_for_a_rebuild():
    with pytest.raises(RuntimeError, match="rebuild"):
        _lib.at_symbol("vitseg_not_a_symbol_at")


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: f"P{c.patch_size}D{c.hidden_size}S{c.image_size}")
def test_at_native_size_is_exactly_the_plain_query(cfg):
    """image_size_in == cfg.image_size: the same workspace bytes and buffer offsets, for every precision and batch sizes on
    both sides of the route boundary (small / large), and the same training workspaces."""
    L = _lib.lib()
    routes = set()
    for precision in (_lib.F32, _lib.BF16, _lib.F16, _lib.F32X3):
        for batch in (1, 2, 5, 16, 33, 64):
            routes.add(_lib.forward_route(cfg, batch, precision))
            a, b = ctypes.c_size_t(), ctypes.c_size_t()
            _lib.check(L.vitseg_query_workspace(_c(cfg), batch, precision, ctypes.byref(a)))
            _lib.check(L.vitseg_query_workspace_at(_c(cfg), cfg.image_size, batch, precision, ctypes.byref(b)))
            assert a.value == b.value
            for buf in (_lib.BUF_TOKENS, _lib.BUF_LOWRES):
                o1, n1, o2, n2 = (ctypes.c_size_t() for _ in range(4))
                _lib.check(L.vitseg_workspace_offset(_c(cfg), batch, precision, buf, ctypes.byref(o1), ctypes.byref(n1)))
                _lib.check(L.vitseg_workspace_offset_at(_c(cfg), cfg.image_size, batch, precision, buf, ctypes.byref(o2),
                                                        ctypes.byref(n2)))
                assert (o1.value, n1.value) == (o2.value, n2.value)
            if precision in (_lib.F32, _lib.BF16):
                _lib.check(L.vitseg_train_workspace(_c(cfg), batch, precision, ctypes.byref(a)))
                _lib.check(L.vitseg_train_workspace_at(_c(cfg), cfg.image_size, batch, precision, ctypes.byref(b)))
                assert a.value == b.value
            assert _lib.query_workspace(cfg, batch, precision, cfg.image_size) == _lib.query_workspace(cfg, batch, precision)
    if cfg.hidden_size % 64 == 0 and cfg.image_size >= 224:
        assert routes == {"small", "large"}, routes


@pytest.mark.parametrize("S_in", [160, 384, 512])
def test_other_size_adds_only_the_table_regions(S_in):
    """The activations of another input size are those of a model built at that size; the workspace only gains the
    resampled table (forward) and, for training, the input-grid dpos plus the adjoint's x-pass scratch -- behind every
    other region, so the buffer offsets equal the native-size model's."""
    cfg = ViTSegConfig(2, 16, 768, 2, 12, image_size=224)
    cin = ViTSegConfig(2, 16, 768, 2, 12, image_size=S_in)
    g0, g1, D = 14, S_in // 16, 768
    for precision in (_lib.F32, _lib.BF16, _lib.F16, _lib.F32X3):
        for batch in (1, 3, 40):
            assert (_lib.query_workspace(cfg, batch, precision, S_in)
                    == _lib.query_workspace(cin, batch, precision) + _up((1 + g1 * g1) * D * 4))
            for buf in (_lib.BUF_TOKENS, _lib.BUF_LOWRES):
                assert _lib.workspace_offset(cfg, batch, precision, buf, S_in) == _lib.workspace_offset(cin, batch, precision, buf)
            assert _lib.forward_route(cfg, batch, precision, S_in) == _lib.forward_route(cin, batch, precision)
            if precision in (_lib.F32, _lib.BF16):
                extra = 2 * _up((1 + g1 * g1) * D * 4) + _up(g1 * g0 * D * 4)
                assert _lib.train_workspace(cfg, batch, precision, S_in) == _lib.train_workspace(cin, batch, precision) + extra


def test_at_validation_is_a_shape_error():
    cfg = ViTSegConfig(2, 16, 192, 2, 3, image_size=224)
    for bad in (200, 0, -16, 8):   # not a multiple of P / g1 < 1
        with pytest.raises(ValueError, match="image_size_in"):
            _lib.query_workspace(cfg, 1, _lib.F32, bad)
        with pytest.raises(ValueError):
            _lib.train_workspace(cfg, 1, _lib.F32, bad)
        n = ctypes.c_size_t()
        assert _lib.lib().vitseg_query_workspace_at(_c(cfg), bad, 1, _lib.F32, ctypes.byref(n)) == _lib.ESHAPE
    # a configuration check_config rejects stays a shape error through the _at form
    bad_cfg = _lib.CConfig.from_config(cfg)
    bad_cfg.num_channels = 1
    n = ctypes.c_size_t()
    assert _lib.lib().vitseg_query_workspace_at(ctypes.byref(bad_cfg), 384, 1, _lib.F32, ctypes.byref(n)) == _lib.ESHAPE


def test_model_validation_with_and_without_the_flag():
    m = ViTSegmentationModel(2, 16, 192, 1, 3).eval()
    with pytest.raises(TypeError):
        m(torch.zeros(1, 3, 224, 224), interpolate_position_encoding=True)   # (HF's keyword name only)
    # a legal other size gets past the size checks and meets the device check
    for S in (384, 160, 16):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m(torch.zeros(1, 3, S, S), interpolate_pos_encoding=True)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            m.predict_mask(torch.zeros(1, 3, S, S), interpolate_pos_encoding=True)
    with pytest.raises(ValueError, match="square"):
        m(torch.zeros(1, 3, 384, 320), interpolate_pos_encoding=True)
    with pytest.raises(ValueError, match="multiple of the patch size"):
        m(torch.zeros(1, 3, 200, 200), interpolate_pos_encoding=True)
    with pytest.raises(ValueError, match="multiple of the patch size"):
        m(torch.zeros(1, 3, 8, 8), interpolate_pos_encoding=True)
    with pytest.raises(ValueError, match="channel dimension"):
        m(torch.zeros(1, 1, 384, 384), interpolate_pos_encoding=True)
    # without the flag: the existing error, unchanged
    with pytest.raises(ValueError, match=r"Input image size \(384\*384\) doesn't match model \(224\*224\)\."):
        m(torch.zeros(1, 3, 384, 384))
    with pytest.raises(ValueError, match="predict_mask_graphed"):
        m.predict_mask_graphed(torch.zeros(1, 3, 384, 384), interpolate_pos_encoding=True)
    with pytest.raises(ValueError, match="doesn't match model"):
        m.predict_mask_graphed(torch.zeros(1, 3, 384, 384))


def test_lightning_flag_is_keyword_only_and_reaches_the_model():
    with pytest.raises(TypeError):
        LightningViTModel(2, 16, 192, 1, 3, True)
    lm = LightningViTModel(2, 16, 192, 1, 3, interpolate_pos_encoding=True)
    assert lm.interpolate_pos_encoding and lm.model.cfg.image_size == 224
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lm(torch.zeros(1, 3, 320, 320))
    assert not LightningViTModel(2, 16, 192, 1, 3).interpolate_pos_encoding


def test_worker_model_spec_sixth_field():
    assert parse_model_spec("3:2:/c/v.ckpt:0:224:512") == dict(model_id=3, num_classes=2, checkpoint="/c/v.ckpt",
                                                               config_id=0, image_size=224, serve_size=512)
    m = parse_model_spec("0:17")
    assert (m["checkpoint"], m["config_id"], m["image_size"], m["serve_size"]) == (None, 0, 224, None)
    assert parse_model_spec("1:2::4:224")["serve_size"] is None


# ---- numpy restatement of torch's bicubic (align_corners=False, A = -0.75, clamped taps) ----------------------------
def _fma(a, b, c):
    """fp32 fused multiply-add (the float64 product of two fp32 values is exact)."""
    return (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32)


def cubic_taps(out, inp):
    """first tap [out] and weights [out, 4] as torch's CPU kernel computes them: fp32, multiply-adds fused (the kernels
    do the same with fmaf)."""
    f = np.float32
    scale = f(inp) / f(out)
    real = _fma(scale, np.arange(out, dtype=np.float32) + f(0.5), f(-0.5))
    i0 = np.minimum(np.floor(real).astype(np.int64), inp - 1)
    t = np.clip(real - i0.astype(np.float32), f(0), f(1)).astype(np.float32)
    A = f(-0.75)

    def c1(x):
        return _fma(_fma(A + f(2), x, -(A + f(3))) * x, x, f(1))

    def c2(x):
        return _fma(_fma(_fma(A, x, -f(5) * A), x, f(8) * A), x, -f(4) * A)

    w = np.stack([c2(t + f(1)), c1(t), c1(f(1) - t), c2((f(1) - t) + f(1))], axis=1).astype(np.float32)
    return i0 - 1, w


def interp_matrix(out, inp):
    """[out, inp] float64 matrix of the 1-D resampling (clamped taps that land on one index summed)."""
    first, w = cubic_taps(out, inp)
    M = np.zeros((out, inp))
    for o in range(out):
        for k in range(4):
            M[o, min(max(first[o] + k, 0), inp - 1)] += w[o, k]
    return M


def np_pos_interp(table, g0, g1):
    """[1 + g1^2, D] from [1 + g0^2, D]: CLS row copied, the grid resampled (x taps inside, y taps outside)."""
    D = table.shape[1]
    M = interp_matrix(g1, g0)
    grid = table[1:].reshape(g0, g0, D).astype(np.float64)
    out = np.einsum("ay,bx,yxd->abd", M, M, grid).reshape(g1 * g1, D)
    return np.concatenate([table[:1].astype(np.float64), out])


def torch_pos_interp(table, g0, g1):
    """HF ViTEmbeddings.interpolate_pos_encoding's arithmetic (the part after its early return)."""
    D = table.shape[-1]
    t = torch.as_tensor(table)
    grid = t[1:].reshape(1, g0, g0, D).permute(0, 3, 1, 2)
    grid = F.interpolate(grid, size=(g1, g1), mode="bicubic", align_corners=False)
    return torch.cat([t[:1], grid.permute(0, 2, 3, 1).reshape(g1 * g1, D)])


GRIDS = [(14, 32), (14, 24), (14, 7), (28, 64), (14, 14), (14, 20), (28, 40), (14, 10)]


@pytest.mark.parametrize("g0,g1", GRIDS)
def test_numpy_restatement_agrees_with_torch(g0, g1):
    """The taps and weights the kernels use, restated, against torch's CPU F.interpolate: this sizes the GPU tolerance
    (1e-6 of max|table|).  The restatement sums in float64, torch in fp32."""
    rng = np.random.default_rng(g0 * 100 + g1)
    D = 64
    table = (rng.standard_normal((1 + g0 * g0, D)) * 0.02).astype(np.float32)
    ref = np_pos_interp(table, g0, g1)
    got = torch_pos_interp(table, g0, g1).numpy().astype(np.float64)
    scale = np.abs(table).max()
    assert np.abs(got - ref).max() <= 1e-6 * scale, np.abs(got - ref).max() / scale
    if g0 == g1:
        assert np.array_equal(interp_matrix(g1, g0), np.eye(g0))   # weights (0, 1, 0, 0): the identity


@pytest.mark.parametrize("g0,g1", GRIDS)
def test_numpy_adjoint_is_the_transpose(g0, g1):
    """The backward pass of the resampling = the transposed matrices applied y then x (what the adjoint kernel sums,
    clamped border taps merged), checked against fp64 autograd through F.interpolate."""
    rng = np.random.default_rng(7 + g1)
    D = 8
    dout = rng.standard_normal((1 + g1 * g1, D))
    leaf = torch.zeros(1 + g0 * g0, D, dtype=torch.float64, requires_grad=True)
    (torch_pos_interp(leaf, g0, g1) * torch.from_numpy(dout)).sum().backward()
    M = interp_matrix(g1, g0)
    grid = dout[1:].reshape(g1, g1, D)
    T = np.einsum("bx,abd->axd", M, grid)          # pass 1: over x
    din = np.einsum("ay,axd->yxd", M, T)           # pass 2: over y
    ref = np.concatenate([dout[:1], din.reshape(g0 * g0, D)])
    # torch's float64 weights differ from the fp32 ones in the last fp32 bits: measured up to 1.7e-6 of the gradient's
    # max, the scale of the GPU adjoint's 1e-5 gate
    assert np.abs(leaf.grad.numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
